"""fc_message[0] folded into the V projection (DESIGN.md §5 "The V fold"; run with -m gpu).

The plans whose pointwise chain is the register-chained one (fused, and the
split plans from 320 chain workgroups on) project V' = (W0 Wv) x, 64 channels,
accumulate a 64-channel O and start the message chain at fc0's BatchNorm / ReLU
with bias W0 bv + b0.  The weights here make a wrong fold visible: V and fc0
biases of O(1), fc0 BatchNorm running means away from 0 and variances away from 1
(a dropped W0 bv term or a misplaced BatchNorm fold moves every feature by O(1)).

FUSED_SHAPE: the smallest batch of the fused plan at N = 250 (one partial key
tile): 160 pairs x 2 chain workgroups = the 320-workgroup rule of use_pw2.  (40 x 256
is 80 workgroups: not fused.)"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ENVELOPE, FEAT_FLOOR, GOLDEN, LOGIT_FLOOR, encoder_torch, fp32_envelope
from parity_rules import NearTieTally, held_to_oracle

pytestmark = pytest.mark.gpu

LAYERS = 4
FUSED_SHAPE = (160, 250)
SHAPES = [(1, 200), (1, 333), (1, 1000), (3, 160), FUSED_SHAPE]
PARENT = os.path.join(GOLDEN, "vfold", "parent.npz")  # our own outputs at the commit before the fold (_record_parent)
_CACHE = {}


def _state_dict():
    """synthetic_state_dict with O(1) V / fc0 biases and fc0 BatchNorm statistics far from (0, 1)."""
    from pointdsc_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(LAYERS, seed=5)
    rng = np.random.RandomState(50)
    for i in range(LAYERS):
        p = f"encoder.blocks.NonLocal_layer_{i}"
        sd[p + ".projection_v.bias"] = rng.uniform(-1.5, 1.5, 128).astype(np.float32)
        sd[p + ".fc_message.0.bias"] = rng.uniform(-1.5, 1.5, 64).astype(np.float32)
        sd[p + ".fc_message.1.running_mean"] = rng.uniform(-1.0, 1.0, 64).astype(np.float32)
        sd[p + ".fc_message.1.running_var"] = rng.uniform(0.1, 6.0, 64).astype(np.float32)
    return sd


def _model(dev, precision="h3"):
    from pointdsc_amd.PointDSC import PointDSC
    m = PointDSC(in_dim=6, num_layers=LAYERS, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                 sigma_d=0.10, k=40, nms_radius=0.10, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state_dict().items()})
    return m.to(dev).eval()


def _batch(B, N, dev):
    from pointdsc_amd.synthetic import synthetic_batch
    b = synthetic_batch(B, N, seed=31)
    return b, tuple(torch.from_numpy(b[k]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))


def _outputs(dev, B, N, precision="h3"):
    """Encoder (the caller's dense M) and testing-forward (packed M) outputs."""
    from pointdsc_amd import kernels
    m = _model(dev, precision)
    cfg, packed = m.pdsc_config(), m.packed_weights()
    _, (corr, src, tgt) = _batch(B, N, dev)
    M = kernels.compat(src, tgt, torch.tensor([0.10], device=dev))
    feat, normed, conf = kernels.encoder(cfg, packed, corr, M)
    T, L, fconf, seeds = kernels.forward_testing(cfg, packed, corr, src, tgt, debug=True)
    return {k: v.cpu().numpy() for k, v in dict(feat=feat, normed=normed, conf=conf, T=T, L=L, fconf=fconf,
                                                  seeds=seeds).items()}


def _attention_outputs(dev, N=200):
    from pointdsc_amd import kernels
    g = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(1, N, 128, generator=g).to(dev) for _ in range(3))
    _, (_, src, tgt) = _batch(1, N, dev)
    M = kernels.compat(src, tgt, torch.tensor([0.10], device=dev))
    return kernels.attention(q, k, v, M).cpu().numpy()


def _vfold(B, N, precision=0):
    """EncoderPlan::vfold of the forward's plan for (B, N) in this process."""
    from pointdsc_amd import _lib
    v = ctypes.c_int32()
    _lib.check(_lib.load().pdsc_encoder_plan_vfold(B, N, precision, ctypes.byref(v)), "encoder_plan_vfold")
    return v.value


def _dump(path, B, N):  # child process entry (knobs set by the parent process)
    np.savez(path, vfold=np.int32(_vfold(B, N)), **_outputs(torch.device("cuda:0"), B, N))


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def _record_parent(path=PARENT):
    """Writes the golden of test_knob_restores_parent / test_standalone_attention_unchanged;
    run once, at the commit before the fold: at FUSED_SHAPE every output's SHA-256,
    and the logits and poses themselves."""
    dev = torch.device("cuda:0")
    o = _outputs(dev, *FUSED_SHAPE)
    out = {"sha_" + k: _sha(v) for k, v in o.items()}
    out.update(knob_conf=o["conf"], knob_T=o["T"], attention_200=_attention_outputs(dev))
    np.savez_compressed(path, **out)


def _child(tmp_path, name, B, N, **env):
    here = os.path.dirname(os.path.abspath(__file__))
    out = tmp_path / f"{name}.npz"
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; " \
           f"import test_gpu_vfold as t; t._dump({str(out)!r}, {B}, {N})"
    subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), check=True, timeout=240)
    return np.load(out)


def _case(b, i):
    """Pair i of a batch as a conftest case; the plain-order torch fp32 evaluation stands for the reference's outputs."""
    sd = _state_dict()
    g = {"corr_pos": b["corr_pos"][i], "src_keypts": b["src_keypts"][i], "tgt_keypts": b["tgt_keypts"][i],
         "sigma_d": np.float32(0.10), "num_layers": LAYERS, "corr_features": np.zeros((0, 128), np.float32)}
    g["confidence"] = encoder_torch(g, sd, torch.device("cuda:0"), torch.float32)[1]
    return g, sd


@pytest.mark.parametrize("precision", ["h3", "f32"])
@pytest.mark.parametrize("B,N", SHAPES)
def test_encoder_vs_fp64(B, N, precision, gpu_device):
    """Features and logits within ENVELOPE x the case's fp32 noise of the fp64
    evaluation of the reference formula (conftest.fp32_envelope), in both modes."""
    from pointdsc_amd import _lib, kernels
    if (B, N) == FUSED_SHAPE:
        fused = ctypes.c_int32()
        _lib.check(_lib.load().pdsc_encoder_plan(B, N, 0, ctypes.byref(fused)), "encoder_plan")
        assert fused.value == 1, (B, N)
    # the fold as built covers the register-chained plans: of the issue's shapes, the fused one in h3
    assert _vfold(B, N, 1 if precision == "f32" else 0) == int((B, N) == FUSED_SHAPE and precision == "h3")
    m = _model(gpu_device, precision)
    b, (corr, src, tgt) = _batch(B, N, gpu_device)
    M = kernels.compat(src, tgt, torch.tensor([0.10], device=gpu_device))
    feat, _, conf = kernels.encoder(m.pdsc_config(), m.packed_weights(), corr, M)
    for i in sorted({0, B // 3, B - 1}):
        if (B, N, i) not in _CACHE:  # the yardstick once per pair, shared by both modes
            g, sd = _case(b, i)
            _CACHE[(B, N, i)] = fp32_envelope(g, sd, gpu_device)
        e_f, e_c, f64, c64, mx = _CACHE[(B, N, i)]
        ours_c = np.abs(conf[i].double().cpu().numpy() - c64).max()
        ours_f = np.abs(feat[i].double().cpu().numpy() - f64).max() / mx
        print(f"vfold {precision} {B}x{N} pair {i}: logits {ours_c:.3g} (noise {e_c:.3g}), features {ours_f:.3g} ({e_f:.3g})")
        assert ours_c <= ENVELOPE * e_c + LOGIT_FLOOR, (i, ours_c, e_c)
        assert ours_f <= ENVELOPE * e_f + FEAT_FLOOR, (i, ours_f, e_f)


def test_fused_equals_split_launches(gpu_device, tmp_path):
    """The folded fused kernels against the folded split launches (PDSC_FUSE=0 in a
    child process, split grid as test_fused_encoder_bit_identical): the same bits."""
    B, N = FUSED_SHAPE
    ours = _outputs(gpu_device, B, N)
    assert _vfold(B, N) == 1
    ref = _child(tmp_path, "unfused", B, N, PDSC_VFOLD="1", PDSC_FUSE="0", PDSC_W64_SK="0")
    assert int(ref["vfold"]) == 1  # the split plan (attention_w64 on the forward's packed M) folds too
    for k, v in ours.items():
        assert np.array_equal(v, ref[k]), k


def test_fold_changes_only_rounding(gpu_device, tmp_path):
    """PDSC_VFOLD=0 at the fused shape: another fp32 realisation of the same function
    (a dropped bias term would be O(1) here), so features agree to fp32 noise but not bitwise."""
    B, N = FUSED_SHAPE
    ours = _outputs(gpu_device, B, N)
    ref = _child(tmp_path, "unfolded", B, N, PDSC_VFOLD="0")
    assert _vfold(B, N) == 1 and int(ref["vfold"]) == 0
    assert not np.array_equal(ours["feat"], ref["feat"])  # the fold is on by default at this shape
    assert np.abs(ours["feat"] - ref["feat"]).max() <= 1e-4 * np.abs(ref["feat"]).max()


def test_knob_restores_parent(gpu_device, tmp_path):
    """PDSC_VFOLD=0 at FUSED_SHAPE, where the plan folds by default: bitwise the
    outputs recorded before the fold (every output's SHA-256; logits and poses raw)."""
    B, N = FUSED_SHAPE
    assert _vfold(B, N) == 1
    ref = np.load(PARENT)
    ours = _child(tmp_path, "knob", B, N, PDSC_VFOLD="0")
    assert int(ours["vfold"]) == 0
    assert np.array_equal(ours["conf"], ref["knob_conf"]) and np.array_equal(ours["T"], ref["knob_T"])
    for k in ("feat", "normed", "conf", "T", "L", "fconf", "seeds"):
        assert np.array_equal(_sha(ours[k]), ref["sha_" + k]), k


def test_standalone_attention_unchanged(gpu_device):
    """pdsc_attention takes the caller's 128-channel V: bitwise the outputs recorded before the fold."""
    assert np.array_equal(_attention_outputs(gpu_device), np.load(PARENT)["attention_200"])


def _trained(dev):
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.synthetic import BENCH_CLS, PRESETS, trained_state_dict
    p = PRESETS["3dmatch"]
    m = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40, nms_radius=p["nms_radius"])
    sd = trained_state_dict("3dmatch", 12, *BENCH_CLS)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(dev).eval(), sd


RAGGED_SIZES = (130, 257, 64, 1000)


def _ragged(m, ps, dev):
    from pointdsc_amd import kernels
    ds = [{k: torch.from_numpy(q[k])[None].to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")} for q in ps]
    corr, counts = kernels.pad_pairs([d["corr_pos"] for d in ds])
    src, _ = kernels.pad_pairs([d["src_keypts"] for d in ds])
    tgt, _ = kernels.pad_pairs([d["tgt_keypts"] for d in ds])
    T, L, st = kernels.forward_ragged(m.pdsc_config(), m.packed_weights(), corr, src, tgt, counts, debug=True)
    return ds, counts, T, L, {k: v.cpu().numpy() for k, v in st.items()}


def test_ragged_vs_single_pairs(gpu_device, capsys):
    """One ragged batch of sizes 130, 257, 64, 1000 (a small-batch plan: no fold)
    against the pairs' own forwards and the oracle by the near-tie rule."""
    from pointdsc_amd.synthetic import synthetic_pair
    m, sd = _trained(gpu_device)
    ps = [synthetic_pair(n, 88000 + i) for i, n in enumerate(RAGGED_SIZES)]
    assert _vfold(len(ps), max(RAGGED_SIZES)) == 0
    ds, counts, T, L, st = _ragged(m, ps, gpu_device)
    tally = NearTieTally("test_ragged_vs_single_pairs")
    for b, (q, n, d) in enumerate(zip(ps, counts, ds)):
        S = int(n * 0.1)
        one = m(dict(d, testing=True))
        assert torch.equal(one["final_labels"][0], L[b, :n]), b  # labels bitwise the pair's own forward
        held_to_oracle(q, L[b, :n].cpu().numpy(), T[b].cpu().numpy(), st["conf"][b, :n], st["seeds"][b, :S],
                       st["knn"][b, :S], sd, gpu_device, f"pair {b} (N={n})", tally=tally, num_layers=12)
    tally.finish(capsys)


def test_ragged_folded_batch(gpu_device, capsys):
    """The same four sizes ten times over: 40 pairs at stride 1000 are the fused plan
    (320 chain workgroups), run as ragged halves with pw2_first's early exit past a
    short pair's rows -- the folded kernels on a ragged batch.  Copies of a pair give
    the same bits wherever they sit in the batch; one copy of each is held to the oracle."""
    from pointdsc_amd.synthetic import synthetic_pair
    m, sd = _trained(gpu_device)
    four = [synthetic_pair(n, 88000 + i) for i, n in enumerate(RAGGED_SIZES)]
    ps = four * 10
    assert _vfold(len(ps), max(RAGGED_SIZES)) == 1
    ds, counts, T, L, st = _ragged(m, ps, gpu_device)
    tally = NearTieTally("test_ragged_folded_batch")
    for b, (q, n) in enumerate(zip(ps, counts)):
        S = int(n * 0.1)
        if b >= 4:
            assert torch.equal(T[b], T[b % 4]) and torch.equal(L[b], L[b % 4]), b
            assert np.array_equal(st["conf"][b, :n], st["conf"][b % 4, :n]), b
            continue
        held_to_oracle(q, L[b, :n].cpu().numpy(), T[b].cpu().numpy(), st["conf"][b, :n], st["seeds"][b, :S],
                       st["knn"][b, :S], sd, gpu_device, f"pair {b} (N={n})", tally=tally, num_layers=12)
    tally.finish(capsys)


def _planes(blob, off, out, inn):
    """A packed dense block read back: (hi + mid) 2^-s as fp64 [out][in] (w3_index, pdsc_internal.hpp)."""
    halfs = blob[off[0]:off[0] + out * inn].view(np.float16).astype(np.float64)
    o, c = np.meshgrid(np.arange(out), np.arange(inn), indexing="ij")
    q = c & 15
    pos = (q & ~12) | ((q & 4) << 1) | ((q & 8) >> 1)
    idx = ((o >> 5) * (inn // 16) + (c >> 4)) * 1024 + (32 * (pos >> 3) + (o & 31)) * 8 + (pos & 7)
    return (halfs[idx] + halfs[idx + 512]) * float(blob[off[4]])


def test_pack_folded_block(gpu_device):
    """pdsc_pack_weights' vm block read back (the pack runs on the device, hence a GPU
    test): bias = W0 bv + b0 and the packed W0 Wv against the fp64 products rounded
    once (summed in the kernel's order, so the fp32 values are equal bit for bit),
    BatchNorm coefficients fc0's own.  The planes hold x = Wm 2^s as hi + mid, two
    fp16 roundings of 11 significant bits each: |x - hi - mid| <= 2^-22 |x| while mid
    is a normal fp16, and at most 2^-25 (half the smallest subnormal) otherwise, which
    for a block scaled to [2^13, 2^14) is below 2^-22 of any row maximum above 2^-3.
    With Wm's own fp32 rounding (2^-24 |x|) that is inside 2^-21 of the row's
    max |Wm|; the same bound is asserted on PointCN's block of the same pack."""
    from pointdsc_amd import _lib
    m = _model(gpu_device)
    cfg, blob = m.pdsc_config(), m.packed_weights().cpu().numpy()
    sd = _state_dict()
    lib = _lib.load()

    def block(layer, which):
        off = (ctypes.c_size_t * 5)()
        _lib.check(lib.pdsc_packed_block(ctypes.byref(cfg), layer, which, off), "packed_block")
        return list(off)

    for l in range(LAYERS):
        p = f"encoder.blocks.NonLocal_layer_{l}"
        w0 = sd[p + ".fc_message.0.weight"][:, :, 0].astype(np.float64)
        wv = sd[p + ".projection_v.weight"][:, :, 0].astype(np.float64)
        wm, bm = np.zeros((64, 128)), sd[p + ".fc_message.0.bias"].astype(np.float64)
        for j in range(128):  # fold_vm_kernel's order
            wm = wm + np.outer(w0[:, j], wv[j])
            bm = bm + w0[:, j] * np.float64(sd[p + ".projection_v.bias"][j])
        wm32, vm, fc0 = wm.astype(np.float32), block(l, 7), block(l, 1)
        assert np.array_equal(blob[vm[1]:vm[1] + 64], bm.astype(np.float32)), l
        assert np.array_equal(blob[vm[2]:vm[2] + 64], blob[fc0[2]:fc0[2] + 64]), l  # alpha
        assert np.array_equal(blob[vm[3]:vm[3] + 64], blob[fc0[3]:fc0[3] + 64]), l  # beta
        s = float(blob[vm[4] + 1])  # 2^s, from max |Wm|
        assert 2.0 ** 13 <= np.abs(wm32).max() * s < 2.0 ** 14 and blob[vm[4]] * s == 1.0, l
        for name, got, want in (("vm", _planes(blob, vm, 64, 128), wm),
                                ("pcn", _planes(blob, block(l, 0), 128, 128),
                                 sd[f"encoder.blocks.PointCN_layer_{l}.0.weight"][:, :, 0].astype(np.float64))):
            bound = 2.0 ** -21 * np.abs(want).max(1, keepdims=True)
            assert (np.abs(got - want) <= bound).all(), (l, name, float((np.abs(got - want) / bound).max()))
        # the fp32 value the planes were split from is the fp64 product rounded once
        assert (np.abs(_planes(blob, vm, 64, 128) - wm32) <= 2.0 ** -22 * np.abs(wm32).max()).all(), l
