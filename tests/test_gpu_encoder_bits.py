"""The encoder row's entries and the forwards' encoder stage, bit for bit against
a recording (tests/golden/encoder_bits/encoder_bits.json).

As test_gpu_tail_bits.py holds the tail to itself, this holds the encoder row
(weight packing, the standalone encoder and attention entries, the encoder
stage inside the testing forwards): a SHA-256 per output tensor of a fixed set
of calls must equal what an earlier build of the same sources produced.  Moving
a kernel, a launcher, the run loop or an entry point between files changes no
arithmetic, no launch shape and no plan, so no bit may move.

The recording is tied to the toolchain.  Only a commit that MEANS to change the
encoder's numerics, or a ROCm update, re-records it:
`python tests/test_gpu_encoder_bits.py --write` on the GPU (PDSC_LIB_VARIANT
selects the build to record from).  Write it twice and compare the two files
before committing.

Cases (3 layers: pw_first, pw_mid / attn_pw2 and pw_last / attn_pw2_last all
run, and the zigzag order takes both parities; in_dim = 6).  A case with knobs
runs in a fresh child process (the knobs are read once per process).  The plan
each case is named after, from plan_encoder's rules (test_case_plans asserts
what the host-only queries can tell):
  fused       160 x 256: 320 tiles of 128 points, one key split -> ATT_FUSED,
              packed M, vfold; the ragged form (counts 256 / 200 alternating)
              runs as two parts on two streams (B >= 32), and with every count
              256 takes rg.eq
  fused_novf  the same with PDSC_VFOLD=0
  fused_dense the same with PDSC_DENSE_M=1 (dense M behind the fused kernels)
  unfused     the same with PDSC_FUSE=0 PDSC_W64_SK=0: pw2 chain + the split
              attention on the split grid (ATT_W64), vfold behind it
  unfused_sk  PDSC_FUSE=0 alone: the stream-K form where the rule takes it; its
              ragged batch turns stream-K back into the split grid, rg.eq keeps it
  w64         128 x 256: attention_w64 behind the LDS-tiled chain (64-point tiles)
  tiny        1 x 1000: the tiny wave-split plan (ATT_H3_WS, 4 waves), 32-point
              tiles, the 8-wave pw_mid with the Q/K/V split and the prefetch
  tiny_ws2    PDSC_ATT_WS=2; tiny_off: PDSC_ATT_TINY=0 (ATT_H3 at PDSC_ATT_NW's 2 waves)
  tiny_nw1/4  PDSC_ATT_TINY=0 with PDSC_ATT_NW=1 / 4
  tiny_plain  PDSC_PW_QKV_SPLIT=0 PDSC_PW_PREFETCH=0 PDSC_PRECOMBINE=0
  early_nw1/2 1 x 2000, PDSC_ATT_TINY=0, PDSC_ATT_NW=1 / 2: splits of 8 / 4 tiles,
              so ATT_H3 with the early-issue loop at 1 and 2 waves
  unfused_h3  160 x 256, PDSC_FUSE=0 PDSC_W64=0: the forward runs the folded
              attention_h3_kernel<4, CH2> on packed M behind the pw2 chain
  w64_forced  3 x 160, PDSC_W64=1: attention_w64 behind the 32-point LDS chain
  f32         1 x 200 and 3 x 160 in PDSC_PRECISION_F32 (ATT_F32)

Which entry reaches which form.  The plans above are the FORWARD's (packed M,
or dense under PDSC_DENSE_M=1): outputs fwd_*.  The standalone encoder (feat,
normed, conf) plans on the caller's dense M and never runs attention_w64: at
160 x 256 it is fused on dense M by default, and under PDSC_FUSE=0 (unfused*,
unfused_h3) it runs the folded attention_h3_kernel<4, CH2> on dense M; at
128 x 256 and 3 x 160 it runs ATT_H3 where the forward runs attention_w64.  The
standalone attention (msg) is always the split launch on dense M, unfolded:
ATT_H3 at 4 waves with the early loop at 160 x 256 (8 tiles, one split), the
case's own ATT_H3 / ATT_H3_WS form at 1 x 1000 and 1 x 2000, ATT_F32 for f32.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

FIXTURE = os.path.join(HERE, "golden", "encoder_bits", "encoder_bits.json")
LAYERS = 3
FUSED = (160, 256)
# id -> (B, N, precision, knobs, ragged counts or None)
_RAG = [256, 200] * (FUSED[0] // 2)
CASES = {
    "fused": (*FUSED, "h3", {}, None),
    "fused_ragged": (*FUSED, "h3", {}, _RAG),
    "fused_eq": (*FUSED, "h3", {}, [256] * FUSED[0]),
    "fused_novf": (*FUSED, "h3", {"PDSC_VFOLD": "0"}, None),
    "fused_dense": (*FUSED, "h3", {"PDSC_DENSE_M": "1"}, None),
    "unfused": (*FUSED, "h3", {"PDSC_FUSE": "0", "PDSC_W64_SK": "0"}, None),
    "unfused_novf": (*FUSED, "h3", {"PDSC_FUSE": "0", "PDSC_W64_SK": "0", "PDSC_VFOLD": "0"}, None),
    "unfused_sk": (*FUSED, "h3", {"PDSC_FUSE": "0"}, None),
    "unfused_sk_ragged": (*FUSED, "h3", {"PDSC_FUSE": "0"}, _RAG),
    "unfused_sk_eq": (*FUSED, "h3", {"PDSC_FUSE": "0"}, [256] * FUSED[0]),
    "w64": (128, 256, "h3", {}, None),
    "tiny": (1, 1000, "h3", {}, None),
    "tiny_ws2": (1, 1000, "h3", {"PDSC_ATT_WS": "2"}, None),
    "tiny_off": (1, 1000, "h3", {"PDSC_ATT_TINY": "0"}, None),
    "tiny_nw1": (1, 1000, "h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "1"}, None),
    "tiny_nw4": (1, 1000, "h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "4"}, None),
    "tiny_plain": (1, 1000, "h3", {"PDSC_PW_QKV_SPLIT": "0", "PDSC_PW_PREFETCH": "0", "PDSC_PRECOMBINE": "0"}, None),
    "early_nw1": (1, 2000, "h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "1"}, None),
    "early_nw2": (1, 2000, "h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "2"}, None),
    "unfused_h3": (*FUSED, "h3", {"PDSC_FUSE": "0", "PDSC_W64": "0"}, None),
    "w64_forced": (3, 160, "h3", {"PDSC_W64": "1"}, None),
    "f32_1x200": (1, 200, "f32", {}, None),
    "f32_3x160": (3, 160, "f32", {}, None),
}
PACK_CASES = [(p, L) for p in ("h3", "f32") for L in (1, 3)]
# What the host-only queries must say of each case under its knobs (plan_of), from
# plan_encoder's rules.  kind (pdsc_encoder_plan): 1 fused, 2 attention_w64, 0 the
# split h3 / f32 launches.  nsplit (pdsc_attention_layout): the workspace's partial
# slots.  160 x 256 has 8 key tiles per pair, so the split grids take one split;
# the stream-K form shows as MORE slots (its segments') than the split grid's.
_PW2 = dict(pw2=1, pw_tile=0)                                                    # 320 tiles of 128 points
_LDS32 = dict(pw2=0, pw_tile=32, pw_mid8=1, pw_first_qkv3=1, pw_mid_qkv3=1, pw_prefetch=1)  # <= 256 workgroups
_FUSED = dict(kind=1, vfold=1, nsplit=1, **_PW2)
_SK = dict(kind=2, vfold=1, nsplit=3, **_PW2)  # 1280 tiles over 256 workgroups: 5 + 2 < 8, stream-K; 3 segment slots
_TINY = dict(kind=0, vfold=0, **_LDS32)
PLANS = {
    "fused": _FUSED, "fused_ragged": _FUSED, "fused_eq": _FUSED,
    "fused_novf": dict(_FUSED, vfold=0),
    "fused_dense": _FUSED,  # (M's layout is not in the queries: PDSC_DENSE_M moves no plan field they show)
    "unfused": dict(kind=2, vfold=1, nsplit=1, **_PW2),       # PDSC_W64_SK=0: the split grid's one split
    "unfused_novf": dict(kind=2, vfold=0, nsplit=1, **_PW2),
    "unfused_sk": _SK, "unfused_sk_ragged": _SK, "unfused_sk_eq": _SK,
    "unfused_h3": dict(kind=0, vfold=1, nsplit=1, **_PW2),    # PDSC_W64=0: attention_h3_kernel<4, CH2> on packed M
    # 128 blocks of 256 queries: attention_w64 (stream-K: 1024 tiles, 4 + 2 < 8; 2 slots) behind 64-point tiles
    "w64": dict(kind=2, vfold=0, nsplit=2, pw2=0, pw_tile=64, pw_mid8=0),
    "w64_forced": dict(kind=2, vfold=0, **_LDS32),
    # 1 x 1000: 8 blocks of 128 queries <= PDSC_ATT_TINY = 16: 32 blocks x 4 splits of 8 tiles, WS waves per split
    "tiny": dict(_TINY, nsplit=4), "tiny_ws2": dict(_TINY, nsplit=4),
    # PDSC_ATT_TINY=0: attention_h3_kernel<nw> at 16 splits of 2 tiles (early needs >= 3: the plain loop)
    "tiny_off": dict(_TINY, nsplit=16), "tiny_nw1": dict(_TINY, nsplit=16), "tiny_nw4": dict(_TINY, nsplit=16),
    "tiny_plain": dict(kind=0, vfold=0, nsplit=4, pw2=0, pw_tile=32, pw_mid8=1, pw_first_qkv3=0, pw_mid_qkv3=0,
                       pw_prefetch=0),
    # 1 x 2000: 63 key tiles in 8 / 16 splits of 8 / 4 tiles (>= 3): attention_h3_kernel<nw, EARLY>
    "early_nw1": dict(_TINY, nsplit=8), "early_nw2": dict(_TINY, nsplit=16),
    "f32_1x200": dict(kind=0, vfold=0, pw2=0, pw_tile=32, pw_mid8=0, pw_first_qkv3=0),
    "f32_3x160": dict(kind=0, vfold=0, pw2=0, pw_tile=32, pw_mid8=0, pw_first_qkv3=0),
}


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _model(dev, precision, layers=LAYERS):
    import torch
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.synthetic import synthetic_state_dict
    m = PointDSC(in_dim=6, num_layers=layers, num_channels=128, num_iterations=10, ratio=0.1, inlier_threshold=0.10,
                 sigma_d=0.10, k=40, nms_radius=0.10, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(layers, seed=5).items()})
    return m.to(dev).eval()


def run_pack(dev, precision, layers):
    return {"packed": _sha(_model(dev, precision, layers).packed_weights())}


def run_case(dev, cid):
    import torch
    from pointdsc_amd import kernels as K
    from pointdsc_amd.synthetic import synthetic_batch
    B, N, precision, _, counts = CASES[cid]
    m = _model(dev, precision)
    cfg, packed = m.pdsc_config(), m.packed_weights()
    b = synthetic_batch(B, N, seed=31)
    corr, src, tgt = (torch.from_numpy(b[k]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    out = {}
    if counts is None:
        M = K.compat(src, tgt, torch.tensor([0.10], device=dev))
        feat, normed, conf = K.encoder(cfg, packed, corr, M)
        g = torch.Generator().manual_seed(9)
        q, k, v = (torch.randn(B, N, 128, generator=g).to(dev) for _ in range(3))
        out.update(feat=feat, normed=normed, conf=conf, msg=K.attention(q, k, v, M, precision))
        out.update({"fwd_" + k: v for k, v in K.forward_stages(cfg, packed, corr, src, tgt).items()})
    else:
        T, L, st = K.forward_ragged(cfg, packed, corr, src, tgt, counts, debug=True)
        out.update(final_trans=T, trans_pre_refine=st["trans_pre_refine"])
        for i in (0, 1, B - 2, B - 1):  # a pair's own rows (the rest of the stride is never written); both parts
            n = counts[i]
            S = int(n * 0.1)
            out.update({f"conf{i}": st["conf"][i, :n], f"labels{i}": L[i, :n], f"seeds{i}": st["seeds"][i, :S],
                        f"knn{i}": st["knn"][i, :S], f"weights{i}": st["weights"][i, :S]})
    return {k: _sha(v) for k, v in out.items()}


def plan_of(cid):
    """What the host-only queries say of the case's shape under this process's knobs."""
    import ctypes
    import torch  # noqa: F401  (before libpdsc.so: the process's HIP runtime is torch's, as in every GPU test)
    from pointdsc_amd import _lib
    L = _lib.load()
    B, N, precision, _, _ = CASES[cid]
    pc, v, w = _lib.precision_code(precision), ctypes.c_int32(), ctypes.c_int32()
    out = {}
    _lib.check(L.pdsc_encoder_plan(B, N, pc, ctypes.byref(v)), "encoder_plan")
    out["kind"] = v.value  # 1 fused, 2 attention_w64, 0 the split h3 / f32 launches
    _lib.check(L.pdsc_encoder_plan_vfold(B, N, pc, ctypes.byref(v)), "encoder_plan_vfold")
    out["vfold"] = v.value
    _lib.check(L.pdsc_attention_layout(B, N, pc, ctypes.byref(v), ctypes.byref(w)), "attention_layout")
    out["Npad"], out["nsplit"] = v.value, w.value
    row = (ctypes.c_int32 * 13)()
    _lib.check(L.pdsc_launch_plan(_lib.make_config(num_layers=LAYERS, precision=precision), B, N, row, 13), "launch_plan")
    out.update(zip(("pw2", "pw_tile", "pw_mid8", "pw_first_qkv3", "pw_mid_qkv3", "pw_prefetch"), row[:6]))
    return out


def _plan_in_child(cid):
    """plan_of(cid) in a fresh process under the case's knobs (no GPU work)."""
    code = f"import sys, json; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; " \
           f"import test_gpu_encoder_bits as t; print('PLAN', json.dumps(t.plan_of({cid!r})))"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **CASES[cid][3]), check=True, timeout=120,
                       capture_output=True, text=True)
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("PLAN "))[5:])


def _in_child(cid):
    """run_case(cid) in a fresh process under the case's knobs."""
    code = f"import sys, json; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; import torch; " \
           f"import test_gpu_encoder_bits as t; print('BITS', json.dumps(t.run_case(torch.device('cuda:0'), {cid!r})))"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **CASES[cid][3]), check=True, timeout=240,
                       capture_output=True, text=True)
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("BITS "))[5:])


def _run(dev, cid):
    return _in_child(cid) if CASES[cid][3] else run_case(dev, cid)


def _pack_key(p, L):
    return f"pack:{p},{L}"


@pytest.fixture(scope="module")
def recording():
    with open(FIXTURE) as f:
        return json.load(f)


def test_recording_lists_these_cases(recording):
    assert sorted(recording) == sorted(list(CASES) + [_pack_key(p, L) for p, L in PACK_CASES])


def test_every_case_names_its_plan():
    assert sorted(PLANS) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_case_plans(cid):
    """Every case has the plan it is named after, as far as the host-only queries
    tell, under the case's own knobs (a fresh child process for a knob case): a
    knob that is misspelt or no longer read fails here, not in the hashes."""
    got = _plan_in_child(cid) if CASES[cid][3] else plan_of(cid)
    want = PLANS[cid]
    assert {k: got[k] for k in want} == want, (cid, got)


@pytest.mark.gpu
@pytest.mark.parametrize("precision,layers", PACK_CASES)
def test_pack_bits(gpu_device, recording, precision, layers):
    assert run_pack(gpu_device, precision, layers) == recording[_pack_key(precision, layers)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_encoder_bits(gpu_device, recording, cid):
    got, want = _run(gpu_device, cid), recording[cid]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    print(cid, "differing outputs:", bad or "none")
    assert not bad, f"{cid}: {bad} differ from the recording"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        import torch
        dev = torch.device("cuda:0")
        table = {cid: _run(dev, cid) for cid in CASES}
        table.update({_pack_key(p, L): run_pack(dev, p, L) for p, L in PACK_CASES})
        path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path, len(table), "cases")
    else:
        sys.exit("usage: test_gpu_encoder_bits.py --write [PATH]")
