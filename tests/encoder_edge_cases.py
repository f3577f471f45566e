"""The encoder's edge-shape cases (DESIGN.md §7 "Encoder plans: edge-shape bars"),
shared by the CPU tests (test_encoder_edge_cases.py) and the GPU tests
(test_gpu_encoder_edges.py, test_gpu_attention_edges.py).

Weights: test_gpu_vfold._state_dict's recipe at 3 layers (pw_first, the mid layer,
the last layer and both zigzag parities all run): O(1) V and fc0 biases and fc0
BatchNorm statistics away from (0, 1), so a wrong softmax denominator moves every
feature.  Inputs: synthetic_batch.

Shapes: B in {1, 3} x N in NS, plus 1 x 993 (31 key tiles plus one key; the
smallest N with 16 key splits, which the precombine rule needs), plus one ragged
batch RAGGED padded to its largest count.  N = 10 is the smallest N with a seed.

Knob sets (KNOB_SETS): each set with knobs runs in ONE fresh child process (the
library reads its knobs once) that computes every shape and writes one .npz
(child_result); `default` and `f32` run in the test process.  What a set is meant
to reach is restated from plan_encoder's rules in plan_form(), which also tells
what the host-only queries cannot (waves, the early loop, the wave split, the
precombine, stream-K); plan_queries() is what the library answers, recorded per
(set, shape) in tests/golden/encoder_edges/plans.json
(`python tests/encoder_edge_cases.py --write-plans`, no GPU needed).
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PLANS_JSON = os.path.join(HERE, "golden", "encoder_edges", "plans.json")

LAYERS = 3
IN_DIM = 6
BATCH_SEED = 31
# The 60 m extent under the model's sigma_d = 0.10: two outliers are compatible by chance
# about once in 200 pairs, so that up to N = 993 some rows have no compatible partner
# (test_encoder_edge_cases.test_case_preconditions); in the 3 m preset none has from N = 31 on.
PRESET = "kitti"
NS = (10, 31, 33, 64, 65, 127, 129, 255, 257, 513)
SHAPES = [(B, N) for B in (1, 3) for N in NS] + [(1, 993)]
RAGGED = (257, 33, 129, 10)
RAGGED_SEED = 88100
# the ragged entry needs min(k, count - 1) equal for every pair (include/pdsc.h): k = 9 with a count of 10
RAGGED_K = 9
ATT_NS = (1, 2, 31, 32, 33, 63, 65, 127, 129, 255, 257, 513)
ATT_SHAPES = [(B, N) for B in (1, 3) for N in ATT_NS] + [(1, 993)]
DEAD_NS = (33, 129, 257)   # rows and columns 0, N // 2, N - 1 of M zeroed
ZERO_NS = (31, 257)        # M == 0
ADVERSARIAL = (2, 257, 7.0, 1.0)  # B, N, sq, sk of test_attention_adversarial_magnitudes' formula

_FUSED = {"PDSC_PW2": "2", "PDSC_ATT_TARGET": "1"}
# id -> (precision, knobs)
KNOB_SETS = {
    "default": ("h3", {}),
    "f32": ("f32", {}),
    "nw2": ("h3", {"PDSC_ATT_TINY": "0"}),
    "nw1": ("h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "1"}),
    "nw4": ("h3", {"PDSC_ATT_TINY": "0", "PDSC_ATT_NW": "4"}),
    "plain": ("h3", {"PDSC_PW_QKV_SPLIT": "0", "PDSC_PW_PREFETCH": "0", "PDSC_PRECOMBINE": "0", "PDSC_PW_WAVES": "4"}),
    "tile64": ("h3", {"PDSC_PW_SMALL_LIMIT": "0"}),
    "fused": ("h3", _FUSED),
    "fused_novf": ("h3", dict(_FUSED, PDSC_VFOLD="0")),
    "fused_dense": ("h3", dict(_FUSED, PDSC_DENSE_M="1")),
    "w64": ("h3", {"PDSC_W64": "1", "PDSC_W64_SK": "0"}),
    "w64_pw2": ("h3", {"PDSC_PW2": "2", "PDSC_FUSE": "0", "PDSC_W64": "1", "PDSC_W64_SK": "0"}),
    "w64_sk": ("h3", {"PDSC_W64": "1", "PDSC_ATT_TARGET": "8"}),
}
IN_PROCESS = ("default", "f32")
ATT_SETS = ("default", "nw1", "nw2", "nw4")  # the sets that also run the standalone attention cases

# A child's time limit: 4 x the measured run of the `default`-equivalent child on the
# MI355X (2.5 s from its start to its .npz, of which 0.6 s after the imports; DESIGN.md
# §7), and not less than 60 s.
CHILD_SECONDS_MEASURED = 2.5
CHILD_TIMEOUT = max(60.0, 4 * CHILD_SECONDS_MEASURED)


def shape_key(B, N):
    return f"{B}x{N}"


RAGGED_KEY = "ragged"
RAGGED_SHAPE = (len(RAGGED), max(RAGGED))


# ------------------------------------------------------------------ weights, inputs
def state_dict(layers=LAYERS):
    """test_gpu_vfold._state_dict's recipe: synthetic_state_dict with O(1) V / fc0
    biases and fc0 BatchNorm statistics far from (0, 1)."""
    from pointdsc_amd.synthetic import synthetic_state_dict
    sd = synthetic_state_dict(layers, seed=5)
    rng = np.random.RandomState(50)
    for i in range(layers):
        p = f"encoder.blocks.NonLocal_layer_{i}"
        sd[p + ".projection_v.bias"] = rng.uniform(-1.5, 1.5, 128).astype(np.float32)
        sd[p + ".fc_message.0.bias"] = rng.uniform(-1.5, 1.5, 64).astype(np.float32)
        sd[p + ".fc_message.1.running_mean"] = rng.uniform(-1.0, 1.0, 64).astype(np.float32)
        sd[p + ".fc_message.1.running_var"] = rng.uniform(0.1, 6.0, 64).astype(np.float32)
    return sd


def batch(B, N):
    from pointdsc_amd.synthetic import synthetic_batch
    return synthetic_batch(B, N, seed=BATCH_SEED, preset=PRESET)


def ragged_pairs():
    from pointdsc_amd.synthetic import synthetic_pair
    return [synthetic_pair(n, RAGGED_SEED + i, PRESET) for i, n in enumerate(RAGGED)]


def pair_case(p):
    """One pair {corr_pos, src_keypts, tgt_keypts} as a conftest case (encoder_torch's `g`)."""
    return {"corr_pos": p["corr_pos"], "src_keypts": p["src_keypts"], "tgt_keypts": p["tgt_keypts"],
            "sigma_d": np.float32(0.10), "num_layers": LAYERS}


def case_pairs(B):
    return sorted({0, B - 1})


def all_pairs():
    """(key, pair index, case) of every pair the tests hold to the reference."""
    for B, N in SHAPES:
        b = batch(B, N)
        for i in case_pairs(B):
            yield shape_key(B, N), i, pair_case({k: b[k][i] for k in ("corr_pos", "src_keypts", "tgt_keypts")})
    for i, p in enumerate(ragged_pairs()):
        yield RAGGED_KEY, i, pair_case(p)


def sim64(f, sigma):
    """The training forward's feature-similarity M (models/PointDSC.py:158-163) in fp64."""
    n = f / np.linalg.norm(f, axis=1, keepdims=True)
    M = np.clip(1.0 - (1.0 - n @ n.T) / float(np.float32(sigma)) ** 2, 0.0, 1.0)
    np.fill_diagonal(M, 0.0)
    return M


_REFERENCE = {}


def reference(g, dev, want_M=True):
    """The yardstick of one pair, computed once per process and left unchanged: the fp64
    evaluation (f64, c64, M64) and the pair's fp32 noise -- conftest.fp32_envelope with
    one plain-order torch-fp32 run standing for the reference's own output (e_f relative
    to mx = max|f64|, e_c), and test_gpu_training._envelope's rule for M (e_m)."""
    import torch
    from conftest import encoder_torch, fp32_envelope
    key = (g["corr_pos"].tobytes(), str(dev), want_M)
    if key not in _REFERENCE:
        sd = state_dict()
        g = dict(g)
        f32, c32 = encoder_torch(g, sd, dev, torch.float32)
        g["corr_features"], g["confidence"] = f32, c32
        e_f, e_c, f64, c64, mx = fp32_envelope(g, sd, dev)
        r = dict(e_f=e_f, e_c=e_c, f64=f64, c64=c64, mx=mx)
        if want_M:
            sigma = float(np.asarray(sd["sigma"]).reshape(-1)[0])
            r["M64"] = sim64(f64, sigma)
            r["e_m"] = max(np.abs(sim64(f, sigma) - r["M64"]).max() for f in
                           [f32] + [encoder_torch(g, sd, dev, torch.float32, seed=s)[0] for s in range(4)])
        _REFERENCE[key] = r
    return _REFERENCE[key]


# ------------------------------------------------------------------ plan_encoder restated
QB, H3_TILE, W64_QPB, PW2_W, PW2_PTS, ATT_NW, ATT_F32_KTS, H3_SPLIT_C0 = 128, 32, 256, 4, 128, 4, 32, 15


def _cdiv(a, b):
    return (a + b - 1) // b


def _knobs(env):
    g = lambda n, d: int(env.get(n, d))  # noqa: E731
    t, nw, ws, sl = g("PDSC_ATT_TARGET", 0), g("PDSC_ATT_NW", 2), g("PDSC_ATT_WS", 4), g("PDSC_ATT_TINY_SLOTS", 0)
    return dict(target=t if t > 0 else 512, nw=nw if nw in (1, 2) else 4, tiny=g("PDSC_ATT_TINY", 16),
                tiny_slots=sl if sl > 0 else 128, ws=ws if ws in (1, 2) else 4, w64=g("PDSC_W64", 2),
                w64_sk=g("PDSC_W64_SK", 1) != 0, fuse=g("PDSC_FUSE", 1) != 0, precombine=g("PDSC_PRECOMBINE", 1) != 0,
                dense_m=g("PDSC_DENSE_M", 0) == 1, vfold=g("PDSC_VFOLD", 1) != 0, pw2=g("PDSC_PW2", 1),
                pw_small_limit=g("PDSC_PW_SMALL_LIMIT", 512), pw_waves8=g("PDSC_PW_WAVES", 8) != 4,
                pw_qkv_split=g("PDSC_PW_QKV_SPLIT", 1) != 0, pw_prefetch=g("PDSC_PW_PREFETCH", 1) != 0)


def _split_count(blocks, nst, slots):
    best, best_cost = 1, -1
    for ns in range(1, max(1, nst // 2) + 1):
        sps = _cdiv(nst, ns)
        if _cdiv(nst, sps) != ns:
            continue
        cost = _cdiv(blocks * ns, slots) * (sps + H3_SPLIT_C0)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = ns, cost
    return best


def _h3_grid(nw, B, N, slots):
    nqb, nst = _cdiv(N, nw * 32), _cdiv(N, H3_TILE)
    sps = _cdiv(nst, _split_count(B * nqb, nst, slots))
    return dict(nqb=nqb, sps=sps, nsplit=_cdiv(nst, sps))


def _f32_grid(B, N, target):
    nqb, nst = _cdiv(N, ATT_NW * 32), _cdiv(N, ATT_F32_KTS)
    ns = max(1, min(_cdiv(target, B * nqb), max(1, nst // 2)))
    sps = _cdiv(nst, ns)
    return dict(nqb=nqb, sps=sps, nsplit=_cdiv(nst, sps))


def _sk_nsplit(B, nqb, nst, nwg):
    T = B * nqb * nst
    owner = lambda x: ((x + 1) * nwg - 1) // T  # noqa: E731
    return max([1] + [owner(k * nst + nst - 1) - owner(k * nst) + 1 for k in range(B * nqb)])


def plan_form(B, N, precision, env, dense_m_caller=False, allow_fused=True, ragged=False):
    """plan_encoder (encoder.hip) restated: the plan of B pairs of N under the knobs
    `env`.  The defaults are the forwards' plan; dense_m_caller=True is the standalone
    encoder's, and with allow_fused=False the standalone attention's.  ragged: a ragged
    batch whose counts differ (EncoderPlan::for_ragged)."""
    k, f32 = _knobs(env), precision == "f32"
    Npad, nst, blocks = _cdiv(N, QB) * QB, _cdiv(N, H3_TILE), B * _cdiv(N, QB)
    p = dict(Npad=Npad, nw=ATT_NW, ws=1, early=False, sk=False)
    fg = _h3_grid(PW2_W, B, N, k["target"] * 4 // PW2_W)
    p["pw2"] = not f32 and k["pw2"] != 0 and (k["pw2"] == 2 or B * _cdiv(Npad, PW2_PTS) >= 320)
    fused = allow_fused and k["fuse"] and p["pw2"] and fg["nsplit"] == 1 and fg["nqb"] * PW2_PTS == Npad
    w64 = not fused and not f32 and not dense_m_caller and k["w64"] != 0 and \
        (k["w64"] == 1 or B * _cdiv(N, W64_QPB) >= 128)
    if f32:
        p.update(kind="ATT_F32", **_f32_grid(B, N, k["target"]))
    elif w64:
        nwg = k["target"] // 2
        g = _h3_grid(W64_QPB // 32, B, N, nwg)
        p.update(kind="ATT_W64", **g)
        T, rounds = B * g["nqb"] * nst, _cdiv(B * g["nqb"] * g["nsplit"], nwg)
        if k["w64_sk"] and T >= 4 * nwg and _cdiv(T, nwg) + 2 < rounds * g["sps"]:
            p["nsplit"] = max(g["nsplit"], _sk_nsplit(B, g["nqb"], nst, nwg))
            if not ragged:
                p.update(kind="ATT_W64_SK", sk=True)
    else:
        tg = _h3_grid(1, B, N, min(k["target"], k["tiny_slots"]))
        if blocks <= k["tiny"] and tg["sps"] <= 24:
            wave_split = k["ws"] > 1 and tg["sps"] >= 4
            p.update(kind="ATT_H3_WS" if wave_split else "ATT_H3", nw=1, ws=k["ws"] if wave_split else 1, **tg)
        else:
            p["nw"] = k["nw"] if blocks <= 16 else ATT_NW
            p.update(kind="ATT_H3", **_h3_grid(p["nw"], B, N, k["target"]))
        p["early"] = p["kind"] == "ATT_H3" and p["sps"] >= 3
    p["precombine"] = k["precombine"] and not f32 and not fused and p["nsplit"] >= 16 and blocks <= 16
    p["dense_m"] = not (w64 or not (f32 or dense_m_caller or k["dense_m"]))
    p["vfold"] = k["vfold"] and allow_fused and not f32 and \
        (fused or (p["pw2"] and not p["precombine"] and
                   (p["kind"] in ("ATT_W64", "ATT_W64_SK") or (p["kind"] == "ATT_H3" and p["nw"] == ATT_NW))))
    if fused:
        p.update(kind="ATT_FUSED", nw=PW2_W, ws=1, early=False, nqb=fg["nqb"], sps=nst)
    p.update(pw_tile=0, pw_mid8=False, pw_first_qkv3=False, pw_mid_qkv3=False, pw_prefetch=False)
    if not p["pw2"]:
        small = B * (Npad // 64) < k["pw_small_limit"]
        p["pw_tile"] = 32 if small else 64
        p["pw_mid8"] = not f32 and k["pw_waves8"] and B * (Npad // 32) <= 256
        qkv3 = k["pw_qkv_split"] and 3 * B * (Npad // 32) <= 256
        p["pw_first_qkv3"] = not f32 and small and qkv3
        p["pw_mid_qkv3"] = p["pw_mid8"] and qkv3
        p["pw_prefetch"] = p["pw_mid8"] and k["pw_prefetch"]
    return p


QUERY_FIELDS = ("kind", "vfold", "Npad", "nsplit", "pw2", "pw_tile", "pw_mid8", "pw_first_qkv3", "pw_mid_qkv3",
                "pw_prefetch")


def form_as_queries(p):
    """What the host-only queries show of a (forward's) plan_form: QUERY_FIELDS as ints."""
    kind = {"ATT_FUSED": 1, "ATT_W64": 2, "ATT_W64_SK": 2}.get(p["kind"], 0)
    return [kind] + [int(p[f]) for f in QUERY_FIELDS[1:]]


def plan_shapes():
    return [(shape_key(B, N), B, N) for B, N in SHAPES] + [(RAGGED_KEY, *RAGGED_SHAPE)]


def plan_queries(precision):
    """QUERY_FIELDS of every shape from the loaded library under this process's knobs
    (pdsc_encoder_plan, pdsc_encoder_plan_vfold, pdsc_attention_layout, pdsc_launch_plan:
    host-only, the forwards' plan)."""
    import ctypes
    import torch  # noqa: F401  (before libpdsc.so: the process's HIP runtime is torch's)
    from pointdsc_amd import _lib
    L = _lib.load()
    pc, v, w = _lib.precision_code(precision), ctypes.c_int32(), ctypes.c_int32()
    cfg = _lib.make_config(num_layers=LAYERS, precision=precision)
    out = {}
    for key, B, N in plan_shapes():
        _lib.check(L.pdsc_encoder_plan(B, N, pc, ctypes.byref(v)), "encoder_plan")
        row = [v.value]
        _lib.check(L.pdsc_encoder_plan_vfold(B, N, pc, ctypes.byref(v)), "encoder_plan_vfold")
        row.append(v.value)
        _lib.check(L.pdsc_attention_layout(B, N, pc, ctypes.byref(v), ctypes.byref(w)), "attention_layout")
        row += [v.value, w.value]
        lp = (ctypes.c_int32 * 13)()
        _lib.check(L.pdsc_launch_plan(cfg, B, N, lp, 13), "launch_plan")
        out[key] = row + list(lp[:6])
    return out


def _clean_env(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDSC_") or k == "PDSC_LIB_VARIANT"}
    env.update(knobs)
    return env


def plan_queries_of(sid):
    """plan_queries under the set's knobs, in a fresh process (no GPU work)."""
    precision, knobs = KNOB_SETS[sid]
    code = f"import sys, json; sys.path[:0] = [{HERE!r}, {ROOT!r}]; import encoder_edge_cases as c; " \
           f"print('PLAN', json.dumps(c.plan_queries({precision!r})))"
    r = subprocess.run([sys.executable, "-c", code], env=_clean_env(knobs), check=True, timeout=120,
                       capture_output=True, text=True)
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("PLAN "))[5:])


def recorded_plans():
    with open(PLANS_JSON) as f:
        return json.load(f)


# ------------------------------------------------------------------ the GPU work of one knob set
def _nan_tailed(t, pad=4096):
    """`t` as the leading part of a larger device allocation whose remainder holds NaN."""
    import torch
    buf = torch.full((t.numel() + pad,), float("nan"), dtype=t.dtype, device=t.device)
    buf[:t.numel()] = t.reshape(-1)
    return buf[:t.numel()].view(t.shape)


def model(dev, precision, k=40):
    import torch
    from pointdsc_amd.PointDSC import PointDSC
    m = PointDSC(in_dim=IN_DIM, num_layers=LAYERS, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=0.10, sigma_d=0.10, k=k, nms_radius=0.10, precision=precision)
    m.load_state_dict({n: torch.from_numpy(v) for n, v in state_dict().items()})
    return m.to(dev).eval()


def _same(a, b):
    import torch
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _finite(*ts):
    import torch
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


def compute_encoder(dev, precision):
    """Every encoder-edge output of one knob set (this process's knobs): per shape
    the standalone encoder, the training forward and the stage forward, each twice
    (det_*: the two calls' bits agree) on NaN-tailed inputs (fin_*: every output
    finite); of the batch, pairs 0 and B - 1 are kept."""
    import torch
    from pointdsc_amd import kernels as K
    m = model(dev, precision)
    cfg, packed = m.pdsc_config(), _nan_tailed(m.packed_weights())
    sig = torch.tensor([0.10], device=dev)
    out = {}
    for B, N in SHAPES:
        key, pairs, b = shape_key(B, N), case_pairs(B), batch(B, N)
        corr, src, tgt = (_nan_tailed(torch.from_numpy(b[n]).to(dev)) for n in ("corr_pos", "src_keypts", "tgt_keypts"))
        M = _nan_tailed(K.compat(src, tgt, sig))
        enc = [K.encoder(cfg, packed, corr, M) for _ in range(2)]
        trn = [K.forward_training(cfg, packed, corr, src, tgt)[:3] for _ in range(2)]
        stg = [K.forward_stages(cfg, packed, corr, src, tgt) for _ in range(2)]
        names = sorted(stg[0])
        out[key + ":det"] = np.array([_same(*enc), _same(*trn), _same(*[[s[n] for n in names] for s in stg])])
        out[key + ":fin"] = np.array([_finite(*enc[0]), _finite(*trn[0]), _finite(*[stg[0][n] for n in names])])
        out[key + ":stg_eq_trn"] = np.array(torch.equal(stg[0]["conf"], trn[0][1]))
        for n, t in (("feat", enc[0][0]), ("normed", enc[0][1]), ("conf", enc[0][2]), ("trn_conf", trn[0][1]),
                     ("trn_M", trn[0][2]), ("stg_conf", stg[0]["conf"])):
            out[f"{key}:{n}"] = t[pairs].cpu().numpy()
    # the ragged batch: rows past a pair's count hold NaN in corr_pos, src and tgt
    mr = model(dev, precision, k=RAGGED_K)
    ps = ragged_pairs()
    stacks = []
    for n in ("corr_pos", "src_keypts", "tgt_keypts"):
        t, counts = K.pad_pairs([torch.from_numpy(p[n]).to(dev) for p in ps])
        for i, c in enumerate(counts):
            t[i, c:] = float("nan")
        stacks.append(_nan_tailed(t))
    rag = [K.forward_ragged(mr.pdsc_config(), packed, *stacks, counts, debug=True) for _ in range(2)]
    own = lambda r: [r[0], r[1]] + [r[2]["conf"][i, :c] for i, c in enumerate(counts)]  # noqa: E731
    out[RAGGED_KEY + ":det"] = np.array(_same(own(rag[0]), own(rag[1])))
    out[RAGGED_KEY + ":fin"] = np.array(_finite(*own(rag[0])))
    out[RAGGED_KEY + ":conf"] = rag[0][2]["conf"].cpu().numpy()
    out[RAGGED_KEY + ":labels"] = rag[0][1].cpu().numpy()
    out[RAGGED_KEY + ":trans"] = rag[0][0].cpu().numpy()
    return out


def attention_inputs(B, N, dev, sq=1.0, sk=1.0, seed=9):
    """q, k, v ~ N(0, 1) (q, k scaled) and M from kernels.compat on a synthetic pair, NaN-tailed."""
    import torch
    from pointdsc_amd import kernels as K
    g = torch.Generator().manual_seed(seed + 1000 * B + N)
    q, k, v = (torch.randn(B, N, 128, generator=g) for _ in range(3))
    b = batch(B, max(N, 2))
    src, tgt = (torch.from_numpy(b[n][:, :N].copy()).to(dev) for n in ("src_keypts", "tgt_keypts"))
    M = K.compat(src, tgt, torch.tensor([0.10], device=dev))
    return [_nan_tailed(t) for t in ((q * sq).to(dev), (k * sk).to(dev), v.to(dev), M)]


def attention_cases(dev):
    """(key, q, k, v, M) of every standalone-attention case: the edge shapes, dead rows
    and columns of M, M == 0, and one adversarial-magnitude case."""
    for B, N in ATT_SHAPES:
        yield (f"att:{shape_key(B, N)}", *attention_inputs(B, N, dev))
    for N in DEAD_NS:
        q, k, v, M = attention_inputs(2, N, dev)
        dead = [0, N // 2, N - 1]
        M[:, dead, :] = 0.0
        M[:, :, dead] = 0.0
        yield (f"dead:{N}", q, k, v, M)
    for N in ZERO_NS:
        q, k, v, M = attention_inputs(2, N, dev)
        M.zero_()
        yield (f"zero:{N}", q, k, v, M)
    B, N, sq, sk = ADVERSARIAL
    q, k, v, M = attention_inputs(B, N, dev, sq, sk)
    v[:, ::7] *= 1e-3  # rows of very different magnitude inside one 32-key tile
    yield ("adv", q, k, v, M)


def compute_attention(dev, precisions):
    """kernels.attention on every attention case (this process's knobs), twice; in f32
    also kernels.attention_lse's msg."""
    import torch
    from pointdsc_amd import kernels as K
    out = {}
    for key, q, k, v, M in attention_cases(dev):
        for pr in precisions:
            a, b = (K.attention(q, k, v, M, precision=pr) for _ in range(2))
            out[f"{key}:{pr}"] = a.cpu().numpy()
            out[f"{key}:{pr}:det"] = np.array(torch.equal(a, b))
            if pr == "f32":
                out[f"{key}:lse_eq"] = np.array(torch.equal(a, K.attention_lse(q, k, v, M)[0]))
    return out


def compute(sid, dev):
    precision, _ = KNOB_SETS[sid]
    out = compute_encoder(dev, precision)
    out["plans"] = np.array(json.dumps(plan_queries(precision)))  # what THIS process's library plans
    if sid in ATT_SETS:  # (the exact-fp32 attention's plan follows none of the children's knobs)
        out.update(compute_attention(dev, ("h3", "f32") if sid == "default" else ("h3",)))
    return out


def _dump(sid, path):  # child process entry (knobs set by the parent process)
    import torch
    t0 = time.time()
    out = compute(sid, torch.device("cuda:0"))
    torch.cuda.synchronize()
    np.savez(path, seconds=np.float64(time.time() - t0), **out)


class KnobSetFailed(Exception):
    pass


_RESULTS = {}   # sid -> dict of arrays, or a KnobSetFailed
_FAULT = []     # [(sid, why)]: a child ended by a signal, its time limit or a HIP fault
_TMP = []
FAULT_WORDS = ("illegal memory access", "hipErrorIllegalAddress", "HSA_STATUS_ERROR", "Memory access fault",
               "hipErrorLaunchFailure", "core dumped")


def child_result(sid, dev):
    """The outputs of knob set `sid`: computed once per session (in this process for
    IN_PROCESS, else in one fresh child under CHILD_TIMEOUT), then read from memory.
    After a child ended by a signal, by its time limit or with a HIP fault in its
    output, no further GPU process starts in the session: every set not yet computed
    raises KnobSetFailed."""
    if sid not in _RESULTS:
        _RESULTS[sid] = _run_set(sid, dev)
    if isinstance(_RESULTS[sid], Exception):
        raise _RESULTS[sid]
    return _RESULTS[sid]


def _run_set(sid, dev):
    if _FAULT:
        return KnobSetFailed(f"{sid}: not started: knob set {_FAULT[0][0]} ended with {_FAULT[0][1]}")
    precision, knobs = KNOB_SETS[sid]
    if sid in IN_PROCESS:
        assert not [k for k in os.environ if k.startswith("PDSC_") and k != "PDSC_LIB_VARIANT"], "knobs in the test process"
        return compute(sid, dev)
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="encoder_edges_"))
    path = os.path.join(_TMP[0], sid + ".npz")
    code = f"import sys; sys.path[:0] = [{HERE!r}, {ROOT!r}]; import encoder_edge_cases as c; c._dump({sid!r}, {path!r})"
    try:
        r = subprocess.run([sys.executable, "-c", code], env=_clean_env(knobs), timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _FAULT.append((sid, f"its time limit of {CHILD_TIMEOUT:.0f} s"))
        return KnobSetFailed(f"{sid}: the child ran into its time limit of {CHILD_TIMEOUT:.0f} s")
    text = (r.stdout or "") + (r.stderr or "")
    word = next((w for w in FAULT_WORDS if w in text), None)
    if r.returncode < 0 or word:
        why = f"signal {-r.returncode}" if r.returncode < 0 else f"a HIP fault ({word})"
        _FAULT.append((sid, why))
        return KnobSetFailed(f"{sid}: the child ended with {why}:\n{text[-2000:]}")
    if r.returncode != 0:
        return KnobSetFailed(f"{sid}: the child failed (exit {r.returncode}):\n{text[-2000:]}")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    sys.path[:0] = [HERE, ROOT]
    if sys.argv[1:2] == ["--write-plans"]:
        table = {sid: plan_queries_of(sid) for sid in KNOB_SETS}
        os.makedirs(os.path.dirname(PLANS_JSON), exist_ok=True)
        with open(PLANS_JSON, "w") as f:
            f.write("{\n" + ",\n".join(
                f' "{sid}": {{\n' + ",\n".join(f'  "{k}": {json.dumps(v)}' for k, v in rows.items()) + "\n }"
                for sid, rows in table.items()) + "\n}\n")
        print("wrote", PLANS_JSON)
    else:
        sys.exit("usage: encoder_edge_cases.py --write-plans")
