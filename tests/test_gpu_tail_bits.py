"""The a-row stage entries and the forwards, bit for bit against a recording
(tests/golden/tail_bits/tail_bits.json).

The other GPU files hold these stages to exact or fp64 references within
tolerances (test_gpu_front_stages.py, test_gpu_nsm_stages.py, the parity
files).  This one holds them to themselves, as test_gpu_solver_bits.py does for
the solvers: every output byte of a fixed set of calls must equal what an
earlier build of the same sources produced.  That is the property a refactor of
the tail relies on ("two builds, same bits"): moving a kernel, a launcher or an
entry point between files changes no arithmetic, no launch shape and no plan,
so no bit may move.

The recording holds a SHA-256 per output tensor.  It is tied to the toolchain:
a different compiler may contract, reassociate or schedule differently.  Only a
commit that MEANS to change the tail's numerics, or a ROCm update, re-records
it: `python tests/test_gpu_tail_bits.py --write` on the GPU (PDSC_LIB_VARIANT
selects the build to record from).  Write it twice and compare the two files
before committing: an output that differs run to run does not belong here.

The cases are the edge shapes the stage tests already generate
(front_reference.py, nsm_reference.py): the dense and packed compatibility at
the tile edges; the seed ranking's big-batch plans; the seed kNN's register,
unaligned-row and radix paths in both precisions; every NSM KC variant and exit
rule; the hypotheses' four launch plans; the refinement's five pairs per launch;
the weighted Kabsch at n = 0, 1, 3, 257; the testing forward with and without
its debug outputs (without: select_best and post_refine in one launch) on the
smallest golden and as a ragged batch of two goldens of different sizes; the
training forward on train_small.  Outputs a ragged call leaves unwritten (rows
past a pair's own count) are not hashed.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import front_reference as F  # noqa: E402
import nsm_reference as R  # noqa: E402
from conftest import golden_hparams, golden_state_dict, load_golden  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "tail_bits", "tail_bits.json")
PRECISIONS = ("h3", "f32")

COMPAT_NS = (1, 31, 32, 33, 65)
RIGID_CASES = [(n, w) for n in (0, 1, 3, 257) for w in (0, 1)]
FORWARD_CASES = [(kind, p) for kind in ("single", "ragged") for p in PRECISIONS]


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def _entry(outputs):
    return {k: _sha(v) for k, v in outputs.items()}


def _t(a, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t if dtype is None else t.to(dtype)


def _scalar(x, dev):
    import torch
    return torch.tensor([x], dtype=torch.float32, device=dev)


def run_compat(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    (N,) = case
    src, tgt = (_t(a, dev) for a in F.compat_pairs(N))
    sd = _scalar(F.COMPAT_SIGMA, dev)
    M = K.compat(src, tgt, sd)
    # the packed tiles themselves (K.compat_packed unpacks them); zeroed first: the hash covers the padding
    Mp = torch.zeros((2, K.query("pdsc_compat_packed_floats", N)), dtype=torch.float32, device=dev)
    K.call("pdsc_compat_packed_f32", src, tgt, 2, N, sd, Mp, device=dev)
    return _entry(dict(M=M, Mp=Mp))


def run_seeds(dev, case):
    from pointdsc_amd import kernels as K
    (cid,) = case
    c = next(x for x in F.SEED_PLAN_CASES if x["id"] == cid)
    src, conf = (_t(a, dev) for a in F.seed_plan_case(c["B"], c["N"], c["S"]))
    seeds, _ = K.pick_seeds(src, conf, F.SEED_RADIUS, c["S"])  # (is_local_max is the entry's scratch)
    return _entry(dict(seeds=seeds))


def run_knn(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    cid, precision = case
    c = next(x for x in F.KNN_CASES if x["id"] == cid)
    d = F.knn_case(c)
    knn = K.seed_knn(_t(d["normed"], dev), _t(d["seeds"], dev, torch.int32), c["k"], precision)
    return _entry(dict(knn=knn))


def _by_id(cases, cid):
    return next(c for c in cases if c["id"] == cid)


def run_nsm(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    cid, precision = case
    d = R.nsm_case(_by_id(R.NSM_CASES, cid))
    w, it = K.nsm_weights(_t(d["normed"], dev), _t(d["src"], dev), _t(d["tgt"], dev), _t(d["knn"], dev, torch.int32),
                          d["T"], _scalar(d["sigma"], dev), _scalar(d["sigma_d"], dev), precision)
    return _entry(dict(weights=w, iters=it))


def run_hyp(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    cid, tau = case
    d = R.hyp_case(_by_id(R.HYP_CASES, cid))
    names = ("seed_trans", "fitness", "best", "trans", "labels")
    out = K.seed_hypotheses(_t(d["src"], dev), _t(d["tgt"], dev), _t(d["knn"], dev, torch.int32), _t(d["w"], dev), tau)
    return _entry(dict(zip(names, out)))


def run_refine(dev, case):
    from pointdsc_amd import kernels as K
    (cid,) = case
    d = R.refine_case(_by_id(R.REFINE_CASES, cid))
    return _entry(dict(trans=K.post_refine(_t(d["trans0"], dev), _t(d["src"], dev), _t(d["tgt"], dev), d["thr"])))


def run_rigid(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    n, weighted = case
    rng = np.random.default_rng(5000 + n)
    pairs = [R.make_pair(rng, max(n, 1))[:2] for _ in range(2)]
    # (n = 0: one-row buffers, so that the pointers are not NULL; no row is read)
    A, B = (_t(np.stack([p[i] for p in pairs]), dev) for i in (0, 1))
    w = _t((rng.random((2, max(n, 1))) - 0.2).astype(np.float32), dev) if weighted else None  # some below 0: clamped
    out = torch.empty((2, 4, 4), dtype=torch.float32, device=dev)
    K.call("pdsc_rigid_transform_3d", A, B, w, 2, n, out, device=dev)
    return _entry(dict(trans=out))


def _model(g, dev, precision):
    import torch
    from pointdsc_amd.PointDSC import PointDSC
    hp = golden_hparams(g)
    m = PointDSC(in_dim=6, num_layers=hp["num_layers"], num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=hp["inlier_threshold"], sigma_d=float(g["sigma_d"]), k=40,
                 nms_radius=hp["nms_radius"], precision=precision)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state_dict(g).items()})
    return m.to(dev).eval()


def run_forward(dev, case):
    from pointdsc_amd import kernels as K
    kind, precision = case
    names = ("corr_pos", "src_keypts", "tgt_keypts")
    if kind == "single":  # the smallest golden: N = 30, k = 29, S = 3
        g = load_golden("tiny_k")
        m = _model(g, dev, precision)
        corr, src, tgt = (_t(g[k], dev)[None] for k in names)
        out = dict(K.forward_stages(m.pdsc_config(), m.packed_weights(), corr, src, tgt))
        T, L, conf, seeds = K.forward_testing(m.pdsc_config(), m.packed_weights(), corr, src, tgt, debug=True)
        out.update(plain_trans=T, plain_labels=L, plain_conf=conf, plain_seeds=seeds)
        return _entry(out)
    # two goldens of different sizes (256 and 64 rows; both keep k = 40) under the first one's weights
    gs = [load_golden("small_3dm"), load_golden("tiny_out")]
    m = _model(gs[0], dev, precision)
    corr, src, tgt = (K.pad_pairs([_t(g[k], dev) for g in gs])[0] for k in names)
    counts = [len(g["corr_pos"]) for g in gs]
    T, L, st = K.forward_ragged(m.pdsc_config(), m.packed_weights(), corr, src, tgt, counts, debug=True)
    out = dict(final_trans=T, final_labels=L, trans_pre_refine=st["trans_pre_refine"])
    for b, n in enumerate(counts):  # a pair's own rows: the rest of the batch's stride is never written
        S = int(n * 0.1)
        out.update({f"conf{b}": st["conf"][b, :n], f"seeds{b}": st["seeds"][b, :S], f"knn{b}": st["knn"][b, :S],
                    f"weights{b}": st["weights"][b, :S]})
    T, L = K.forward_ragged(m.pdsc_config(), m.packed_weights(), corr, src, tgt, counts)
    out.update(plain_trans=T, plain_labels=L)
    return _entry(out)


def run_training(dev, case):
    from pointdsc_amd import kernels as K
    (precision,) = case
    g = load_golden("train_small")  # B = 2, N = 256
    m = _model(g, dev, precision)
    corr, src, tgt = (_t(g[k], dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    T, conf, M, seeds = K.forward_training(m.pdsc_config(), m.packed_weights(), corr, src, tgt, want_M=True,
                                           want_seeds=True)
    return _entry(dict(final_trans=T, confidence=conf, seeds=seeds, M=M))


GROUPS = {
    "compat": ([(N,) for N in COMPAT_NS], run_compat),
    "seeds": ([(c["id"],) for c in F.SEED_PLAN_CASES], run_seeds),
    "knn": ([(c["id"], p) for c in F.KNN_CASES for p in PRECISIONS], run_knn),
    "nsm": ([(c["id"], p) for c in R.NSM_CASES for p in PRECISIONS], run_nsm),
    "hyp": ([(c["id"], tau) for c in R.HYP_CASES for tau in R.HYP_TAUS], run_hyp),
    "refine": ([(c["id"],) for c in R.REFINE_CASES], run_refine),
    "rigid": (RIGID_CASES, run_rigid),
    "forward": (FORWARD_CASES, run_forward),
    "training": ([(p,) for p in PRECISIONS], run_training),
}


def _key(group, case):
    return group + ":" + ",".join(str(v) for v in case)


ALL = [(g, c) for g, (cases, _) in GROUPS.items() for c in cases]


@pytest.fixture(scope="module")
def recording():
    with open(FIXTURE) as f:
        return json.load(f)


def test_recording_lists_these_cases(recording):
    assert sorted(recording) == sorted(_key(g, c) for g, c in ALL)


@pytest.mark.gpu
@pytest.mark.parametrize("group,case", ALL, ids=[_key(g, c) for g, c in ALL])
def test_tail_bits(gpu_device, recording, group, case):
    got, want = GROUPS[group][1](gpu_device, case), recording[_key(group, case)]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    print(_key(group, case), "differing outputs:", bad or "none")
    assert not bad, f"{_key(group, case)}: {bad} differ from the recording"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        import torch
        dev = torch.device("cuda:0")
        table = {_key(g, c): GROUPS[g][1](dev, c) for g, c in ALL}
        path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path, len(table), "cases")
    else:
        sys.exit("usage: test_gpu_tail_bits.py --write [PATH]")
