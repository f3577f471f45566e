"""The filtered-RANSAC front end (include/pdsc.h f7, pointdsc_amd/matching.py,
pointdsc_amd/fr.py) on the GPU against the goldens recorded from the reference
(tests/golden/fr) and the fp64 restatement tests/fr_reference.py.

Indices, sets, cells, per_quad and kept sets are compared exactly, on cases whose
decisions are free of near-ties by the margins derived in fr_reference.py (the
condition is asserted on the CPU reference; it selects seeds and widens
nothing).  feat_dist against the reference's fp32 values: both sides are fp32
evaluations of two length-D sums, each within RATIO_REL(D) = 1.01 (D + 6) u of
the exact ratio, so they differ by at most 2 RATIO_REL(D) relative; norm by at
most twice its bound 4 e / (max - min) + 3 u.  The GPF cases pass norm in as
data, so every decision there is an exact comparison of the same fp32 values:
no margin is needed.  Refit poses: 1e-9 absolute against numpy's fp64 Kabsch."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import fr_reference as F
import ransac_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _golden(name):
    with np.load(os.path.join(GOLDEN, "fr", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


# ----------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("name", sorted(F.GOLDEN_CASES))
def test_goldens(name, gpu_device):
    from pointdsc_amd import matching as M
    g = _golden(name)
    D, G, factor = g["f0"].shape[1], int(g["grid"]), float(g["factor"])
    assert g["margins"].min() > 1.0
    f0, f1, xyz0 = _t(g["f0"], gpu_device), _t(g["f1"], gpu_device), _t(g["xyz0"], gpu_device)
    nn1, nn2, rev = M.nn2(f0, f1)
    assert np.array_equal(_np(nn1), g["nn1"]) and np.array_equal(_np(nn2), g["nn2"])
    fd, is_bb, norm, num_bb = M.match_ratio(f0, f1, nn1, nn2, rev)
    assert np.array_equal(_np(is_bb) != 0, g["is_bb"]) and int(num_bb.item()) == int(g["num_bb"])
    rel = np.abs(_np(fd).astype(np.float64) - g["feat_dist"]) / g["feat_dist"]
    ref = F.match_ratio(g["f0"], g["f1"], g["nn1"], g["nn2"], _np(rev))
    err = np.abs(_np(norm).astype(np.float64) - g["norm_feat_dist"]).max()
    print("feat_dist relative:", rel.max(), "bound", 2 * F.ratio_rel(D), " norm:", err, "bound", 2 * ref["norm_bound"])
    assert rel.max() <= 2 * F.ratio_rel(D) and err <= 2 * ref["norm_bound"]
    kept, kept_norm, dbg = M.gpf_select(xyz0, norm, num_bb, G, factor, debug=True)
    assert np.array_equal(_np(dbg["cell"]), g["quadrant_i"] * G + g["quadrant_j"])
    assert np.array_equal(_np(dbg["max_per_quad"]).reshape(G, G), g["max_per_quad"])
    assert np.array_equal(_np(dbg["per_quad"]).reshape(G, G), g["per_quad"])
    assert float(dbg["height"].item()) == float(g["height"])
    assert np.array_equal(_np(kept), g["kept"])
    assert np.array_equal(_np(kept_norm).view(np.int32), _np(norm)[g["kept"]].view(np.int32))
    # the reference's names
    i0, i1, i2 = M.find_nn(f0, f1, return_2nd=True)
    assert i1.dtype == torch.int64 and np.array_equal(_np(i0), np.arange(len(g["f0"]))) and M.find_nn(f0, f1)[2] is None
    m0, m1, m2 = M.nn_to_mutual(f0, f1, i0, i1, i2)
    assert np.array_equal(_np(m0), g["mutual_idx0"]) and np.array_equal(_np(m1), g["mutual_idx1"])
    assert np.array_equal(_np(m2), g["nn2"][g["mutual_idx0"]])
    assert M.nn_to_mutual(f0, f1, i0, i1, None, force_return_2nd=True)[2] is None and len(M.nn_to_mutual(f0, f1, i0, i1)) == 2
    bb, n = M.mark_best_buddies(f0, f1, i0, i1)
    assert np.array_equal(_np(bb), g["is_bb"]) and n == int(g["num_bb"])
    assert torch.equal(M.calc_distance_ratio_in_feature_space(f0, f1, i0, i1, i2), fd)
    out = M.Grid_Prioritized_Filter(f0, f1, i0, i1, i2, xyz0, types.SimpleNamespace(GPF_grid_wid=G, GPF_factor=factor))
    assert len(out) == 7 and np.array_equal(_np(out[0]), g["kept"]) and np.array_equal(_np(out[1]), g["nn1"][g["kept"]])
    assert np.array_equal(_np(out[2]), g["nn2"][g["kept"]]) and out[3] is i0 and out[4] is i1 and out[5] is i2
    assert torch.equal(out[6], kept_norm)
    t = M.find_2nn(f0, f1)
    assert torch.equal(t[1], i1) and torch.equal(t[2], i2) and isinstance(t[3], float)


# ------------------------------------------------------------- 2. nn2 shapes
def _nn2_seed(N0, N1, D):
    for seed in range(100):
        f0, f1, _ = F.desc_case(10000 * D + seed, N0, N1, D)
        ref = F.nn2(f0, f1)
        if ref["margin"] > 1.0:
            return f0, f1, ref
    raise RuntimeError("no tie-free seed")


@pytest.mark.parametrize("D", [1, 5, 32, 33, 64])
@pytest.mark.parametrize("N1", [2, 63, 65, 130])
@pytest.mark.parametrize("N0", [1, 63, 64, 65, 257])
def test_nn2_shapes(N0, N1, D, gpu_device):
    from pointdsc_amd import matching as M
    f0, f1, ref = _nn2_seed(N0, N1, D)
    assert ref["margin"] > 1.0
    nn1, nn2, rev = M.nn2(_t(f0, gpu_device), _t(f1, gpu_device))
    assert np.array_equal(_np(nn1), ref["nn1"]) and np.array_equal(_np(nn2), ref["nn2"])
    assert np.array_equal(_np(rev), ref["rev"])
    if N1 == 2:
        assert np.array_equal(_np(nn2), 1 - ref["nn1"])


def test_nn2_duplicates(gpu_device):
    from pointdsc_amd import matching as M
    f0, f1, _ = F.desc_case(5, 130, 200, 32)
    f1[150], f1[199] = f1[3], f1[70]      # duplicate target rows, across column tiles
    f0[0], f0[129] = f1[3], f1[70]        # sources at distance 0 from both copies
    f0[100], f0[64] = f0[7], f0[7]        # duplicate source rows, across row stripes
    ref = F.nn2(f0, f1)
    assert ref["margin"] > 1.0  # duplicates are exempt; nothing else is close
    nn1, nn2, rev = (_np(x) for x in M.nn2(_t(f0, gpu_device), _t(f1, gpu_device)))
    assert (nn1[0], nn2[0]) == (3, 150) and (nn1[129], nn2[129]) == (70, 199)
    assert nn1[64] == nn1[100] == nn1[7] and rev[nn1[7]] not in (64, 100)
    assert np.array_equal(nn1, ref["nn1"]) and np.array_equal(nn2, ref["nn2"]) and np.array_equal(rev, ref["rev"])


def test_nn2_split_is_exact(gpu_device):
    """18 column tiles: the result with one workgroup per row stripe, with the
    default split, with an uneven one and with the largest is the same, bit for
    bit, and is the reference's."""
    from pointdsc_amd import matching as M
    for seed in range(100):
        f0, f1, _ = F.desc_case(seed, 130, 1100, 32)
        ref = F.nn2(f0, f1)
        if ref["margin"] > 1.0:
            break
    assert ref["margin"] > 1.0
    a, b = _t(f0, gpu_device), _t(f1, gpu_device)
    base = [_np(x) for x in M.nn2(a, b)]
    for split in (1, 5, 16, 1000):  # above 16: clamped
        got = [_np(x) for x in M.nn2(a, b, split=split)]
        assert all(np.array_equal(x, y) for x, y in zip(base, got)), split
    assert np.array_equal(base[0], ref["nn1"]) and np.array_equal(base[1], ref["nn2"]) and np.array_equal(base[2], ref["rev"])
    with pytest.raises(RuntimeError, match="split"):
        M.nn2(a, b, split=0)


def test_find_nn_single_target_and_full_range(gpu_device):
    """The reference's find_nn accepts one target row; GPF insists on the full range it assumes."""
    from pointdsc_amd import matching as M
    f0, f1, xyz0 = (_t(x, gpu_device) for x in F.desc_case(1, 10, 4, 8))
    i0, i1, i2 = M.find_nn(f0, f1[:1])
    assert np.array_equal(_np(i0), np.arange(10)) and not _np(i1).any() and i1.dtype == torch.int64 and i2 is None
    with pytest.raises(RuntimeError, match="N1=1"):
        M.find_nn(f0, f1[:1], return_2nd=True)
    i0, i1, i2 = M.find_nn(f0, f1, return_2nd=True)
    args = types.SimpleNamespace(GPF_grid_wid=2, GPF_factor=1.0)
    with pytest.raises(ValueError, match="full range"):
        M.Grid_Prioritized_Filter(f0, f1, i0.flip(0), i1, i2, xyz0, args)
    with pytest.raises(ValueError, match="full range"):
        M.Grid_Prioritized_Filter(f0, f1, i0[:5], i1, i2, xyz0, args)


# ------------------------------------------------------------- 3. GPF shapes
def _gpf_check(dev, xyz0, norm, num_bb, G, factor):
    from pointdsc_amd import matching as M
    ref = F.gpf_select(xyz0, norm, num_bb, G, factor)
    kept, kn, dbg = M.gpf_select(_t(xyz0, dev), _t(norm, dev), torch.tensor([num_bb], dtype=torch.int32, device=dev), G,
                                 factor, debug=True)
    assert np.array_equal(_np(dbg["cell"]), ref["cell"])
    assert np.array_equal(_np(dbg["max_per_quad"]).reshape(G, G), ref["max_per_quad"])
    assert np.array_equal(_np(dbg["per_quad"]).reshape(G, G), ref["per_quad"])
    assert float(dbg["height"].item()) == ref["height"]
    assert np.array_equal(_np(kept), ref["kept"])
    assert np.array_equal(_np(kn), np.asarray(norm, np.float32)[ref["kept"]])
    return ref


@pytest.mark.parametrize("G", [1, 3, 10, 64])
@pytest.mark.parametrize("N0", [1, 257, 1500])
def test_gpf_shapes(N0, G, gpu_device):
    rng = np.random.RandomState(N0 + G)
    xyz0 = (rng.rand(N0, 3) * 50).astype(np.float32)
    norm = (rng.rand(N0) * 2 - 1).astype(np.float32)
    nb = max(1, N0 // 3)
    for factor in (0.0, 0.5, 1.0, 1.5, 100.0):
        ref = _gpf_check(gpu_device, xyz0, norm, nb, G, factor)
        if factor == 0.0:
            assert len(ref["kept"]) == 0
        if factor == 100.0:
            assert len(ref["kept"]) == N0
    if G == 64:
        assert (ref["max_per_quad"] == 0).any()  # empty cells


def test_gpf_branches(gpu_device):
    rng = np.random.RandomState(2)
    N0 = 400
    xyz0 = (rng.rand(N0, 3) * 50).astype(np.float32)
    xyz0[:300, :2] = rng.rand(300, 2) * 12  # a crowded corner: tall cells beside sparse ones
    norm = (np.round(rng.rand(N0) * 4) / 4 - (rng.rand(N0) < 0.3)).astype(np.float32)  # few distinct values: ties
    ref = _gpf_check(gpu_device, xyz0, norm, 120, 4, 1.0)
    pq, mpq = ref["per_quad"], ref["max_per_quad"]
    assert ((pq == mpq) & (mpq > 0)).any() and ((pq > 0) & (pq < mpq)).any()  # keep-all beside truncated
    cut = [c for c in range(16) if 0 < pq.reshape(-1)[c] < mpq.reshape(-1)[c]]
    tied = False
    for c in cut:  # an equal norm on both sides of a cut: the lower row was kept
        rows = np.flatnonzero(ref["cell"] == c)
        k = np.isin(rows, ref["kept"])
        tied |= bool(np.intersect1d(norm[rows[k]], norm[rows[~k]]).size)
    assert tied
    # every x equal: M - m = 0, the x quadrant is 0 for every row
    flat = xyz0.copy()
    flat[:, 0] = 7.25
    r = _gpf_check(gpu_device, flat, norm, 120, 3, 1.0)
    assert (r["cell"] < 3).all()
    # a height that rounds to 0: nothing is kept although TOTAL > 0
    r = _gpf_check(gpu_device, xyz0, norm, 1, 10, 0.4)
    assert r["height"] <= 0.5 and len(r["kept"]) == 0
    # an extent that loses the 1e-3: the farthest row is in no cell
    far = xyz0.copy()
    far[0, 0] = 3e5
    r = _gpf_check(gpu_device, far, norm, 120, 3, 1.0)
    assert r["cell"][0] == -1 and 0 not in r["kept"]


def test_match_ratio_max_equals_min(gpu_device):
    from pointdsc_amd import matching as M
    f = _t(np.eye(4, dtype=np.float32), gpu_device)
    idx = torch.arange(4, device=gpu_device)
    fd, is_bb, norm, num_bb = M.match_ratio(f, f, idx, (idx + 1) % 4, idx)
    assert np.array_equal(_np(fd), np.zeros(4)) and np.array_equal(_np(norm), -np.ones(4)) and int(num_bb.item()) == 4


# ------------------------------------------------------------------ 4. refit
def test_refit_inliers(gpu_device):
    from pointdsc_amd import matching as M
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    src, tgt, true, _ = R.make_case(21, 300, 0.5)
    pose = true @ R.rigid([1, 2, 3], 0.3, [0.004, -0.003, 0.002])  # a hypothesis near the truth
    d = np.sqrt(R.distances2(pose, src, tgt))
    assert (np.abs(d - 0.1) / 0.1).min() >= 1e-7  # no inlier decision is a near-tie
    want, n, inl = F.refit_inliers(pose, src, tgt, 0.1)
    assert 100 < n < 300
    s, t = _t(src, gpu_device), _t(tgt, gpu_device)
    T, T32, cnt, labels = M.refit_inliers(torch.from_numpy(pose), s, t, 0.1)
    err = np.abs(_np(T) - want).max()
    print("max |dT| vs numpy:", err)
    assert err <= 1e-9 and int(cnt.item()) == n and np.array_equal(_np(labels) > 0, inl)
    assert np.array_equal(_np(T32), _np(T).astype(np.float32))
    # fewer than 3 inliers: the input pose, bit for bit (also its last row)
    odd = np.arange(16, dtype=np.float64).reshape(4, 4) * 1000.0 + 0.1
    T, _, cnt, labels = M.refit_inliers(torch.from_numpy(odd), s, t, 0.1)
    assert np.array_equal(_np(T).view(np.int64), odd.view(np.int64)) and int(cnt.item()) == 0 and not _np(labels).any()
    two = np.eye(4)
    T, _, cnt, _ = M.refit_inliers(torch.from_numpy(two), s[:2], s[:2], 0.1)
    assert np.array_equal(_np(T), two) and int(cnt.item()) == 2
    # on RANSAC's own point set and winner it is RANSAC's refit
    plain = ransac(s, t, None, 0.1, ransac_n=4, max_iteration=2048, seed=3)
    refit = ransac(s, t, None, 0.1, ransac_n=4, max_iteration=2048, seed=3, refit=True)
    assert plain.n_inliers >= 3
    T, T32, cnt, labels = M.refit_inliers(plain.transformation, s, t, 0.1)
    assert np.array_equal(_np(T).view(np.int64), _np(refit.transformation).view(np.int64))
    assert np.array_equal(_np(T32).view(np.int32), _np(refit.transformation_f32).view(np.int32))
    assert int(cnt.item()) == plain.n_inliers and torch.equal(labels, plain.labels)


# --------------------------------------------------------------------- 5. FR
_FR_REF = {}


def _fr_case():
    if not _FR_REF:
        seed = F.planted_seed()
        _FR_REF["in"] = F.planted_registration(seed)
    return _FR_REF["in"]


@pytest.mark.parametrize("mode", ["no_filter", "MFR", "GPF"])
def test_fr_end_to_end(mode, gpu_device):
    from pointdsc_amd import FR
    xyz0, xyz1, f0, f1, T_gt = _fr_case()
    ref = F.fr(xyz0, xyz1, f0, f1, T_gt, mode, 4096, seed=5)
    args = types.SimpleNamespace(mode=mode, algo="RANSAC", iters=4096, ELC=False, GPF_grid_wid=10, GPF_factor=1.0)
    dev_in = [_t(x, gpu_device) for x in (xyz0, xyz1, f0, f1)]
    out = FR(*dev_in, args, T_gt, seed=5)
    assert len(out) == 8 and out[2] is dev_in[0] and out[3] is dev_in[1] and out[1] > 0
    assert out[4:] == (ref["num_pairs_init"], ref["inlier_ratio_init"], ref["num_pairs_filtered"],
                       ref["inlier_ratio_filtered"])
    T = _np(out[0])
    err, rerr = np.abs(T - T_gt).max(), np.abs(ref["T"] - T_gt).max()
    print(mode, "pairs", out[6], "of", out[4], " max |T - planted|:", err, " reference's:", rerr)
    assert T.dtype == np.float64 and err <= 1e-3 and rerr <= 1e-3
    again = FR(*dev_in, args, T_gt, seed=5)
    assert np.array_equal(_np(again[0]).view(np.int64), T.view(np.int64)) and again[4:] == out[4:]


def test_fr_rejects(gpu_device):
    from pointdsc_amd import FR
    xyz0, xyz1, f0, f1, T_gt = _fr_case()
    dev_in = [_t(x[:50], gpu_device) for x in (xyz0, xyz1, f0, f1)]
    base = dict(mode="MFR", algo="RANSAC", iters=64, ELC=True, GPF_grid_wid=10, GPF_factor=1.0)
    with pytest.raises(NotImplementedError):
        FR(*dev_in, types.SimpleNamespace(**dict(base, algo="GC")), T_gt)
    with pytest.raises(AssertionError):
        FR(*dev_in, types.SimpleNamespace(**dict(base, mode="DFR")), T_gt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FR(*(torch.from_numpy(x) for x in (xyz0, xyz1, f0, f1)), types.SimpleNamespace(**base), T_gt)
    # a filter that keeps nothing: the identity
    out = FR(*dev_in, types.SimpleNamespace(**dict(base, mode="GPF", GPF_factor=0.0)), T_gt)
    assert out[6] == 0 and np.array_equal(_np(out[0]), np.eye(4))
    assert len(FR(*dev_in, types.SimpleNamespace(**base), T_gt)) == 8  # ELC on: runs


# ------------------------------------------------------------- 6. ABI errors
def test_abi_errors_launch_nothing(gpu_device):
    """Every rejected call returns its documented status and leaves the (real,
    pre-filled) output buffers untouched."""
    from pointdsc_amd import _lib
    from pointdsc_amd.kernels import _p, _stream
    L = _lib.load()
    ARG, UNSUP = 1, 3
    dev = gpu_device
    N0, N1, D = 70, 66, 64
    f0, f1 = torch.rand(N0, 65, device=dev), torch.rand(N1, 65, device=dev)
    xyz = torch.rand(N0, 3, device=dev)
    outs = {k: torch.full((max(N0, N1),), -7, dtype=torch.int32, device=dev) for k in ("a", "b", "r", "bb", "nb", "kept", "cnt")}
    fo = {k: torch.full((N0,), -7.0, device=dev) for k in ("fd", "norm", "kn")}
    pose = torch.eye(4, dtype=torch.float64, device=dev)
    tr = torch.full((4, 4), -7.0, dtype=torch.float64, device=dev)
    nb = L.pdsc_nn2_workspace_bytes(N0, N1)
    gb = L.pdsc_gpf_select_workspace_bytes(N0, 10)
    assert nb > 0 and gb > 0 and L.pdsc_nn2_workspace_bytes(N0, 1) == 0 and L.pdsc_gpf_select_workspace_bytes(N0, 65) == 0
    assert L.pdsc_gpf_select_workspace_bytes(262144, 1) > 0 and L.pdsc_gpf_select_workspace_bytes(262145, 1) == 0
    ws = torch.full((max(nb, gb),), 0x5A, dtype=torch.uint8, device=dev)
    st = _stream(dev)
    o = {k: _p(v) for k, v in {**outs, **fo}.items()}

    def nn2(f0_=_p(f0), f1_=_p(f1), n0=N0, n1=N1, d=D, a=o["a"], w=_p(ws), wb=nb):
        return L.pdsc_nn2(f0_, f1_, n0, n1, d, a, o["b"], o["r"], w, wb, st)

    def ratio(d=D, n1=N1, fd=o["fd"], rev=o["r"], bb=o["bb"]):
        return L.pdsc_match_ratio(_p(f0), _p(f1), N0, n1, d, o["a"], o["b"], rev, bb, fd, o["norm"], o["nb"], st)

    def gpf(g=10, factor=1.0, x=_p(xyz), w=_p(ws), wb=gb, n0=N0):
        return L.pdsc_gpf_select(x, o["norm"], o["nb"], n0, g, factor, o["kept"], o["cnt"], o["kn"], None, w, wb, st)

    def refit(p=_p(pose), n=N0, r=0.1, t=_p(tr)):
        return L.pdsc_refit_inliers(p, _p(xyz), _p(xyz), n, r, t, None, None, None, st)

    for call, want, word in [
        (lambda: nn2(d=0), ARG, b"D=0"), (lambda: nn2(d=65), UNSUP, b"D=65"), (lambda: nn2(n1=1), ARG, b"N1=1"),
        (lambda: nn2(n0=0), ARG, b"N0=0"), (lambda: nn2(wb=nb - 1), ARG, b"workspace"),
        (lambda: nn2(f0_=None), ARG, b"null"), (lambda: nn2(a=None), ARG, b"null"), (lambda: nn2(w=None), ARG, b"null"),
        (lambda: ratio(d=0), ARG, b"D=0"), (lambda: ratio(d=65), UNSUP, b"D=65"), (lambda: ratio(n1=1), ARG, b"N1=1"),
        (lambda: ratio(fd=None), ARG, b"null"), (lambda: ratio(bb=None), ARG, b"null"),
        (lambda: gpf(g=0), ARG, b"grid_wid=0"), (lambda: gpf(g=65), UNSUP, b"grid_wid=65"),
        (lambda: gpf(wb=gb - 1), ARG, b"workspace"), (lambda: gpf(x=None), ARG, b"null"),
        (lambda: gpf(w=None), ARG, b"null"), (lambda: gpf(factor=-1.0), ARG, b"gpf_factor"),
        (lambda: gpf(factor=float("nan")), ARG, b"gpf_factor"), (lambda: gpf(n0=0), ARG, b"N0=0"),
        (lambda: gpf(n0=262145), UNSUP, b"N0=262145"),
        (lambda: refit(p=None), ARG, b"null"), (lambda: refit(t=None), ARG, b"null"), (lambda: refit(n=0), ARG, b"N=0"),
        (lambda: refit(r=0.0), ARG, b"radius"),
    ]:
        assert call() == want and word in L.pdsc_last_error(), word
    torch.cuda.synchronize(dev)
    assert all(bool((v == -7).all()) for v in outs.values()) and all(bool((v == -7.0).all()) for v in fo.values())
    assert bool((tr == -7.0).all()) and bool((ws == 0x5A).all())
    # and the same buffers are accepted once the arguments are right
    assert nn2() == 0 and ratio() == 0 and gpf() == 0 and refit() == 0
    torch.cuda.synchronize(dev)
    assert 0 <= int(outs["cnt"][0]) <= N0
