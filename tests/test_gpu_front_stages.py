"""The forward's front half on the GPU against the exact references of
tests/front_reference.py (run with -m gpu): pdsc_compat_f32 / pdsc_compat_packed_f32
(a1), pdsc_pick_seeds (a5), pdsc_seed_knn (a6) and pdsc_mutual_nn /
pdsc_build_correspondences (f1) at the shapes where compat.hip, seeds.hip, knn.hip's
knn kernels and corr.hip take another path.  Everything goes through the C ABI
(pointdsc_amd._lib) on output buffers prefilled with a sentinel, so an unwritten slot
shows; every form is reached by shape under the default knobs, and where
pdsc_launch_plan reports the form it is asserted.  The cases and their
preconditions: tests/test_front_reference.py."""
import ctypes

import numpy as np
import pytest
import torch

import front_reference as R
from oracle import pdsc_oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32


def _t(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _lib():
    from pointdsc_amd import _lib as lib
    return lib.load(), lib.check


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _ids(cases):
    return [c["id"] for c in cases]


# ===================================================================== a1
def _compat(src, tgt, sigma, dev, packed):
    """The raw output of one entry point on a NaN-prefilled buffer."""
    L, check = _lib()
    B, N, _ = src.shape
    s, t, sg = _t(src, dev), _t(tgt, dev), _t(f32([sigma]), dev)
    if packed:
        nf = L.pdsc_compat_packed_floats(N)
        assert nf == R.packed_floats(N)
        out = torch.full((B, nf), float("nan"), dtype=torch.float32, device=dev)
        check(L.pdsc_compat_packed_f32(_p(s), _p(t), B, N, _p(sg), _p(out), _stream(dev)), "pdsc_compat_packed_f32")
    else:
        out = torch.full((B, N, N), float("nan"), dtype=torch.float32, device=dev)
        check(L.pdsc_compat_f32(_p(s), _p(t), B, N, _p(sg), _p(out), _stream(dev)), "pdsc_compat_f32")
    return out.cpu().numpy()


def _assert_compat(src, tgt, sigma, dev):
    """Both entry points bit for bit against the oracle; the packed buffer whole:
    no NaN left, the tiles in include/pdsc.h's order, everything past N exactly +0."""
    ref = R.compat_reference(src, tgt, sigma)
    nan = np.isnan(ref)
    M = _compat(src, tgt, sigma, dev, packed=False)
    Mp = _compat(src, tgt, sigma, dev, packed=True)
    for b in range(len(src)):
        assert np.array_equal(np.isnan(M[b]), nan[b])
        assert np.array_equal(_bits(M[b])[~nan[b]], _bits(ref[b])[~nan[b]]), f"dense pair {b}"
        want = R.pack_symmetric(ref[b])
        wn = np.isnan(want)
        assert np.array_equal(np.isnan(Mp[b]), wn), f"packed pair {b}: NaN left in the buffer"
        assert np.array_equal(_bits(Mp[b])[~wn], _bits(want)[~wn]), f"packed pair {b}"
    return ref


@pytest.mark.parametrize("N", R.COMPAT_SIZES)
def test_compat_sizes(N, gpu_device):
    src, tgt = R.compat_pairs(N)
    ref = _assert_compat(src, tgt, R.COMPAT_SIGMA, gpu_device)
    assert N < 31 or ((ref > 0) & (ref < 1)).any()


@pytest.mark.parametrize("sigma", R.ZERO_PROOF_SIGMAS)
def test_compat_zero_proof_boundary(sigma, gpu_device):
    """|ds - dt| = sigma (1 + delta), delta = 0, +-2^-12 .. +-2^-6, on both sides of the
    packed kernel's square-root-free zero test and of its xs + xt <= 2^20 sigma^2 guard."""
    src, tgt = R.zero_proof_pair(sigma)
    _assert_compat(src, tgt, sigma, gpu_device)


@pytest.mark.parametrize("sigma", R.SIGMA_OUTSIDE)
def test_compat_sigma_outside_fast_path(sigma, gpu_device):
    """sigma_d^2 subnormal / >= 1e30: the library sqrtf and division branch."""
    src, tgt = R.compat_pairs(R.SIGMA_OUTSIDE_N, dups=5)
    _assert_compat(src, tgt, sigma, gpu_device)


# ===================================================================== a5
def _plan(B, N, S):
    """pdsc_launch_plan's (seed_rows, nms_rpt, seed_rank, seed_wpb) for S = int(N * ratio) seeds."""
    from pointdsc_amd import _lib as lib
    L, check = _lib()
    cfg = lib.make_config(ratio=R.plan_ratio(N, S))
    out = (ctypes.c_int32 * 13)()
    check(L.pdsc_launch_plan(ctypes.byref(cfg), B, N, out, 13), "pdsc_launch_plan")
    return out[6], out[7], out[8], out[9]


def _pick_seeds(src, conf, radius, S, dev):
    """(seeds [B,S], is_local_max [B,N]) on buffers prefilled with -1 / NaN."""
    L, check = _lib()
    B, N = conf.shape
    seeds = torch.full((B, S), -1, dtype=torch.int32, device=dev)
    lm = torch.full((B, N), float("nan"), dtype=torch.float32, device=dev)
    s, c = _t(src, dev), _t(conf, dev)
    check(L.pdsc_pick_seeds(_p(s), _p(c), B, N, float(radius), S, _p(seeds), _p(lm), _stream(dev)), "pdsc_pick_seeds")
    return seeds.cpu().numpy(), lm.cpu().numpy()


def _assert_seeds(src, conf, radius, S, dev, pairs=None):
    seeds, lm = _pick_seeds(src, conf, radius, S, dev)
    for b in (range(len(src)) if pairs is None else pairs):
        r_seeds, r_lm = R.seed_reference(src[b], conf[b], radius, S)
        assert np.array_equal(_bits(lm[b]), _bits(r_lm)), (b, np.nonzero(lm[b] != r_lm)[0][:8])
        assert np.array_equal(seeds[b], r_seeds), (b, S, np.nonzero(seeds[b] != r_seeds)[0][:8])
    return seeds, lm


@pytest.mark.parametrize("B", R.SEED_BS)
@pytest.mark.parametrize("N", R.SEED_SIZES)
def test_pick_seeds_sizes(N, B, gpu_device):
    """Flags and list bit-exact for S = 1, N // 10 and N: duplicate points, heavy
    ties, +-0, negative maxima, an all-equal pair and one with -inf confidences."""
    src, conf = R.seed_case(B, N)
    for S in R.seed_counts(N):
        if N >= 2:  # B = 1: the one-row NMS on 16-row blocks; B = 3: two rows per thread; compare ranking
            assert _plan(B, N, S)[:3] == (16, 1 if B == 1 else 2, 0)
        _assert_seeds(src, conf, R.SEED_RADIUS, S, gpu_device)


@pytest.mark.parametrize("c", R.SEED_PLAN_CASES, ids=_ids(R.SEED_PLAN_CASES))
def test_pick_seeds_forms_by_shape(c, gpu_device):
    """The 64-row kernels, the select ranking and its compare fallback, each reached
    by the shape alone; the form asserted through pdsc_launch_plan."""
    B, N, S = c["B"], c["N"], c["S"]
    assert _plan(B, N, S)[:3] == c["plan"]
    src, conf = R.seed_plan_case(B, N, S)
    _assert_seeds(src, conf, R.SEED_RADIUS, S, gpu_device)


@pytest.mark.parametrize("name", R.RADIUS_CASES)
def test_pick_seeds_radius_edges(name, gpu_device):
    """R = 0, distances exactly R, R^2 underflowing (subnormal threshold) and
    overflowing (+inf threshold): the oracle's sqrtf form is the truth."""
    src, conf, radius = R.radius_case(name)
    _assert_seeds(src, conf, radius, 13, gpu_device)


def test_pick_seeds_pair_isolation(gpu_device):
    """A pair of NaN confidences changes nothing in its neighbours' results."""
    src, conf = R.isolation_case()
    S = R.ISOLATION["S"]
    seeds, lm = _pick_seeds(src, conf, R.SEED_RADIUS, S, gpu_device)
    for b in (0, 2):
        s1, l1 = _pick_seeds(src[b:b + 1], conf[b:b + 1], R.SEED_RADIUS, S, gpu_device)
        assert np.array_equal(_bits(lm[b]), _bits(l1[0])) and np.array_equal(seeds[b], s1[0])
    _assert_seeds(src, conf, R.SEED_RADIUS, S, gpu_device, pairs=(0, 2))
    torch.cuda.synchronize(gpu_device)
    assert float(torch.ones(8, device=gpu_device).sum().item()) == 8.0  # the stream is healthy


# ===================================================================== a6
GUARD = 4096


def _seed_knn(normed, seeds, k, precision, dev):
    """knn [B,S,k] on a buffer prefilled with -1; the workspace is followed by a guard
    that must stay untouched."""
    from pointdsc_amd import _lib as lib
    L, check = _lib()
    B, N, C = normed.shape
    S = seeds.shape[1]
    nb = L.pdsc_seed_knn_workspace_bytes(B, N, S)
    ws = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((B, S, k), -1, dtype=torch.int32, device=dev)
    f, s = _t(normed, dev), _t(seeds, dev, torch.int32)
    check(L.pdsc_seed_knn(_p(f), _p(s), B, N, C, S, k, lib.precision_code(precision), _p(out), _p(ws), nb,
                          _stream(dev)), "pdsc_seed_knn")
    assert bool((ws[nb:] == 0xA5).all()), "pdsc_seed_knn wrote past its workspace"
    return out.cpu().numpy()


@pytest.mark.parametrize("precision", ["h3", "f32"])
@pytest.mark.parametrize("c", R.KNN_CASES, ids=_ids(R.KNN_CASES))
def test_seed_knn_rows_vs_fp64(c, precision, gpu_device):
    """Every row of every pair by front_reference.check_knn_row (eps 2e-6, both
    precisions); on planted duplicates the tie group in index order, exactly."""
    d = R.knn_case(c)
    B, N, S, k = (c[n] for n in "BNSk")
    knn = _seed_knn(d["normed"], d["seeds"], k, precision, gpu_device)
    for b in range(B):
        f = d["normed"][b].astype(np.float64)
        d64 = 2.0 - 2.0 * (f[d["seeds"][b]] @ f.T)
        g = d["groups"][b]
        for r, s in enumerate(d["seeds"][b]):
            try:
                R.check_knn_row(knn[b, r], d64[r], k)
            except AssertionError as e:
                raise AssertionError(f"pair {b} seed row {r} (index {s}): {e}") from None
            if len(g) and s in g:
                lead = R.tie_group_row(g, k)
                assert np.array_equal(knn[b, r, :len(lead)], lead), (b, r, s)
        if len(g):  # ... which is the oracle's stable-argsort row on that group
            ref = O.knn_seed_rows(d["normed"][b], d["seeds"][b], k)
            for r, s in enumerate(d["seeds"][b]):
                on = np.isin(ref[r], g) & (s in g)
                assert np.array_equal(knn[b, r][on], ref[r][on]), (b, r, s)


def test_seed_knn_four_seeds_per_workgroup_plan():
    """The (16, 300, 129) case runs 4 seeds per workgroup (B ceil(S / 4) >= 512):
    pdsc_launch_plan with int(N * ratio) = 129 reports seed_wpb = 4."""
    assert _plan(16, 300, 129)[3] == 4
    assert _plan(2, 300, 129)[3] == 1


# ===================================================================== f1
def _build(src, tgt, sd, td, mutual, gt, dev):
    """pdsc_build_correspondences on sentinel-filled outputs: (status, dict of host arrays)."""
    L, _ = _lib()
    Ns, D = sd.shape
    Nt = td.shape[0]
    nb = L.pdsc_mutual_nn_workspace_bytes(Ns, Nt)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    nan = float("nan")
    o = dict(corr=torch.full((Ns, 2), -1, dtype=torch.int32, device=dev),
             count=torch.full((1,), -1, dtype=torch.int32, device=dev),
             corr_pos=torch.full((Ns, 6), nan, dtype=torch.float32, device=dev),
             src_keypts=torch.full((Ns, 3), nan, dtype=torch.float32, device=dev),
             tgt_keypts=torch.full((Ns, 3), nan, dtype=torch.float32, device=dev),
             labels=torch.full((Ns,), nan, dtype=torch.float32, device=dev))
    g = _t(gt.reshape(-1), dev, torch.float64) if gt is not None else None
    a, b, s, t = _t(sd, dev), _t(td, dev), _t(src, dev), _t(tgt, dev)
    st = L.pdsc_build_correspondences(_p(a), _p(b), _p(s), _p(t), Ns, Nt, D, int(mutual), _p(g), 0.10, _p(o["corr"]),
                                      _p(o["count"]), _p(o["corr_pos"]), _p(o["src_keypts"]), _p(o["tgt_keypts"]),
                                      _p(o["labels"]) if g is not None else None, _p(ws), nb, _stream(dev))
    torch.cuda.synchronize(dev)
    return st, {k: v.cpu().numpy() for k, v in o.items()}


def _assert_corr(o, ref, gt):
    """The list equal to the oracle's; keypoints and corr_pos bit-exact; labels exact
    away from the threshold; every row past count untouched."""
    n = int(o["count"][0])
    assert n == len(ref["corr"])
    assert np.array_equal(o["corr"][:n], ref["corr"])
    assert np.array_equal(_bits(o["src_keypts"][:n]), _bits(ref["src_keypts"]))
    assert np.array_equal(_bits(o["tgt_keypts"][:n]), _bits(ref["tgt_keypts"]))
    assert np.array_equal(_bits(o["corr_pos"][:n]), _bits(ref["corr_pos"]))
    assert (o["corr"][n:] == -1).all()
    for name in ("corr_pos", "src_keypts", "tgt_keypts", "labels"):
        assert np.isnan(o[name][n:]).all(), name
    if gt is not None:
        far = np.abs(ref["label_distance"] - 0.10) > 1e-9
        assert np.array_equal(o["labels"][:n][far], ref["labels"][far])
    else:
        assert np.isnan(o["labels"]).all()


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("shape", sorted(R.CORR_EDGE_SEEDS), ids=str)
def test_build_correspondences_edge_shapes(shape, mutual, gpu_device):
    """D = 1 and 64, a tile boundary in either direction, corr_select_kernel's
    1024-row chunk: the list equal to the oracle's (every nearest neighbour has a
    margin >= 1e-5), then the bit-exact bars."""
    Ns, Nt, D = shape
    src, tgt, sd, td, gt = R.corr_pair(Ns, Nt, D, R.CORR_EDGE_SEEDS[shape])
    ref = O.build_correspondences(src, tgt, sd, td, use_mutual=mutual, gt_trans=gt, inlier_threshold=0.10)
    st, o = _build(src, tgt, sd, td, mutual, gt, gpu_device)
    assert st == 0
    _assert_corr(o, ref, gt)


def test_build_correspondences_fewest_mutual_pairs(gpu_device):
    """Every source picks target 0, so exactly one pair is mutual (an empty mutual
    set does not exist: the first global minimum of the distance matrix is always
    mutual); nothing past that one row may be touched, with and without labels."""
    src, tgt, sd, td = R.single_mutual_pair()
    ref = O.build_correspondences(src, tgt, sd, td)
    assert len(ref["corr"]) == 1
    st, o = _build(src, tgt, sd, td, True, None, gpu_device)
    assert st == 0 and int(o["count"][0]) == 1
    _assert_corr(o, ref, None)


def test_mutual_nn_first_index_across_tiles(gpu_device):
    """Identical target descriptors either side of the 64-column tile edge: the lower
    index wins, as numpy.argmin."""
    from pointdsc_amd.correspondence import mutual_nn
    for sd, td, rows, expect in R.straddle_ties():
        ref = O.build_correspondences(np.zeros((len(sd), 3), f32), np.zeros((len(td), 3), f32), sd, td)
        si, ti = mutual_nn(_t(sd, gpu_device), _t(td, gpu_device))
        si, ti = si.cpu().numpy(), ti.cpu().numpy()
        assert (si[rows] == expect).all()
        assert np.array_equal(si, ref["source_idx"]) and np.array_equal(ti, ref["target_idx"])
