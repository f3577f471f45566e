"""The fp64 RANSAC restatement of tests/ransac_reference.py on the CPU (its own
properties, before tests/test_gpu_ransac.py holds the kernels to it), the
preconditions of every GPU case (a seed that lands on a near-tie fails here and
not on the GPU), and the f6 additions to the C ABI without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import ransac_reference as R
from conftest import ROOT


def test_mix64_hand_computed():
    """splitmix64 from state 0: its first two outputs are mix64(0) and
    mix64(0x9E3779B97F4A7C15) (the finaliser adds the increment itself), and
    mix64(1) by hand: 1 + 0x9E3779B97F4A7C15 = 0x9E3779B97F4A7C16, then the three
    xor-shift / multiply steps."""
    got = R.mix64(np.array([0, 0x9E3779B97F4A7C15, 1], np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x910A2DEC89025CC1]

    def by_hand(z):  # python integers, masked
        m = (1 << 64) - 1
        z = (z + 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)

    for z in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 0x0123456789ABCDEF):
        assert int(R.mix64(np.array([z], np.uint64))[0]) == by_hand(z)


def test_draw_is_the_header_formula():
    N, seed = 257, 0xFFFFFFFFFFFFFFF0  # seed + k GOLDEN wraps
    got = R.draw(seed, np.array([0, 1, 1000, 2 ** 31 - 1]), 4, N)
    m = (1 << 64) - 1
    for row, h in zip(got, (0, 1, 1000, 2 ** 31 - 1)):
        for j in range(4):
            u = int(R.mix64(np.array([(seed + (8 * h + j) * 0x9E3779B97F4A7C15) & m], np.uint64))[0])
            assert row[j] == ((u >> 32) * N) >> 32 and 0 <= row[j] < N


def test_recovers_pose_without_outliers_and_noise():
    src, _, true, _ = R.make_case(5, 80, 1.0, noise=0.0)
    tgt = src.astype(np.float64) @ true[:3, :3].T + true[:3, 3]  # fp64 targets: exact correspondences
    ref = R.ransac(src, tgt, 0.1, 3, 0.0, 200, 1.0, 3)
    assert ref["n_inliers"] == 80 and ref["fitness"] == 1.0 and ref["best"] >= 0
    np.testing.assert_allclose(ref["transformation"], true, atol=1e-12)
    assert ref["inlier_rmse"] < 1e-12
    refit = R.ransac(src, tgt, 0.1, 3, 0.0, 200, 1.0, 3, refit=True)
    np.testing.assert_allclose(refit["transformation"], true, atol=1e-12)
    assert np.array_equal(refit["labels"], ref["labels"])
    # f = 1 stops a call with confidence < 1 after its first round
    stop = R.ransac(src, tgt, 0.1, 3, 0.0, 200, 0.999, 3, round_size=50)
    assert stop["iterations"] == 50 and np.all(stop["count"][50:] == -3) and np.all(stop["count"][:50] != -3)


def test_order_and_status_rows():
    src, tgt = R.stage_inputs(63)
    ref = R.ransac(src, tgt, 0.1, 3, 0.9, 1000, 1.0, 7)
    c = ref["count"]
    assert (c == -1).any() and (c == -2).any() and (c >= 0).any() and not (c == -3).any()
    assert ref["n_validated"] == int((c >= 0).sum()) and ref["iterations"] == 1000
    v = np.flatnonzero(c >= 0)
    top = v[c[v] == c[v].max()]
    assert ref["best"] == top[np.lexsort((top, ref["sumsq"][top]))[0]]
    # the round size only matters through the stop rule
    again = R.ransac(src, tgt, 0.1, 3, 0.9, 1000, 1.0, 7, round_size=64)
    assert again["best"] == ref["best"] and np.array_equal(again["count"], c)


@pytest.mark.parametrize("N,n,H,es", R.STAGE_CASES)
def test_stage_cases_are_tie_free(N, n, H, es):
    """The stage tests compare the per-hypothesis rows, not the winner: at N = 3
    and 4 every valid hypothesis is a permutation of one sample and the winner
    is decided by rounding (sumsq gap 0), which those tests do not look at."""
    src, tgt = R.stage_inputs(N)
    ref = R.ransac(src, tgt, 0.1, n, es, H, 1.0, 7)
    assert R.tie_free(ref["diag"], winner=False), ref["diag"]


def test_stage_cases_cover_every_status():
    seen = set()
    for N, n, H, es in R.STAGE_CASES:
        if H == 1000:
            src, tgt = R.stage_inputs(N)
            seen |= set(np.unique(np.minimum(R.ransac(src, tgt, 0.1, n, es, H, 1.0, 7)["count"], 0)).tolist())
    assert seen == {0, -1, -2}


@pytest.mark.parametrize("name", sorted(R.WHOLE_CASES))
def test_whole_cases_are_tie_free(name):
    N, ratio, n, H, ds, ss = R.WHOLE_CASES[name]
    src, tgt, true, inl = R.make_case(ds, N, ratio)
    ref = R.ransac(src, tgt, 0.1, n, 0.0, H, 1.0, ss)
    print(name, ref["best"], ref["n_inliers"], ref["n_validated"], ref["diag"])
    assert R.tie_free(ref["diag"]), ref["diag"]
    assert ref["iterations"] == H and ref["n_inliers"] >= int(inl.sum()) - 2
    re_, te = R.pose_error(ref["transformation"], true)
    assert re_ < 2.0 and te < 0.05


def test_early_stop_cases_are_tie_free():
    N, ratio, n, ds, ss = R.EARLY["sparse"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = R.ransac(src, tgt, 0.1, n, 0.0, 8 * R.ROUND, 0.999, ss)
    assert R.tie_free(ref["diag"]), ref["diag"]
    assert ref["iterations"] % R.ROUND == 0 and ref["iterations"] < 8 * R.ROUND
    assert np.all(ref["count"][ref["iterations"]:] == -3) and np.all(ref["count"][:ref["iterations"]] != -3)
    N, ratio, n, ds, ss = R.EARLY["dense"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = R.ransac(src, tgt, 0.1, n, 0.0, 8 * R.ROUND, 0.999, ss)
    assert R.tie_free(ref["diag"]) and ref["iterations"] == R.ROUND


def test_baseline_case_reaches_the_pose():
    """The property tests/test_gpu_ransac.py asserts of baselines.RANSAC, on the
    reference first: a synthetic 30 %-inlier pair at N = 1000, ransac_n = 4, 1000
    iterations: RE < 1 degree and TE < 3 cm."""
    from pointdsc_amd.synthetic import synthetic_pair
    pair = synthetic_pair(1000, seed=11, inlier_ratio=0.3)
    ref = R.ransac(pair["src_keypts"], pair["tgt_keypts"], 0.10, 4, 0.0, 1000, 1.0, 0)
    assert R.tie_free(ref["diag"]), ref["diag"]
    re_, te = R.pose_error(ref["transformation"], pair["gt_trans"].astype(np.float64))
    print(ref["n_inliers"], re_, te)
    assert re_ < 1.0 and te < 0.03


def test_remaining_gpu_cases():
    """The other references tests/test_gpu_ransac.py compares exactly."""
    pair, _, rows = R.solver_case()
    sub = R.ransac(pair["src_keypts"][rows], pair["tgt_keypts"][rows], 0.10, 3, 0.0, 5000, 1.0, 4)
    assert R.tie_free(sub["diag"]) and sub["n_inliers"] >= 290
    N, ratio, n, H, ds, ss = R.WHOLE_CASES["partial_round"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    det = R.ransac(src, tgt, 0.1, n, 0.9, H, 1.0, ss)  # the determinism test's call
    assert R.tie_free(det["diag"]) and 0 < det["n_validated"] < H
    rej = R.ransac(*R.rejected_case(), 0.1, 3, 0.9, 300, 1.0, 2)
    assert rej["best"] == -1 and rej["n_validated"] == 0 and rej["diag"]["checker_margin"] >= 1e-7
    assert np.array_equal(rej["transformation"], np.eye(4)) and not rej["labels"].any()
    three = R.ransac(*R.make_case(3, 3, 1.0)[:2], 0.1, 3, 0.0, 200, 1.0, 3)
    assert three["n_inliers"] == 3 and three["diag"]["distance_margin"] >= 1e-7
    assert three["diag"]["sigma_ratio"] >= 1e-5


# ------------------------------------------------------------------ the C ABI
def test_header_symbols_in_ctypes_table():
    from pointdsc_amd import _lib
    src = open(os.path.join(ROOT, "include", "pdsc.h")).read()
    assert re.search(r"typedef struct pdsc_ransac_result", src) and re.search(r"typedef struct pdsc_ransac_debug", src)
    for name in ("pdsc_ransac_round", "pdsc_ransac_workspace_bytes", "pdsc_ransac_correspondence"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS, name
    assert "max_validation" in src  # the header says what is left out


def test_round_and_workspace_queries():
    from pointdsc_amd import _lib
    lib = _lib.load()
    rnd = lib.pdsc_ransac_round()
    assert rnd > 0 and rnd == R.ROUND and rnd & (rnd - 1) == 0
    sizes = [lib.pdsc_ransac_workspace_bytes(n) for n in (3, 4, 64, 256, 257, 1000, 5000, 20000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert lib.pdsc_ransac_workspace_bytes(0) == 0


def test_argument_errors_before_any_launch():
    """Bad arguments return PDSC_ERR_ARG / PDSC_ERR_UNSUPPORTED on the host (dummy
    non-null pointers: nothing is dereferenced, no device is needed)."""
    from pointdsc_amd import _lib
    lib = _lib.load()
    d = ctypes.c_void_p(16)

    def call(src=d, tgt=d, N=10, r=0.1, n=3, es=0.0, H=100, conf=1.0, ws=d, nb=1 << 40):
        return lib.pdsc_ransac_correspondence(src, tgt, N, r, n, es, H, conf, 0, 0, None, None, None, None, ws, nb,
                                              None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(N=2), dict(N=3, n=4), dict(N=0), dict(H=0), dict(H=-5), dict(r=0.0), dict(r=-0.1), dict(r=nan),
               dict(r=inf), dict(conf=0.0), dict(conf=1.5), dict(conf=-0.1), dict(conf=nan), dict(es=-0.1),
               dict(es=1.01), dict(es=nan), dict(src=None), dict(tgt=None), dict(ws=None), dict(nb=16)):
        assert call(**kw) == 1, kw
        assert lib.pdsc_last_error(), kw
    assert b"workspace" in lib.pdsc_last_error()
    for n in (2, 5, 0, -1):
        assert call(n=n) == 3, n
        assert b"ransac_n" in lib.pdsc_last_error()


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    import pointdsc_amd
    from pointdsc_amd.baselines import RANSAC
    x = torch.zeros(1, 10, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointdsc_amd.registration_ransac_based_on_correspondence(x[0], x[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pointdsc_amd.ransac_solver(x, x, torch.ones(1, 10), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RANSAC(torch.zeros(1, 10, 6), x, x)
