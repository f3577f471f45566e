"""The fp64 ICP restatement of tests/icp_reference.py on the CPU (its own
properties, before tests/test_gpu_icp.py holds the kernels to it), the
preconditions of the GPU cases (a seed that lands on a near-tie fails here and not
on the GPU), and the C ABI's new symbols in the ctypes table."""
import os
import re

import numpy as np
import pytest

import icp_reference as R
from conftest import ROOT

# (Ns, Nt, seed) of tests/test_gpu_icp.py
FULL_CASES = [(1000, 1500, 0), (257, 300, 0), (65, 64, 0), (512, 600, 0)]
EVAL_CASES = [(ns, nt, 100) for ns in (1, 63, 64, 65, 257, 1000) for nt in (1, 300, 1500)]


def test_recovers_known_motion_on_noiseless_cloud():
    rng = np.random.RandomState(7)
    src = (rng.rand(400, 3) * 2).astype(np.float32)
    true = R.rigid([1, 2, 3], 20.0, [0.3, -0.2, 0.5])
    tgt = R.transform(true, src)[rng.permutation(400)]  # fp64 targets: exact correspondences exist
    init = R.rigid([0, 1, 0], 1.5, [0.02, 0.0, -0.01]) @ true
    ref = R.registration_icp(src, tgt, 0.1, init)
    assert ref["fitness"] == 1.0 and ref["inlier_rmse"] < 1e-12
    np.testing.assert_allclose(ref["transformation"], true, atol=1e-12)
    assert 1 <= ref["iterations"] < 30


def test_no_correspondences_returns_init_after_one_identity_update():
    src, tgt, init, _ = R.make_case(3, 50, 60)
    far = init.copy()
    far[:3, 3] += 100.0
    ref = R.registration_icp(src, tgt, 0.1, far)
    assert np.array_equal(ref["transformation"], far)
    assert ref["iterations"] == 1 and ref["n_corr"] == 0 and ref["fitness"] == 0.0 and ref["inlier_rmse"] == 0.0
    assert np.all(ref["correspondence"] == -1)
    assert ref["d_fitness"] == [0.0] and ref["d_rmse"] == [0.0]


def test_max_iteration_zero_evaluates_init():
    src, tgt, init, _ = R.make_case(4, 80, 90)
    ref = R.registration_icp(src, tgt, 0.1, init, max_iteration=0)
    corr, _, fit, rmse, _, _ = R.evaluate(src, tgt, init, 0.1)
    assert np.array_equal(ref["transformation"], init) and ref["iterations"] == 0
    assert np.array_equal(ref["correspondence"], corr) and ref["fitness"] == fit and ref["inlier_rmse"] == rmse
    assert 0 < ref["n_corr"] < 80


def test_coincident_targets_resolve_to_the_lower_index():
    src, tgt, init, _ = R.make_case(5, 40, 50)
    corr = R.evaluate(src, tgt, init, 0.1)[0]
    tgt3 = np.repeat(tgt, 3, 0)  # target j -> 3 j, 3 j + 1, 3 j + 2
    corr3, _, _, _, gap, _ = R.evaluate(src, tgt3, init, 0.1)
    assert (corr >= 0).any() and gap == 0.0
    assert np.array_equal(corr3, np.where(corr >= 0, 3 * corr, -1))


def test_radius_is_inclusive_and_second_nearest_ignored():
    src = np.zeros((1, 3), np.float32)
    tgt = np.array([[0.5, 0, 0], [0.25, 0, 0], [2, 0, 0]], np.float32)
    assert R.evaluate(src, tgt, np.eye(4), 0.25)[0][0] == 1  # d^2 == r^2 exactly
    assert R.evaluate(src, tgt, np.eye(4), 0.2)[0][0] == -1


@pytest.mark.parametrize("ns,nt,seed", FULL_CASES)
def test_full_loop_cases_are_tie_free(ns, nt, seed):
    src, tgt, init, true = R.make_case(seed, ns, nt)
    ref = R.registration_icp(src, tgt, 0.1, init)
    print(ns, nt, ref["iterations"], ref["n_corr"], ref["min_gap"], ref["min_margin"], ref["d_fitness"], ref["d_rmse"])
    assert R.tie_free(ref)
    assert 1 < ref["iterations"] < 30 and ref["n_corr"] > ns // 2
    e0, e1 = R.pose_error(init, true), R.pose_error(ref["transformation"], true)
    assert e1[0] < e0[0] and e1[1] < e0[1]


@pytest.mark.parametrize("ns,nt,seed", EVAL_CASES)
def test_evaluation_cases_are_tie_free(ns, nt, seed):
    src, tgt, init, _ = R.make_case(seed, ns, nt)
    assert R.tie_free(R.registration_icp(src, tgt, 0.1, init, max_iteration=0))


def test_header_symbols_in_ctypes_table():
    from pointdsc_amd import _lib
    src = open(os.path.join(ROOT, "include", "pdsc.h")).read()
    assert re.search(r"typedef struct pdsc_icp_result", src)
    for name in ("pdsc_icp_workspace_bytes", "pdsc_icp_point_to_point"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.pdsc_icp_workspace_bytes(1000, 1500) > 0 and lib.pdsc_icp_workspace_bytes(0, 5) == 0


def test_argument_errors_before_any_launch():
    """Bad arguments return PDSC_ERR_ARG on the host (dummy non-null pointers:
    nothing is dereferenced, no device is needed)."""
    import ctypes
    from pointdsc_amd import _lib
    lib = _lib.load()
    d = ctypes.c_void_p(16)

    def call(ns=10, nt=10, r=0.1, it=30, ws=1 << 30):
        return lib.pdsc_icp_point_to_point(d, ns, d, nt, None, r, it, 1e-6, 1e-6, None, None, None, d, ws, None)

    for kw in (dict(ns=0), dict(nt=0), dict(r=0.0), dict(r=-1.0), dict(r=float("inf")), dict(r=float("nan")),
               dict(it=-1), dict(ws=16)):
        assert call(**kw) == 1, kw
        assert lib.pdsc_last_error()
    assert b"workspace" in lib.pdsc_last_error()
