"""GC-RANSAC on the GPU (include/pdsc.h f10, pointdsc_amd/csrc/gc_ransac.hip)
against its numpy fp64 restatement tests/gc_reference.py: the grid exactly, the
labelling exactly from the same pose bits (energies to 1e-12), the solver's
stages, the whole call and the drivers.  Every case compared exactly is free of
near-ties on the reference alone (tests/test_gc_reference.py holds that)."""
import types

import numpy as np
import pytest
import torch

import fr_reference as F
import gc_reference as G

pytestmark = pytest.mark.gpu


def _t(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def test_library_constants():
    from pointdsc_amd import gc_ransac as M
    assert M.gc_ransac_round() == G.ROUND and M.gc_cell_bounds() == (G.WAVE_CELL, G.LDS_CELL)


# ------------------------------------------------------------------------ grid
@pytest.mark.parametrize("name", [*G.GRID_SHAPES, "flat_axis", "far_outlier"], ids=str)
def test_grid(name, gpu_device):
    from pointdsc_amd import gc_grid
    src, tgt, g = G.grid_inputs(name)
    ref = G.gc_grid(src, tgt, g)
    order, cell_start, cell_of, n_cells = gc_grid(_t(src, gpu_device), _t(tgt, gpu_device), g)
    nc = int(n_cells.item())
    assert nc == ref["n_cells"]
    assert np.array_equal(_np(order), ref["order"])
    assert np.array_equal(_np(cell_start)[:nc + 1], ref["cell_start"])
    assert np.array_equal(_np(cell_of), ref["cell_of"])
    again = gc_grid(_t(src, gpu_device), _t(tgt, gpu_device), g)
    assert all(torch.equal(a, b) for a, b in zip(again, (order, cell_start, cell_of, n_cells)))


def test_grid_above_the_lds_sort(gpu_device):
    """N > 2048: the sort runs in global memory."""
    from pointdsc_amd import gc_grid
    src, tgt = G.RR.make_case(77, 5000, 0.5)[:2]
    ref = G.gc_grid(src, tgt, 3)
    order, cell_start, cell_of, n_cells = gc_grid(_t(src, gpu_device), _t(tgt, gpu_device), 3)
    nc = int(n_cells.item())
    assert nc == ref["n_cells"] and np.array_equal(_np(order), ref["order"])
    assert np.array_equal(_np(cell_start)[:nc + 1], ref["cell_start"]) and np.array_equal(_np(cell_of), ref["cell_of"])


# ----------------------------------------------------------------------- label
@pytest.mark.parametrize("name", sorted(G.LABEL_CASES))
@pytest.mark.parametrize("lam", G.LABEL_LAMBDAS)
def test_label(name, lam, gpu_device):
    from pointdsc_amd import gc_grid, gc_label
    src, tgt, g, pose = G.label_inputs(name)
    grid, ref = G.label_reference(name, lam)
    assert G.label_tie_free(ref["diag"])
    s, t = _t(src, gpu_device), _t(tgt, gpu_device)
    dgrid = gc_grid(s, t, g)
    nc = int(dgrid[3].item())
    assert nc == grid["n_cells"] and np.array_equal(_np(dgrid[0]), grid["order"])
    labels, count, dbg = gc_label(_t(pose, gpu_device, torch.float64), s, t, dgrid, G.EPS, lam, debug=True)
    d2 = _np(dbg["d2"])
    print(name, lam, "count", int(count.item()), "ref", ref["count"], "max |d2 - ref|", np.abs(d2 - ref["d2"]).max())
    assert np.array_equal(_np(dbg["m_star"])[:nc], ref["m_star"])
    assert np.array_equal(_np(labels), ref["labels"]) and int(count.item()) == ref["count"]
    assert np.all(np.abs(d2 - ref["d2"]) <= 1e-12 * np.maximum(ref["d2"], 1.0))
    e = _np(dbg["energy"])[:nc]
    assert np.all(np.abs(e - ref["energy"]) <= 1e-12 * np.abs(ref["energy"])), np.abs(e - ref["energy"]).max()
    gap = _np(dbg["energy_gap"])[:nc]
    assert np.all(np.abs(gap - ref["energy_gap"]) <= 1e-12 * np.maximum(np.abs(ref["energy"]), 1.0))
    again = gc_label(_t(pose, gpu_device, torch.float64), s, t, dgrid, G.EPS, lam, debug=True)
    assert torch.equal(again[0], labels) and torch.equal(again[1], count)
    assert np.array_equal(_bits(_np(again[2]["energy"])[:nc]), _bits(e))


# ---------------------------------------------------------------------- solver
def _run(dev, src, tgt, **kw):
    from pointdsc_amd.gc_ransac import gc_ransac
    return gc_ransac(_t(src, dev), _t(tgt, dev), G.EPS, **kw)


def test_stages(gpu_device):
    S = G.STAGE
    src, tgt = G.solver_inputs(S["N"], S["ratio"], S["data_seed"])
    ref = G.stage_reference()
    assert G.tie_free(ref["diag"])
    res = _run(gpu_device, src, tgt, spatial_coherence_weight=S["lam"], neighborhood_size=S["G"],
               max_iteration=S["H"], confidence=1.0,
               seed=S["seed"], debug=True)
    d = {k: _np(v) for k, v in res.debug.items()}
    assert np.array_equal(d["samples"], ref["samples"])
    assert np.array_equal(d["count"], ref["count"])  # status and counts
    v = ref["count"] >= 0
    err = np.abs(d["score"][v] - ref["hyp_score"][v]) / np.maximum(ref["hyp_score"][v], 1e-300)
    perr = np.abs(d["trans"][v] - ref["trans"][v]).max()
    print("stages: max rel score error", err[ref["hyp_score"][v] > 0].max(), " max pose error", perr)
    assert np.all(np.abs(d["score"][v] - ref["hyp_score"][v]) <= 1e-12 * ref["hyp_score"][v])
    assert perr <= 1e-9
    _check_whole(res, ref)


def _check_whole(res, ref):
    assert (res.best, res.iterations, res.lo_runs, res.lo_steps, res.n_inliers, res.n_cells) == \
        (ref["best"], ref["iterations"], ref["lo_runs"], ref["lo_steps"], ref["n_inliers"], ref["n_cells"])
    assert np.array_equal(_np(res.labels), ref["labels"])
    T = _np(res.transformation)
    assert np.abs(T - ref["transformation"]).max() <= 1e-9
    assert abs(res.score - ref["score"]) <= 1e-12 * max(ref["score"], 1e-300)
    assert np.array_equal(_bits(_np(res.transformation_f32)), _bits(T.astype(np.float32)))
    assert res.score >= ref["best_minimal_score"] * (1 - 1e-12)


@pytest.mark.parametrize("name", sorted(G.WHOLE_CASES))
@pytest.mark.parametrize("lo", [False, True])
def test_whole_call(name, lo, gpu_device):
    ratio, rounds, data_seed, seed = G.WHOLE_CASES[name]
    src, tgt = G.solver_inputs(G.WHOLE_N, ratio, data_seed)
    ref = G.whole_reference(name, lo)
    assert G.tie_free(ref["diag"])
    kw = dict(spatial_coherence_weight=G.WHOLE_LAMBDA, neighborhood_size=G.WHOLE_G, max_iteration=rounds * G.ROUND,
              confidence=1.0, seed=seed, local_optimization=lo)
    res = _run(gpu_device, src, tgt, **kw)
    print(name, lo, "best", res.best, "score", res.score, "inliers", res.n_inliers, "lo", res.lo_runs, res.lo_steps)
    _check_whole(res, ref)
    again = _run(gpu_device, src, tgt, **kw)
    assert np.array_equal(_bits(_np(again.transformation)), _bits(_np(res.transformation)))
    assert torch.equal(again.labels, res.labels) and again.score == res.score
    # the refit is pdsc_refit_inliers': on its own output's inliers it is a fixed point only by chance, but the
    # labels it reports are those of the pose before the refit, as n_inliers
    assert int(_np(res.labels).sum()) == res.n_inliers


def test_lo_off_ignores_lambda(gpu_device):
    ratio, rounds, data_seed, seed = G.WHOLE_CASES["r30_one_round"]
    src, tgt = G.solver_inputs(G.WHOLE_N, ratio, data_seed)
    kw = dict(max_iteration=G.ROUND, confidence=1.0, seed=seed, local_optimization=False)
    a = _run(gpu_device, src, tgt, spatial_coherence_weight=0.0, **kw)
    b = _run(gpu_device, src, tgt, spatial_coherence_weight=0.73, **kw)
    assert np.array_equal(_bits(_np(a.transformation)), _bits(_np(b.transformation)))
    assert torch.equal(a.labels, b.labels) and (a.best, a.score, a.n_inliers) == (b.best, b.score, b.n_inliers)


def test_confidence_stops_after_round_0(gpu_device):
    e = G.EARLY
    src, tgt = G.solver_inputs(G.WHOLE_N, e["ratio"], e["data_seed"])
    res = _run(gpu_device, src, tgt, spatial_coherence_weight=G.WHOLE_LAMBDA, neighborhood_size=G.WHOLE_G,
               max_iteration=e["rounds"] * G.ROUND, confidence=e["confidence"], seed=e["seed"])
    one = G.whole_reference("r30_one_round", True)  # the same inputs, stopped by H instead
    assert res.iterations == G.ROUND
    _check_whole(res, one)


# --------------------------------------------------------------------- drivers
_FR = {}


def _fr_case():
    if not _FR:
        _FR["in"] = F.planted_registration(F.planted_seed())
    return _FR["in"]


def _gc_args(**kw):
    base = dict(mode="MFR", algo="GC", iters=4096, ELC=False, GPF_grid_wid=10, GPF_factor=1.0,
                spatial_coherence_weight=0.1, GC_conf=0.999, GC_LO=True, prosac=False, use_edge_len=False,
                use_sprt=True)
    return types.SimpleNamespace(**dict(base, **kw))


def _nn_pairs(xyz0, xyz1, f0, f1):
    nn = np.argmin(((f0[:, None, :] - f1[None, :, :]) ** 2).sum(2), 1)
    return xyz0, xyz1[nn]


def test_drivers(gpu_device):
    from pointdsc_amd import FR, GC_RANSAC, GCRANSAC
    xyz0, xyz1, f0, f1, T_gt = _fr_case()
    A, B = (_t(x, gpu_device) for x in _nn_pairs(xyz0, xyz1, f0, f1))
    # GC_RANSAC: (pose, elapsed_time), the pose source -> target as the reference's pose_T.T
    T, dt = GC_RANSAC(A, B, 0.6, 4096, _gc_args(), None, seed=5)
    assert isinstance(dt, float) and dt > 0 and T.shape == (4, 4) and T.dtype == torch.float64
    err = np.abs(_np(T) - T_gt).max()
    print("GC_RANSAC max |T - planted|:", err)
    assert err <= 1e-3
    T2, _ = GC_RANSAC(A, B, 0.6, 4096, _gc_args(GC_LO=False), None, seed=5)
    assert np.abs(_np(T2) - T_gt).max() <= 1e-3
    with pytest.raises(NotImplementedError, match="prosac"):
        GC_RANSAC(A, B, 0.6, 4096, _gc_args(prosac=True), np.zeros(len(xyz0)), seed=5)
    with pytest.raises(NotImplementedError, match="use_edge_len"):
        GC_RANSAC(A, B, 0.6, 4096, _gc_args(use_edge_len=True), None, seed=5)
    assert np.array_equal(_np(GC_RANSAC(A[:2], B[:2], 0.6, 64, _gc_args(), None)[0]), np.eye(4))
    # GCRANSAC: the baselines' (pred_trans [1,4,4], pred_labels [1,N])
    N = A.shape[0]
    corr = torch.cat([A, B], 1)[None]
    trans, labels = GCRANSAC(corr, A[None], B[None], inlier_threshold=0.1, max_iteration=4096, seed=5)
    assert trans.shape == (1, 4, 4) and trans.dtype == torch.float32 and labels.shape == (1, N)
    assert set(np.unique(_np(labels))) <= {0.0, 1.0} and _np(labels).sum() >= 0.3 * N
    err = np.abs(_np(trans[0]).astype(np.float64) - T_gt).max()
    print("GCRANSAC max |T - planted|:", err)
    assert err <= 1e-3
    # FR(algo="GC"): the 8-tuple, no refit step
    dev_in = [_t(x, gpu_device) for x in (xyz0, xyz1, f0, f1)]
    for mode in ("no_filter", "MFR", "GPF"):
        out = FR(*dev_in, _gc_args(mode=mode), T_gt, seed=5)
        assert len(out) == 8 and out[2] is dev_in[0] and out[3] is dev_in[1] and out[1] > 0
        err = np.abs(_np(out[0]) - T_gt).max()
        print("FR GC", mode, "pairs", out[6], "of", out[4], " max |T - planted|:", err)
        assert _np(out[0]).dtype == np.float64 and err <= 1e-3
        again = FR(*dev_in, _gc_args(mode=mode), T_gt, seed=5)
        assert np.array_equal(_bits(_np(again[0])), _bits(_np(out[0])))
    with pytest.raises(NotImplementedError, match="prosac"):
        FR(*dev_in, _gc_args(prosac=True), T_gt)
    # without the GC options FR still refuses, naming the missing one
    bare = types.SimpleNamespace(mode="MFR", algo="GC", iters=64, ELC=True, GPF_grid_wid=10, GPF_factor=1.0)
    with pytest.raises(NotImplementedError, match="spatial_coherence_weight"):
        FR(*dev_in, bare, T_gt)
    # fewer than 3 filtered pairs: the identity
    out = FR(*[x[:50] for x in dev_in], _gc_args(mode="GPF", GPF_factor=0.0), T_gt)
    assert out[6] == 0 and np.array_equal(_np(out[0]), np.eye(4))
