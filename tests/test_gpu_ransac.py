"""RANSAC on correspondences (include/pdsc.h f6, pointdsc_amd/ransac.py) on the
GPU against the fp64 restatement tests/ransac_reference.py.  Every comparison
first asserts, on the reference's own diagnostics, that the case is free of
near-ties (distance and checker margins at least 1e-7 relative, sigma_2 /
sigma_1 of every sample at least 1e-5, the two best sumsq 1e-9 apart, the stop
rule's sides 1 % apart): the GPU differs from the reference in its SVD (fp64
Jacobi and a compensated Newton step, not extended precision), its fused
multiply-adds and its summation order, which then cannot flip an inlier, a
checker decision, the winner or the stop round.  That
condition selected the seeds (tests/test_ransac_reference.py checks it on the
CPU); it widens no tolerance.  Bounds: samples, status, counts, labels and the
winner exact; poses 1e-9 absolute; sumsq and inlier_rmse 1e-12 relative."""
import numpy as np
import pytest
import torch

import ransac_reference as R

pytestmark = pytest.mark.gpu

RADIUS = 0.1
_REF = {}


def _ref(key, src, tgt, **kw):
    """The reference of a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = R.ransac(src, tgt, RADIUS, **kw)
    return _REF[key]


def _run(dev, src, tgt, r=RADIUS, **kw):
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    return ransac(torch.from_numpy(np.ascontiguousarray(src, np.float32)).to(dev),
                  torch.from_numpy(np.ascontiguousarray(tgt, np.float32)).to(dev), None, r, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """Two results bitwise equal."""
    for f in ("transformation", "transformation_f32", "labels", "correspondence_set"):
        assert np.array_equal(_bits(_np(getattr(a, f))), _bits(_np(getattr(b, f)))), f
    assert np.array_equal(_bits(np.array([a.fitness, a.inlier_rmse])), _bits(np.array([b.fitness, b.inlier_rmse])))
    assert (a.n_inliers, a.iterations, a.best, a.n_validated) == (b.n_inliers, b.iterations, b.best, b.n_validated)
    if a.debug is not None and b.debug is not None:
        for k in a.debug:
            assert np.array_equal(_bits(_np(a.debug[k])), _bits(_np(b.debug[k]))), k


def _check_whole(res, ref, refit=False):
    assert (res.best, res.n_inliers, res.iterations, res.n_validated) == \
        (ref["best"], ref["n_inliers"], ref["iterations"], ref["n_validated"])
    assert np.array_equal(_np(res.labels), ref["labels"])
    assert res.fitness == ref["fitness"]
    T = _np(res.transformation)
    err = np.abs(T - ref["transformation"]).max()
    rel = abs(res.inlier_rmse - ref["inlier_rmse"]) / max(ref["inlier_rmse"], 1e-300)
    print("max |dT| vs fp64 reference:", err, " inlier_rmse relative:", rel)
    assert err <= 1e-9
    assert rel <= 1e-12
    assert np.array_equal(_bits(_np(res.transformation_f32)), _bits(T.astype(np.float32)))
    assert np.array_equal(_np(res.correspondence_set)[:, 0], np.flatnonzero(ref["labels"] > 0))


# ------------------------------------------------------------------- 1. stages
@pytest.mark.parametrize("N,n,H,es", R.STAGE_CASES)
def test_stages(N, n, H, es, gpu_device):
    src, tgt = R.stage_inputs(N)
    ref = _ref(("stage", N, n, H, es), src, tgt, ransac_n=n, edge_similarity=es, max_iteration=H, seed=7)
    assert R.tie_free(ref["diag"], winner=False)
    res = _run(gpu_device, src, tgt, ransac_n=n, edge_similarity=es, max_iteration=H, seed=7, debug=True)
    d = {k: _np(v) for k, v in res.debug.items()}
    assert np.array_equal(d["samples"], ref["samples"])
    assert np.array_equal(d["count"] < 0, ref["count"] < 0)
    assert np.array_equal(np.minimum(d["count"], 0), np.minimum(ref["count"], 0))  # the -1 / -2 status
    v = np.flatnonzero(ref["count"] >= 0)
    assert res.n_validated == len(v) and res.iterations == H
    if not len(v):
        assert res.best == -1
        return
    terr = np.abs(d["trans"][v] - ref["trans"][v]).max()
    rs = np.abs(d["sumsq"][v] - ref["sumsq"][v]) / np.maximum(ref["sumsq"][v], 1e-300)
    print("valid:", len(v), " max |dT|:", terr, " max relative sumsq error:", rs.max())
    assert terr <= 1e-9
    assert np.array_equal(d["count"][v], ref["count"][v])
    # the scoring kernel apart from the Kabsch: a recount from the GPU's own poses
    own = np.array([(R.distances2(d["trans"][h], src, tgt) < RADIUS * RADIUS).sum() for h in v])
    assert np.array_equal(d["count"][v], own)
    assert rs.max() <= 1e-12


# --------------------------------------------------------------- 2. whole call
@pytest.mark.parametrize("name", sorted(R.WHOLE_CASES))
def test_whole_call(name, gpu_device):
    from pointdsc_amd.ransac import ransac_round
    assert ransac_round() == R.ROUND
    N, ratio, n, H, ds, ss = R.WHOLE_CASES[name]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = _ref(("whole", name), src, tgt, ransac_n=n, max_iteration=H, seed=ss)
    assert R.tie_free(ref["diag"])
    _check_whole(_run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, seed=ss), ref)


# --------------------------------------------------------------- 3. early stop
def test_early_stop(gpu_device):
    N, ratio, n, ds, ss = R.EARLY["sparse"]
    H = 8 * R.ROUND
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = _ref("early-sparse", src, tgt, ransac_n=n, max_iteration=H, confidence=0.999, seed=ss)
    assert R.tie_free(ref["diag"]) and ref["iterations"] < H
    res = _run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, confidence=0.999, seed=ss, debug=True)
    _check_whole(res, ref)
    cnt = _np(res.debug["count"])
    assert np.all(cnt[res.iterations:] == -3) and np.all(cnt[:res.iterations] != -3)
    full = _ref(("whole", "eight_rounds"), src, tgt, ransac_n=n, max_iteration=H, seed=ss)  # the same pair and seed
    assert R.tie_free(full["diag"])
    res = _run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, confidence=1.0, seed=ss, debug=True)
    _check_whole(res, full)
    assert res.iterations == H and not np.any(_np(res.debug["count"]) == -3)
    N, ratio, n, ds, ss = R.EARLY["dense"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = _ref("early-dense", src, tgt, ransac_n=n, max_iteration=H, confidence=0.999, seed=ss)
    assert R.tie_free(ref["diag"]) and ref["iterations"] == R.ROUND
    _check_whole(_run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, confidence=0.999, seed=ss), ref)


# ------------------------------------------------ 4. determinism and isolation
def test_determinism_and_isolation(gpu_device, monkeypatch):
    from pointdsc_amd import _call as mod  # where the solver's workspace is allocated
    N, ratio, n, H, ds, ss = R.WHOLE_CASES["partial_round"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    kw = dict(ransac_n=n, edge_similarity=0.9, max_iteration=H, seed=ss, debug=True)
    a = _run(gpu_device, src, tgt, **kw)
    _same(a, _run(gpu_device, src, tgt, **kw))
    assert a.best >= 0 and 0 < a.n_validated < H
    # a dirty workspace (every byte 0xFF) on a side stream
    monkeypatch.setattr(mod, "_workspace", lambda nb, dev: torch.full((max(int(nb), 1),), 0xFF, dtype=torch.uint8,
                                                                      device=dev))
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        b = _run(gpu_device, src, tgt, **kw)
    side.synchronize()
    _same(a, b)
    monkeypatch.undo()
    c = _run(gpu_device, src, tgt, **dict(kw, seed=ss + 1))
    assert not np.array_equal(_np(c.debug["samples"]), _np(a.debug["samples"]))


# -------------------------------------------------------------------- 5. refit
def test_refit(gpu_device):
    N, ratio, n, H, ds, ss = R.WHOLE_CASES["odd_points"]
    src, tgt, true, _ = R.make_case(ds, N, ratio)
    ref = _ref(("whole", "odd_points"), src, tgt, ransac_n=n, max_iteration=H, seed=ss)
    assert R.tie_free(ref["diag"])
    plain = _run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, seed=ss)
    res = _run(gpu_device, src, tgt, ransac_n=n, max_iteration=H, seed=ss, refit=True)
    lab = _np(res.labels)
    assert np.array_equal(lab, _np(plain.labels)) and np.array_equal(lab, ref["labels"])
    assert (res.best, res.n_inliers, res.fitness, res.inlier_rmse) == \
        (plain.best, plain.n_inliers, plain.fitness, plain.inlier_rmse)
    T = _np(res.transformation)
    want = R.kabsch(src.astype(np.float64)[lab > 0], tgt.astype(np.float64)[lab > 0])
    err = np.abs(T - want).max()
    print("max |dT| of the refit vs numpy:", err)
    assert err <= 1e-9
    assert np.abs(T - _np(plain.transformation)).max() > 1e-9  # it is another pose than the winner's
    assert np.array_equal(_bits(_np(res.transformation_f32)), _bits(T.astype(np.float32)))
    assert R.pose_error(T, true)[1] <= R.pose_error(_np(plain.transformation), true)[1]


# --------------------------------------------------------------- 6. degenerate
def test_three_points(gpu_device):
    """N = 3, n = 3: only the permutations of the one sample are valid; which of
    them wins is decided by rounding, so the winner is only required to be one."""
    src, tgt = R.make_case(3, 3, 1.0)[:2]
    ref = _ref("three", src, tgt, ransac_n=3, max_iteration=200, seed=3)
    res = _run(gpu_device, src, tgt, ransac_n=3, max_iteration=200, seed=3, debug=True)
    cnt = _np(res.debug["count"])
    assert np.array_equal(cnt < 0, ref["count"] < 0) and np.all(cnt[cnt < 0] == -1)
    valid = np.flatnonzero(cnt >= 0)
    assert len(valid) == res.n_validated > 0
    assert all(sorted(s) == [0, 1, 2] for s in _np(res.debug["samples"])[valid])
    assert res.best in valid and res.n_inliers == ref["n_inliers"] == cnt[res.best] == 3
    assert np.abs(_np(res.transformation) - ref["transformation"]).max() <= 1e-9


def test_all_hypotheses_rejected(gpu_device):
    src, tgt = R.rejected_case()
    ref = _ref("rejected", src, tgt, ransac_n=3, edge_similarity=0.9, max_iteration=300, seed=2)
    assert ref["best"] == -1 and ref["n_validated"] == 0 and ref["diag"]["checker_margin"] >= 1e-7
    res = _run(gpu_device, src, tgt, ransac_n=3, edge_similarity=0.9, max_iteration=300, seed=2, debug=True)
    assert res.best == -1 and res.n_validated == 0 and res.n_inliers == 0 and res.iterations == 300
    assert res.fitness == 0.0 and res.inlier_rmse == 0.0
    assert np.array_equal(_np(res.transformation), np.eye(4)) and np.array_equal(_np(res.transformation_f32), np.eye(4))
    assert not _np(res.labels).any() and res.correspondence_set.shape == (0, 2)
    assert np.array_equal(_np(res.debug["count"]), ref["count"])


def test_duplicate_source_points_stay_finite(gpu_device):
    """Every source point the same: H has rank 1 (in fact 0 after centring); the
    result is finite, no exactness claim."""
    rng = np.random.RandomState(6)
    src = np.tile(np.array([[0.5, 1.0, 1.5]], np.float32), (32, 1))
    src[16:] = np.array([1.5, 1.0, 0.5], np.float32)  # two distinct points: rank-1 samples too
    tgt = (rng.rand(32, 3) * 2).astype(np.float32)
    for refit in (False, True):
        res = _run(gpu_device, src, tgt, ransac_n=3, max_iteration=500, seed=1, refit=refit, debug=True)
        T = _np(res.transformation)
        assert np.all(np.isfinite(T)) and np.isfinite(res.inlier_rmse) and np.isfinite(res.fitness)
        assert np.all(np.isfinite(_np(res.debug["trans"]))) and np.all(np.isfinite(_np(res.debug["sumsq"])))
        assert res.n_validated > 0 and np.array_equal(T[3], [0, 0, 0, 1])


# ----------------------------------------------------------------- 7. wrappers
def test_wrappers(gpu_device):
    from pointdsc_amd import ransac_solver
    from pointdsc_amd.baselines import RANSAC
    pair, pred_np, rows = R.solver_case()
    src = torch.from_numpy(pair["src_keypts"])[None].to(gpu_device)
    tgt = torch.from_numpy(pair["tgt_keypts"])[None].to(gpu_device)
    corr = torch.from_numpy(pair["corr_pos"])[None].to(gpu_device)
    gt = pair["gt_trans"].astype(np.float64)
    # the baseline: shapes, dtypes, devices as SM's; the pose (a property of the case, on the reference first)
    ref = _ref("baseline", pair["src_keypts"], pair["tgt_keypts"], ransac_n=4, max_iteration=1000, seed=0)
    assert R.tie_free(ref["diag"])
    re_, te = R.pose_error(ref["transformation"], gt)
    assert re_ < 1.0 and te < 0.03
    trans, labels = RANSAC(corr, src, tgt, inlier_threshold=0.10, max_iteration=1000, seed=0)
    assert trans.shape == (1, 4, 4) and trans.dtype == torch.float32 and trans.device == src.device
    assert labels.shape == (1, 1000) and labels.dtype == torch.float32 and labels.device == src.device
    assert np.array_equal(_np(labels[0]), ref["labels"])
    assert np.abs(_np(trans[0]).astype(np.float64) - ref["transformation"]).max() <= 1e-6  # fp32 copy of a 1e-9 pose
    re_, te = R.pose_error(_np(trans[0]).astype(np.float64), gt)
    print("baselines.RANSAC: RE", re_, "TE", te)
    assert re_ < 1.0 and te < 0.03
    # the solver: RANSAC over pred_labels > 0, labels scattered back to N
    pred = torch.from_numpy(pred_np)[None].to(gpu_device)  # some predicted inliers are outliers
    sub = _ref("solver", pair["src_keypts"][rows], pair["tgt_keypts"][rows], ransac_n=3, max_iteration=5000, seed=4)
    assert R.tie_free(sub["diag"])
    strans, slabels = ransac_solver(src, tgt, pred, 0.10, seed=4)
    assert strans.shape == (1, 4, 4) and strans.dtype == torch.float32 and strans.device == src.device
    assert slabels.shape == (1, 1000) and slabels.dtype == torch.float32 and slabels.device == src.device
    want = np.zeros(1000, np.float32)
    want[rows[sub["labels"] > 0]] = 1
    assert np.array_equal(_np(slabels[0]), want)
    assert np.abs(_np(strans[0]).astype(np.float64) - sub["transformation"]).max() <= 1e-6
    # nothing predicted, and fewer than 3
    for k in (0, 2):
        few = torch.zeros_like(pred)
        few[0, :k] = 1
        strans, slabels = ransac_solver(src, tgt, few, 0.10)
        assert torch.equal(strans, torch.eye(4, device=src.device)[None]) and not slabels.any()
        assert slabels.shape == (1, 1000) and strans.dtype == torch.float32


def test_corres_argument_and_errors(gpu_device):
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    N, ratio, n, H, ds, ss = R.WHOLE_CASES["partial_round"]
    src, tgt, _, _ = R.make_case(ds, N, ratio)
    ref = _ref(("whole", "partial_round"), src, tgt, ransac_n=n, max_iteration=H, seed=ss)
    perm = np.random.RandomState(1).permutation(N)
    s = torch.from_numpy(src).to(gpu_device)
    t = torch.from_numpy(np.ascontiguousarray(tgt[perm])).to(gpu_device)  # target row perm[i] <- row i
    inv = np.argsort(perm)
    corres = torch.from_numpy(np.stack([np.arange(N), inv], 1)).to(gpu_device)
    res = ransac(s, t, corres, RADIUS, ransac_n=n, max_iteration=H, seed=ss)
    assert res.best == ref["best"] and np.array_equal(_np(res.labels), ref["labels"])
    assert np.array_equal(_np(res.correspondence_set), _np(corres)[ref["labels"] > 0])
    with pytest.raises(RuntimeError, match="ransac_n"):
        ransac(s, t, corres, RADIUS, ransac_n=5)
    with pytest.raises(RuntimeError, match="confidence"):
        ransac(s, t, corres, RADIUS, confidence=0.0)
    assert ransac(s, t, corres, RADIUS, ransac_n=n, max_iteration=H, seed=ss).best == ref["best"]  # still works
