"""The ICP refinement (include/pdsc.h f5, pointdsc_amd/icp.py) on the GPU against
the fp64 restatement tests/icp_reference.py.  Every comparison first asserts, on
the reference's own diagnostics, that the case is free of near-ties (nearest /
second-nearest gaps and radius margins above 1e-9 relative, every per-iteration
|delta fitness| and |delta rmse| below 0.5e-6 or above 2e-6): the GPU differs from
the reference only in the order of its fp64 sums, which then cannot decide a
correspondence or the convergence test the other way.  That condition selected
the seeds (tests/test_icp_reference.py checks it on the CPU); it widens no
tolerance.  Bounds: index outputs, counts and fitness exact; inlier_rmse 1e-12
relative; the pose 1e-9 absolute (summation order over a few thousand fp64 terms
is expected at or below 1e-12; 1e-9 is still 100x under fp32 resolution)."""
import os

import numpy as np
import pytest
import torch

import icp_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RADIUS = 0.1
_REF = {}


def _case(ns, nt, seed):
    return R.make_case(seed, ns, nt)


def _ref(key, src, tgt, init, **kw):
    """The reference of a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = R.registration_icp(src, tgt, RADIUS, init, **kw)
    return _REF[key]


def _run(dev, src, tgt, init, r=RADIUS, **kw):
    from pointdsc_amd.icp import registration_icp
    res = registration_icp(torch.from_numpy(np.ascontiguousarray(src, np.float32)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(tgt, np.float32)).to(dev), r,
                           None if init is None else torch.from_numpy(np.asarray(init, np.float64)).to(dev),
                           want_correspondences=True, **kw)
    return res, res.transformation.cpu().numpy(), res.correspondence.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _same(a, b):
    """Two results bitwise equal."""
    (ra, Ta, ca), (rb, Tb, cb) = a, b
    assert np.array_equal(_bits(Ta), _bits(Tb))
    assert np.array_equal(_bits(ra.transformation_f32.cpu().numpy()), _bits(rb.transformation_f32.cpu().numpy()))
    assert np.array_equal(_bits(np.array([ra.fitness, ra.inlier_rmse])), _bits(np.array([rb.fitness, rb.inlier_rmse])))
    assert (ra.iterations, ra.n_corr) == (rb.iterations, rb.n_corr)
    assert np.array_equal(ca, cb)


def _check_evaluation(res, T, corr, ref):
    assert np.array_equal(corr, ref["correspondence"])
    assert res.n_corr == ref["n_corr"] and res.fitness == ref["fitness"]
    assert abs(res.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 * ref["inlier_rmse"]


def _check_full(res, T, corr, ref):
    assert res.iterations == ref["iterations"] and res.n_corr == ref["n_corr"]
    err = np.abs(T - ref["transformation"]).max()
    print("max |dT| vs fp64 reference:", err)
    assert err <= 1e-9
    _check_evaluation(res, T, corr, ref)
    assert np.array_equal(_bits(res.transformation_f32.cpu().numpy()), _bits(T.astype(np.float32)))


# ------------------------------------------------------------ 1. evaluation only
@pytest.mark.parametrize("nt", [1, 300, 1500])
@pytest.mark.parametrize("ns", [1, 63, 64, 65, 257, 1000])
def test_evaluation_only(ns, nt, gpu_device):
    src, tgt, init, _ = _case(ns, nt, 100)
    ref = _ref(("eval", ns, nt), src, tgt, init, max_iteration=0)
    assert R.tie_free(ref)
    res, T, corr = _run(gpu_device, src, tgt, init, max_iteration=0)
    _check_evaluation(res, T, corr, ref)
    assert res.iterations == 0
    assert np.array_equal(_bits(T), _bits(init))


# ------------------------------------------------------------------ 2. full loop
@pytest.mark.parametrize("ns,nt", [(1000, 1500), (257, 300)])
def test_full_loop(ns, nt, gpu_device):
    src, tgt, init, true = _case(ns, nt, 0)
    ref = _ref(("full", ns, nt), src, tgt, init)
    assert R.tie_free(ref) and ref["iterations"] > 1
    res, T, corr = _run(gpu_device, src, tgt, init)
    _check_full(res, T, corr, ref)
    e0, e1 = R.pose_error(init, true), R.pose_error(T, true)
    assert e1[0] < e0[0] and e1[1] < e0[1]


# ------------------------------------------- 3. queries outside the target's box
def outside_case():
    """Half the source 50 m past the target's box, a quarter 50 m before it
    (negative cells / cells past the end), the rest in place, and queries 0.03 and
    0.09 outside the six faces, straight out from the target point that spans the
    face (so each has that point in range, from cell -1 or from past the last cell)."""
    src, tgt, init, _ = R.make_case(11, 400, 500)
    src = src.copy()
    src[:200] += 50.0
    src[200:300] -= 50.0
    t64 = tgt.astype(np.float64)
    faces = []
    for c in range(3):
        for arg, sign in ((np.argmin, -1.0), (np.argmax, 1.0)):
            for off in (0.03, 0.09):
                q = t64[arg(t64[:, c])].copy()
                q[c] += sign * off
                faces.append(q)
    faces = np.array(faces)
    inv = np.linalg.inv(init)
    src = np.concatenate([src, R.transform(inv, faces).astype(np.float32)])
    return src, tgt, init, len(faces)


def test_queries_outside_the_target_box(gpu_device):
    src, tgt, init, nf = outside_case()
    ref = _ref("outside", src, tgt, init, max_iteration=0)
    assert R.tie_free(ref)
    assert np.all(ref["correspondence"][:300] == -1) and np.all(ref["correspondence"][-nf:] >= 0)
    q = R.transform(init, src[-nf:])
    lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
    assert np.all(((q < lo) | (q > hi)).any(1))  # every face query is outside the box
    res, T, corr = _run(gpu_device, src, tgt, init, max_iteration=0)
    _check_evaluation(res, T, corr, ref)
    ref = _ref("outside-loop", src, tgt, init)
    assert R.tie_free(ref)
    _check_full(*_run(gpu_device, src, tgt, init), ref)


# --------------------------------------------------------- 4. no correspondences
def test_no_correspondences(gpu_device):
    src, tgt, init, _ = _case(257, 300, 0)
    far = init.copy()
    far[:3, 3] += 100.0
    res, T, corr = _run(gpu_device, src, tgt, far)
    assert np.array_equal(_bits(T), _bits(far))
    assert res.fitness == 0.0 and res.inlier_rmse == 0.0 and res.n_corr == 0 and res.iterations == 1
    assert np.all(corr == -1)


# ---------------------------------------------------- 5. coincident target points
def test_coincident_targets(gpu_device):
    src, tgt, init, _ = _case(257, 300, 0)
    ref = _ref(("full", 257, 300), src, tgt, init)
    assert R.tie_free(ref)
    res1, T1, corr1 = _run(gpu_device, src, tgt, init)
    res3, T3, corr3 = _run(gpu_device, src, np.repeat(tgt, 3, 0), init)
    assert np.array_equal(corr3, np.where(corr1 >= 0, 3 * corr1, -1))
    assert np.array_equal(corr3, np.where(ref["correspondence"] >= 0, 3 * ref["correspondence"], -1))
    assert res3.iterations == res1.iterations and res3.n_corr == res1.n_corr
    assert np.abs(T3 - T1).max() <= 1e-9 and np.abs(T3 - ref["transformation"]).max() <= 1e-9


# ------------------------------------------------------------ 6. degenerate sets
@pytest.mark.parametrize("n", [1, 2])
def test_degenerate_correspondence_sets(n, gpu_device):
    """Exactly 1 correspondence (H = 0) and 2, collinear as any 2 points are (rank 1)."""
    tgt = np.array([[0, 0, 0], [1, 0.5, 0.25], [3, 3, 3], [-2, 1, 5]], np.float32)
    src = np.full((6, 3), 40.0, np.float32) + np.arange(6, dtype=np.float32)[:, None]
    src[:n] = tgt[:n] + np.array([[0.03, -0.02, 0.01], [-0.01, 0.04, 0.02]], np.float32)[:n]
    res, T, corr = _run(gpu_device, src, tgt, None)
    assert res.n_corr == n and res.iterations >= 1
    assert np.array_equal(corr, np.array([0, 1][:n] + [-1] * (6 - n)))
    assert np.all(np.isfinite(T)) and np.isfinite(res.inlier_rmse)
    Rm = T[:3, :3]
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-9 and abs(np.linalg.det(Rm) - 1) <= 1e-9
    assert np.array_equal(T[3], [0, 0, 0, 1])
    if n == 1:  # one pair is matched exactly by the first update's translation
        assert res.inlier_rmse <= 1e-12 and np.abs(Rm - np.eye(3)).max() == 0.0


# ------------------------------------------------ 7. path equality, 8. determinism
@pytest.mark.parametrize("ns,nt", [(1000, 1500), (65, 64), (257, 300), (512, 600)])
def test_one_workgroup_and_multi_launch_paths_bitwise_equal(ns, nt, gpu_device, monkeypatch):
    """PDSC_ICP_ONE_WG is read at every call, so it is a per-call knob.  The
    one-workgroup path exists up to 512 source points (one and two chunks here,
    and the largest size); above that both settings take the multi-launch path."""
    src, tgt, init, _ = _case(ns, nt, 0)
    ref = _ref(("full", ns, nt), src, tgt, init)
    assert R.tie_free(ref)
    monkeypatch.setenv("PDSC_ICP_ONE_WG", "0")
    multi = _run(gpu_device, src, tgt, init)
    monkeypatch.setenv("PDSC_ICP_ONE_WG", "1")
    one = _run(gpu_device, src, tgt, init)
    _same(multi, one)
    _check_full(*multi, ref)
    for it in (0, 1):  # evaluation only, and the iteration cap
        monkeypatch.setenv("PDSC_ICP_ONE_WG", "0")
        multi = _run(gpu_device, src, tgt, init, max_iteration=it)
        monkeypatch.setenv("PDSC_ICP_ONE_WG", "1")
        _same(multi, _run(gpu_device, src, tgt, init, max_iteration=it))
        assert multi[0].iterations == it


def test_two_calls_bitwise_equal(gpu_device):
    src, tgt, init, _ = _case(1000, 1500, 0)
    _same(_run(gpu_device, src, tgt, init), _run(gpu_device, src, tgt, init))


# ------------------------------------------------- 9. reference-signature wrapper
def test_icp_refine_wrapper_and_stream(gpu_device):
    from pointdsc_amd import icp_refine, registration_icp
    src, tgt, init, _ = _case(257, 300, 0)
    s = torch.from_numpy(src)[None].to(gpu_device)
    t = torch.from_numpy(tgt)[None].to(gpu_device)
    p = torch.from_numpy(init.astype(np.float32))[None].to(gpu_device)
    out = icp_refine(s, t, p)
    assert out.shape == (1, 4, 4) and out.dtype == torch.float32 and out.device == p.device
    direct = registration_icp(s[0], t[0], 0.1, p[0])
    assert torch.equal(out[0], direct.transformation_f32)
    ref = R.registration_icp(src, tgt, 0.1, init.astype(np.float32))
    assert R.tie_free(ref)
    assert np.abs(direct.transformation.cpu().numpy() - ref["transformation"]).max() <= 1e-9
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        out2 = icp_refine(s, t, p)
    side.synchronize()
    assert torch.equal(out2, out)
    two = icp_refine(torch.cat([s, s]), torch.cat([t, t]), torch.cat([p, p]))  # B > 1: pair by pair
    assert two.shape == (2, 4, 4) and torch.equal(two[0], out[0]) and torch.equal(two[1], out[0])


# ------------------------------------------------------------------ 10. error path
def test_error_paths(gpu_device):
    from pointdsc_amd.icp import registration_icp
    src, tgt, init, _ = _case(65, 64, 0)
    s = torch.from_numpy(src).to(gpu_device)
    wide = torch.tensor([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0]], device=gpu_device)
    with pytest.raises(RuntimeError, match=r"2\^21"):  # the grid range error, reported after the call's sync
        registration_icp(s, wide, 0.1)
    with pytest.raises(RuntimeError, match="max_distance"):
        registration_icp(s, torch.from_numpy(tgt).to(gpu_device), 0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        registration_icp(torch.from_numpy(src), torch.from_numpy(tgt), 0.1)
    res, _, _ = _run(gpu_device, src, tgt, init)  # the library still works after the errors
    assert res.n_corr == _ref(("full", 65, 64), src, tgt, init)["n_corr"]


# ------------------------------------------------------------------ 11. demo cloud
def demo_case(down):
    """down: cloud_bin_0.ply voxel-downsampled at 0.05, fp32 [n,3].  The target is a
    known motion of it (rounded to fp32, shuffled), init the motion perturbed by 1
    degree and 2 cm."""
    rng = np.random.RandomState(21)
    true = R.rigid([0.2, 1.0, -0.4], 30.0, [0.4, -0.3, 0.2])
    tgt = R.transform(true, down).astype(np.float32)[rng.permutation(len(down))]
    init = R.rigid([1.0, 0.3, 0.5], 1.0, [0.012, -0.012, 0.011]) @ true
    return tgt, init, true


def test_demo_cloud(gpu_device, monkeypatch):
    from pointdsc_amd.descriptors import read_ply, voxel_down_sample
    raw = torch.from_numpy(read_ply(os.path.join(GOLDEN, "demo_data", "cloud_bin_0.ply"))).to(gpu_device)
    down = voxel_down_sample(raw, 0.05)[0].cpu().numpy()
    tgt, init, true = demo_case(down)
    ref = _ref("demo", down, tgt, init, max_iteration=3)
    assert R.tie_free(ref)
    runs = []
    for knob in ("0", "1"):  # this cloud is above the one-workgroup path's 512 points: both settings must agree
        monkeypatch.setenv("PDSC_ICP_ONE_WG", knob)
        runs.append(_run(gpu_device, down, tgt, init, max_iteration=3))
        _check_full(*runs[-1], ref)
    if len(runs) == 2:
        _same(*runs)
    assert R.pose_error(runs[0][1], true)[1] < R.pose_error(init, true)[1]
