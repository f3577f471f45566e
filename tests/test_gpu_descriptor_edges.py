"""The descriptor stage (pointdsc_amd/csrc/descriptors.hip: voxel grid, radius
kNN, normals, SPFH / FPFH) held to its CPU restatement at edge shapes: the
clouds of tests/descriptor_cases.py -- exact d^2 ties at the K-th place,
neighbours at exactly d^2 == r^2, points on cell and voxel faces, counts at K
and K + 1, every placement of the threshold walk, coincident points up to and
past the LDS sort's capacity, n from 1 across the launch boundaries, the 2^21
cell range from both sides.  tests/test_descriptor_cases.py asserts on the CPU
that each case contains what it is named after.

Index outputs, d^2, voxel means and the degenerate normals are compared
bitwise; FPFH bitwise on every row the reference does not mark fragile
(descriptor_cases.fpfh_fragility), and within the size of its possible bin
flips on the others."""
import numpy as np
import pytest
import torch

import descriptor_cases as DC
from oracle import descriptors_oracle as DO
from test_gpu_descriptors import _normal_check

pytestmark = pytest.mark.gpu

RANGE_ERROR = r"extent / cell size >= 2\^21"
CAP_ERROR = r"> 1024 points within one d\^2 bin"


def _knn(p, r, K, dev):
    from pointdsc_amd import descriptors as D
    nbr, d2, cnt = D.radius_knn(torch.from_numpy(p).to(dev), r, K)
    return nbr.cpu().numpy(), d2.cpu().numpy(), cnt.cpu().numpy()


def _assert_knn_equal(ours, ref, K):
    nbr, d2, cnt = ours
    rn, rd, rc = ref
    assert np.array_equal(cnt, rc)
    assert np.array_equal(nbr, rn)
    assert np.array_equal(d2.view(np.int64), rd.view(np.int64))  # bit-equal, -0.0 included
    pad = np.arange(K)[None, :] >= cnt[:, None]
    assert np.all(nbr[pad] == -1) and np.all(d2[pad] == 0.0)
    assert np.array_equal(nbr[:, 0], np.arange(len(nbr))) and np.all(d2[:, 0] == 0.0)  # the query first


@pytest.mark.parametrize("name", sorted(DC.knn_cases()))
def test_radius_knn_bit_exact(name, gpu_device):
    p, r, K = DC.knn_cases()[name]
    _assert_knn_equal(_knn(p, r, K, gpu_device), DC.knn_reference(name), K)


@pytest.mark.parametrize("inside,K", [(True, 4), (False, 128)])
def test_radius_knn_coincident_at_capacity(inside, K, gpu_device):
    """1024 copies of one point: the most one d^2 bin may hold; exact, ties by index."""
    p, r = DC.coincident_case(DC.KNN_CAP, inside)
    _assert_knn_equal(_knn(p, r, K, gpu_device), DO.radius_knn(p, r, K), K)


@pytest.mark.parametrize("inside,K", [(True, 4), (False, 128)])
def test_radius_knn_coincident_past_capacity_is_refused(inside, K, gpu_device):
    p, r = DC.coincident_case(DC.KNN_CAP + 1, inside)
    with pytest.raises(RuntimeError, match=CAP_ERROR):
        _knn(p, r, K, gpu_device)


def test_radius_knn_range_error(gpu_device):
    p, cell = DC.range_case("knn_over")
    with pytest.raises(RuntimeError, match=RANGE_ERROR):
        _knn(p, cell, 4, gpu_device)
    # the voxel grid's over case is inside the neighbour grid's range (half a cell lower)
    p, cell = DC.range_case("voxel_over")
    _assert_knn_equal(_knn(p, cell, 4, gpu_device), DO.radius_knn(p, cell, 4), 4)


def test_radius_knn_is_deterministic(gpu_device):
    """Two calls are bit-identical (the LDS slots are claimed by atomics in any order; the
    sort's (d^2, index) key is total)."""
    for name in ("lattice-neg-r0.375-K20", "ladder-n1023-K128", "one-cell-K64"):
        p, r, K = DC.knn_cases()[name]
        a, b = _knn(p, r, K, gpu_device), _knn(p, r, K, gpu_device)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def _voxel(p, v, nrm, dev):
    from pointdsc_amd import descriptors as D
    op, on = D.voxel_down_sample(torch.from_numpy(p).to(dev), v, None if nrm is None else torch.from_numpy(nrm).to(dev))
    return op.cpu().numpy(), None if on is None else on.cpu().numpy()


@pytest.mark.parametrize("name", sorted(DC.voxel_cases()))
def test_voxel_down_sample_bit_exact(name, gpu_device):
    p, v, nrm = DC.voxel_cases()[name]
    ours, on = _voxel(p, v, nrm, gpu_device)
    ref, rn, _ = DO.voxel_down_sample(p, v, nrm)
    assert ours.shape == ref.shape  # the voxel count
    assert ours.tobytes() == ref.tobytes()
    np.testing.assert_allclose(on, rn, rtol=0, atol=2e-7)
    assert _voxel(p, v, None, gpu_device)[0].tobytes() == ref.tobytes()  # ... and without normals


def test_voxel_zero_normal_sum_stays_zero(gpu_device):
    p, nrm, z = DC.zero_sum_case()
    _, on = _voxel(p, 0.5, nrm, gpu_device)
    assert on[z].tobytes() == np.zeros(3, np.float32).tobytes()


def test_voxel_range(gpu_device):
    p, cell = DC.range_case("voxel_under")
    ours, _ = _voxel(p, cell, None, gpu_device)
    assert ours.tobytes() == DO.voxel_down_sample(p, cell)[0].tobytes()
    p, cell = DC.range_case("voxel_over")
    with pytest.raises(RuntimeError, match=RANGE_ERROR):
        _voxel(p, cell, None, gpu_device)


def _normals(p, r, K, dev, **kw):
    from pointdsc_amd import descriptors as D
    return D.estimate_normals(torch.from_numpy(p).to(dev), r, K, **kw).cpu().numpy()


@pytest.mark.parametrize("orient", ["open3d", "viewpoint", "centroid"])
def test_normals_degenerate_cases_bitwise(orient, gpu_device):
    """1 and 2 neighbours, a zero covariance, axis-aligned lines (FastEigen3x3's p1 == 0
    branch, a zero product column): (0, 0, 1) exactly, flipped only where the orientation
    product is < 0 -- with the viewpoint on a query point it is exactly 0 there: no flip."""
    p, r, _ = DC.degenerate_normals_cloud()
    vp = np.array([0.0, 0.0, 4.5], np.float32) if orient == "viewpoint" else None
    ours = _normals(p, r, 30, gpu_device, viewpoint=vp, orient=orient)
    ref, _ = DO.estimate_normals(p, r, 30, viewpoint=vp, orient=orient)
    assert ours.tobytes() == ref.tobytes()
    if orient == "open3d":
        assert np.array_equal(ours, np.tile(np.array([0, 0, 1], np.float32), (len(p), 1)))


@pytest.mark.parametrize("max_nn", [1, 2])
def test_normals_under_three_neighbours_bitwise(max_nn, gpu_device):
    """max_nn 1 and 2 leave every point under 3 neighbours on a cloud that has them."""
    p, r, _, _, _, _ = DC.normals_ladder_case(65, 3, "centroid")
    for orient, vp in (("open3d", None), ("viewpoint", DC.VIEWPOINT), ("centroid", None)):
        ours = _normals(p, r, max_nn, gpu_device, viewpoint=vp, orient=orient)
        ref, _ = DO.estimate_normals(p, r, max_nn, viewpoint=vp, orient=orient)
        assert np.all(np.abs(ref[:, 2]) == 1) and ours.tobytes() == ref.tobytes()


@pytest.mark.parametrize("n,max_nn,off", DC.NORMALS_SMALL)
def test_normals_one_and_two_points_bitwise(n, max_nn, off, gpu_device):
    """The bottom of the size ladder: a cloud of one or two points has under 3 neighbours
    everywhere, so the normal is (0, 0, 1), flipped by an orientation product that is exact."""
    p, r, K = DC.normals_small_case(n, max_nn, off)
    for orient, vp in (("open3d", None), ("viewpoint", DC.VIEWPOINT), ("centroid", None)):
        ours = _normals(p, r, K, gpu_device, viewpoint=vp, orient=orient)
        ref, _ = DO.estimate_normals(p, r, K, viewpoint=vp, orient=orient)
        assert ours.shape == (n, 3) and np.all(np.abs(ref[:, 2]) == 1) and ours.tobytes() == ref.tobytes()


@pytest.mark.parametrize("n,max_nn,orient", DC.NORMALS_LADDER)
def test_normals_size_ladder(n, max_nn, orient, gpu_device):
    p, r, K, orient, vp, look = DC.normals_ladder_case(n, max_nn, orient)
    ours = _normals(p, r, K, gpu_device, viewpoint=vp, orient=orient)
    ref, w = DC.normals_ladder_reference(n, max_nn, orient)
    np.testing.assert_allclose(np.linalg.norm(ours, axis=1), 1.0, atol=1e-6)
    _normal_check(ours, ref, w, p.astype(np.float64), look)


def test_normals_centroid_past_one_stats_pass(gpu_device):
    """n = 70001: the cloud statistics' 256 x 256 threads take a second grid-stride pass; the
    centroid they sum orients the normals (a first-pass-only centroid flips > 5% of them)."""
    p, r, q, ref, w = DC.big_centroid_case()
    ours = _normals(p, r, 30, gpu_device, orient="centroid")
    _normal_check(ours[q], ref, w, p[q].astype(np.float64), p.astype(np.float64).mean(0))


def _ulp_distance(a, b):
    """Largest distance in units in the last place between two fp64 arrays of one sign pattern."""
    ia, ib = a.view(np.int64), b.view(np.int64)
    return int(np.abs(ia - ib).max(initial=0))


def _check_fpfh(name, R, gpu_device):
    """Normals from the oracle.  Off the fragile rows both sides run the same IEEE fp64
    operations in the same order (no fma contraction; divide and sqrt correctly rounded;
    d^2 bit-equal), and the transcendental functions only pick bins: bit-identical.  A
    fragile row may differ by its possible bin flips, descriptor_cases.fpfh_fragility."""
    from pointdsc_amd import descriptors as D
    tp, tn = torch.from_numpy(R["pts"]).to(gpu_device), torch.from_numpy(R["normals"]).to(gpu_device)
    f, fn = D.compute_fpfh(tp, tn, R["radius"], R["max_nn"])
    f, fn = f.cpu().numpy(), fn.cpu().numpy()
    rf, rfn, solid = R["f"], R["fn"], ~R["fragile"]
    assert np.all(f >= 0) and np.all(rf >= 0)
    print(f"{name}: worst ulp distance on non-fragile rows {_ulp_distance(f[solid], rf[solid])}, "
          f"fragile rows {int(R['fragile'].sum())}, worst |diff| there "
          f"{np.abs(f - rf)[R['fragile']].max(initial=0):.3g}")
    assert f[solid].tobytes() == rf[solid].tobytes()
    slack = R["bound"][:, None] * (1 + 1e-9) + 1e-9 * np.maximum(np.abs(rf), 1.0)
    assert np.all(np.abs(f - rf) <= slack)
    np.testing.assert_allclose(fn[solid], rfn[solid], rtol=0, atol=1e-6)
    assert not f[R["count"] == 1].any() and not fn[R["count"] == 1].any()  # isolated points
    f2, fn2 = D.compute_fpfh(tp, tn, R["radius"], R["max_nn"])
    assert f2.cpu().numpy().tobytes() == f.tobytes() and fn2.cpu().numpy().tobytes() == fn.tobytes()
    assert f.shape == rf.shape and fn.shape == rfn.shape


@pytest.mark.parametrize("name", sorted(DC.FPFH_CASES))
def test_fpfh_bitwise_off_fragile_rows(name, gpu_device):
    _check_fpfh(name, DC.fpfh_reference(name), gpu_device)


@pytest.mark.parametrize("n,max_nn,radius", DC.FPFH_LADDER)
def test_fpfh_size_ladder(n, max_nn, radius, gpu_device):
    """n from 1 across the four-waves-per-block tail, max_nn from 1 (count == 1 on every row:
    all zeros) over 2 and 3 (one and two pairs) to both ballot rounds."""
    _check_fpfh(f"n{n}-K{max_nn}", DC.fpfh_ladder_reference(n, max_nn, radius), gpu_device)
