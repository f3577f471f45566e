"""The preconditions of tests/test_gpu_descriptor_edges.py, on the CPU: every
tie, boundary, count-equals-K, histogram-bin and range placement that a case of
tests/descriptor_cases.py is named after really occurs in it, the FPFH cases'
fragile share stays under its cap, and the normals cases are well posed (or
degenerate in exactly the intended way) -- all from the restatement oracle/
descriptors_oracle.py alone.  A seed or a coordinate that misses its edge fails
here and not, silently, on the GPU."""
import numpy as np
import pytest

import descriptor_cases as DC
from oracle import descriptors_oracle as DO
from test_gpu_descriptors import _normal_check

FRAGILE_CAP = 0.02
LADDER_N = {1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023}
LADDER_K = {1, 2, 3, 64, 65, 127, 128}


@pytest.mark.parametrize("off,r,K", DC.KNN_LATTICE)
def test_lattice_has_radius_and_face_points(off, r, K):
    """Every lattice cloud: neighbours at exactly d^2 == r^2 and points on cell faces."""
    p, r, K = DC.knn_cases()[f"lattice-{off}-r{r}-K{K}"]
    f = DC.knn_facts(p, r, K)
    assert f["on_radius"] >= 800 and f["on_face"] >= 90
    assert np.array_equal(p.astype(np.float64) * 8, np.round(p.astype(np.float64) * 8))  # dyadic: d^2 exact


def test_lattice_cases_cut_and_end_on_shells():
    """K = 5, 19, 20, 100 cut a shell of equal d^2 (the index decides); K = 33 equals the
    interior count of r = 1/4; K = 64 and 128 exceed every count (the total <= K path)."""
    facts = {(off, r, K): DC.knn_facts(*DC.knn_cases()[f"lattice-{off}-r{r}-K{K}"]) for off, r, K in DC.KNN_LATTICE}
    assert facts[("zero", 0.25, 5)]["tie"].sum() >= 100
    assert facts[("mixed", 0.25, 19)]["tie"].sum() >= 50
    assert facts[("neg", 0.375, 20)]["tie"].sum() >= 100
    assert facts[("mixed", 0.375, 100)]["tie"].sum() >= 1
    f = facts[("neg", 0.25, 33)]
    assert (f["total"] == 33).sum() == 8 and f["total"].max() == 33
    assert facts[("big", 0.25, 64)]["total"].max() < 64 and 100 < facts[("big", 0.375, 128)]["total"].max() < 128


@pytest.mark.parametrize("name", sorted(DC._DENSITY))
def test_density_case_hits_its_placement(name):
    p, r, K, q = DC.density_case(name)
    f = DC.knn_facts(p, r, K)
    if name == "count_eq_K":
        assert f["total"][q] == K
    elif name == "count_eq_K_plus_1":
        assert f["total"][q] == K + 1
    else:
        assert f["total"][q] > K  # the threshold walk runs
        r2 = float(np.float32(r)) ** 2
        kth = np.sort(DO._d2(p[q], p))[K - 1]
        assert int(kth / r2 * DC.KNN_BINS) == DC.DENSITY_BINS[name] == f["kth_bin"][q]
    if name == "kth_in_bin_1023":  # ... and a neighbour at d^2 == r^2, whose unclamped bin is 1024
        assert int(np.sort(DO._d2(p[q], p))[K] / float(np.float32(r)) ** 2 * DC.KNN_BINS) == DC.KNN_BINS
    if name == "kth_in_bin_16":
        assert f["tie"][q]


def test_one_cell_case_needs_two_lane_rounds():
    p, r, q = DC.one_cell_case()
    f = DC.knn_facts(p, r, 64)
    assert f["max_cell"] == 100 > 64 and f["total"][q] == 100
    assert len(np.unique(DO.voxel_keys(p, r, 0.0)[DO._d2(p[q], p) <= r * r])) == 1


@pytest.mark.parametrize("copies", [DC.KNN_CAP, DC.KNN_CAP + 1])
def test_coincident_cases(copies):
    """The copies' rows hold exactly `copies` points in d^2 bin 0 and the nearest other point in a
    later bin; with others inside the radius and K = 4, each of them finds K points below
    the copies' bin, so only the copies' own rows can overflow the sort."""
    for inside, K in ((True, 4), (False, 128)):
        p, r = DC.coincident_case(copies, inside)
        D = DO._d2(p[:, None, :], p[None, :, :])
        bins = np.minimum((D / (r * r) * DC.KNN_BINS).astype(np.int64), DC.KNN_BINS - 1)
        is_copy = (D == 0).sum(1) == copies
        assert is_copy.sum() == copies
        assert np.all(((bins == 0) & (D <= r * r)).sum(1)[is_copy] == copies)
        others = ~is_copy
        inr = D <= r * r
        if inside:
            assert (inr[others][:, is_copy].any(1)).sum() == 5  # five see the copies ...
            sees = others & inr[:, is_copy].any(1)
            own_bin0 = ((bins == 0) & inr)[sees].sum(1)
            assert np.all(own_bin0 >= K) and np.all(own_bin0 < 10)  # ... but stop in bin 0
        else:
            assert not inr[others][:, is_copy].any()


def test_knn_ladder_covers_sizes_and_paths():
    ns = {n for n, _, _, _ in DC.KNN_LADDER}
    ks = {k for _, k, _, _ in DC.KNN_LADDER}
    assert ns >= LADDER_N and ks >= LADDER_K
    paths = set()
    for n, K, r, off in DC.KNN_LADDER:
        f = DC.knn_facts(*DC.knn_cases()[f"ladder-n{n}-K{K}"])
        paths |= {"below"} if (f["total"] < K).any() else set()
        paths |= {"equal"} if (f["total"] == K).any() else set()
        paths |= {"walk"} if (f["total"] > K).any() else set()
        paths |= {"single"} if (f["total"] == 1).any() else set()
        paths |= {"big-cell"} if f["max_cell"] > 64 else set()
    assert paths == {"below", "equal", "walk", "single", "big-cell"}


def test_range_cases_sit_on_their_sides_of_2_21():
    for kind, half_cells, last in (("knn_under", 0.0, DC.RANGE - 1), ("knn_over", 0.0, DC.RANGE),
                                   ("voxel_under", 0.5, DC.RANGE - 1), ("voxel_over", 0.5, DC.RANGE)):
        p, cell = DC.range_case(kind)
        assert DC.max_cell_index(p, cell, half_cells * cell) == last
        if last == DC.RANGE:
            with pytest.raises(ValueError, match="2\\^21"):
                DO.voxel_keys(p, cell, half_cells * cell)
        else:
            DO.voxel_keys(p, cell, half_cells * cell)
    # the voxel grid's largest index is half a cell higher: its over case would pass the neighbour grid
    p, cell = DC.range_case("voxel_over")
    assert DC.max_cell_index(p, cell, 0.0) == DC.RANGE - 1


def test_voxel_cases_are_what_they_are_named():
    cases = DC.voxel_cases()
    p, v, _ = cases["faces"]
    x = (p.astype(np.float64) - (p.astype(np.float64).min(0) - 0.5 * v)) / v
    assert np.any(x == np.floor(x), 1).sum() >= 150  # points exactly on voxel faces
    counts = {name: np.unique(DO.voxel_keys(p, v, 0.5 * v), return_counts=True)[1] for name, (p, v, _) in cases.items()}
    assert len(counts["one-voxel"]) == 1
    assert len(counts["own-voxel"]) == 125 and counts["own-voxel"].max() == 1
    assert len(counts["voxels-256"]) == 256 and len(counts["voxels-257"]) == 257
    assert counts["voxels-256"].max() == counts["voxels-257"].max() == 2
    assert counts["big-voxel"].max() == 3000 and len(counts["big-voxel"]) > 10


def test_voxel_ladder_covers_sizes_and_occupancies():
    """Every n of the size ladder; one voxel, every point in its own, several per voxel, and
    points exactly on voxel faces all occur."""
    assert {n for n, _, _ in DC.VOXEL_LADDER} == LADDER_N
    seen = set()
    for n, v, off in DC.VOXEL_LADDER:
        p, v, nrm = DC.voxel_cases()[f"ladder-n{n}-v{v}"]
        assert len(p) == len(nrm) == n
        cnt = np.unique(DO.voxel_keys(p, v, 0.5 * v), return_counts=True)[1]
        x = (p.astype(np.float64) - (p.astype(np.float64).min(0) - 0.5 * v)) / v
        seen |= {"one-voxel"} if len(cnt) == 1 and n > 1 else set()
        seen |= {"own-voxel"} if cnt.max() == 1 and n > 1 else set()
        seen |= {"shared"} if cnt.max() > 1 and len(cnt) > 1 else set()
        seen |= {"faces"} if np.any(x == np.floor(x)) else set()
        seen |= {"past-one-block"} if len(cnt) > 256 else set()
    assert seen == {"one-voxel", "own-voxel", "shared", "faces", "past-one-block"}


def test_zero_sum_voxel_stays_zero_in_the_oracle():
    p, nrm, z = DC.zero_sum_case()
    _, on, _ = DO.voxel_down_sample(p, 0.5, nrm)
    assert np.array_equal(on[z], np.zeros(3, np.float32))
    rest = np.delete(on, z, 0)
    np.testing.assert_allclose(np.linalg.norm(rest, axis=1), 1.0, atol=1e-6)


def test_degenerate_normals_cloud_is_degenerate_as_intended():
    """Counts 1 and 2, a zero covariance, and for the axis-aligned lines FastEigen3x3's p1 == 0
    branch with a zero product column: the oracle's normal is exactly (0, 0, 1) everywhere."""
    p, r, labels = DC.degenerate_normals_cloud()
    nbr, _, cnt = DO.radius_knn(p, r, 30)
    assert np.all(cnt[labels == "isolated"] == 1) and np.all(cnt[labels == "pair"] == 2)
    assert np.all(cnt[labels == "coincident"] == 5)
    C = DO.neighbourhood_covariance(p, nbr, cnt)
    assert not C[labels == "coincident"].any()
    for ax, name in enumerate(("line-x", "line-y", "line-z")):
        m = labels == name
        assert cnt[m].min() == 3 and cnt[m].max() == 5
        Cm = C[m]
        p1 = Cm[:, 0, 1] ** 2 + Cm[:, 0, 2] ** 2 + Cm[:, 1, 2] ** 2
        assert np.all(p1 == 0.0) and np.all(Cm[:, ax, ax] > 0)
        others = [a for a in range(3) if a != ax]
        assert not Cm[:, others, others].any()
        assert not DO.fast_eigen3x3(Cm).any()  # the zero vector EstimateNormals replaces
    n, _ = DO.estimate_normals(p, r, 30)
    assert np.array_equal(n, np.tile(np.array([0, 0, 1], np.float32), (len(p), 1)))


def test_viewpoint_on_a_query_point_does_not_flip_it():
    """The viewpoint is a point of the z line: its own orientation product is exactly 0 (strict
    <: no flip), the points above it flip, the points below do not."""
    p, r, labels = DC.degenerate_normals_cloud()
    vp = np.array([0.0, 0.0, 4.5], np.float32)
    on = np.nonzero(np.all(p == vp, 1))[0]
    assert len(on) == 1 and labels[on[0]] == "line-z"
    n, _ = DO.estimate_normals(p, r, 30, viewpoint=vp)
    assert np.array_equal(n[on[0]], [0, 0, 1])
    m = labels == "line-z"
    assert np.all(n[m & (p[:, 2] > 4.5), 2] == -1) and np.all(n[m & (p[:, 2] < 4.5), 2] == 1)


@pytest.mark.parametrize("n,max_nn,orient", DC.NORMALS_LADDER)
def test_normals_ladder_is_well_posed(n, max_nn, orient):
    """_normal_check's own >= 95% well-posed condition, met by the reference alone."""
    p, _, _, _, _, look = DC.normals_ladder_case(n, max_nn, orient)
    ref, w = DC.normals_ladder_reference(n, max_nn, orient)
    _normal_check(ref, ref, w, p.astype(np.float64), look)


def test_normals_ladder_covers_sizes_and_orientations():
    """NORMALS_SMALL (bitwise, every orientation) and NORMALS_LADDER (well posed) together."""
    assert {n for n, _, _ in DC.NORMALS_LADDER} | {n for n, _, _ in DC.NORMALS_SMALL} >= LADDER_N
    assert {k for _, k, _ in DC.NORMALS_LADDER} | {k for _, k, _ in DC.NORMALS_SMALL} >= LADDER_K
    assert {n for n, _, _ in DC.NORMALS_SMALL} == {1, 2} and {k for _, k, _ in DC.NORMALS_SMALL} >= {1, 2}
    assert {o for _, _, o in DC.NORMALS_LADDER} == {"open3d", "viewpoint", "centroid"}


@pytest.mark.parametrize("n,max_nn,off", DC.NORMALS_SMALL)
def test_normals_small_cases_are_exactly_z(n, max_nn, off):
    """One or two points: under 3 neighbours everywhere, so the oracle's normal is (0, 0, +-1),
    and both signs occur over the orientations.  The orientation products are exact: the
    coordinates are dyadic, and the centroid of at most two of them is too."""
    p, r, K = DC.normals_small_case(n, max_nn, off)
    assert len(p) == n and DO.radius_knn(p, r, K)[2].max() <= min(n, K) < 3
    c = p.astype(np.float64).mean(0)
    assert np.array_equal(c * 128, np.round(c * 128))
    for orient, vp in (("open3d", None), ("viewpoint", DC.VIEWPOINT), ("centroid", None)):
        nv, _ = DO.estimate_normals(p, r, K, viewpoint=vp, orient=orient)
        assert not nv[:, :2].any() and np.all(np.abs(nv[:, 2]) == 1)
        if orient == "open3d":
            assert np.all(nv[:, 2] == 1)
        if orient == "viewpoint" and off == "big":
            assert np.all(nv[:, 2] == -1)  # the viewpoint lies far below the cloud: every normal flips


def test_big_centroid_case_is_well_posed_and_needs_the_second_pass():
    p, r, q, ref, w = DC.big_centroid_case()
    assert len(p) == 70001 > 256 * 256 and len(q) == 500
    c = p.astype(np.float64).mean(0)
    _normal_check(ref, ref, w, p[q].astype(np.float64), c)
    # a centroid from the first 65536 points alone (one pass of 256 x 256 threads, / n) flips normals
    c1 = p[:65536].astype(np.float64).sum(0) / len(p)
    flips = (np.sum(ref * (c1 - p[q]), 1) < 0) != (np.sum(ref * (c - p[q]), 1) < 0)
    assert flips.mean() > 0.05


@pytest.mark.parametrize("name", sorted(DC.FPFH_CASES))
def test_fpfh_case_fragile_share_and_coverage(name):
    R = DC.fpfh_reference(name)
    share = float(R["fragile"].mean())
    print(f"{name}: n={len(R['pts'])} fragile share {share:.4%} (delta {DC.DELTA:g})")
    assert share <= FRAGILE_CAP
    assert np.all(R["bound"][~R["fragile"]] == 0)
    np.testing.assert_allclose(np.linalg.norm(R["normals"], axis=1), 1.0, atol=1e-6)
    cnt, K = R["count"], R["max_nn"]
    assert (cnt == 1).sum() == 3 and not R["f"][cnt == 1].any()  # isolated points: all-zero rows
    live = np.arange(K)[None, :] < cnt[:, None]
    assert ((R["d2"][:, 1:] == 0) & live[:, 1:]).any(1).sum() >= 8  # rows with a coincident neighbour
    if K == 65:
        assert (cnt == 65).mean() > 0.5  # neighbour 64 on the first round's last lane, the second round empty
    elif K > 65:
        assert (cnt > 65).mean() > 0.5  # the second ballot round carries neighbours 65..
    assert cnt.max() == K


def test_fpfh_ladder_covers_sizes_counts_and_block_tails():
    """Every n and max_nn of the size ladder, every n % 4 (four waves per block), clouds of one and
    two points, rows with count 1 only (max_nn = 1), with one pair and with two."""
    assert {n for n, _, _ in DC.FPFH_LADDER} == LADDER_N and {k for _, k, _ in DC.FPFH_LADDER} == LADDER_K
    assert {n % 4 for n, _, _ in DC.FPFH_LADDER} == {0, 1, 2, 3}
    full = set()
    for n, K, r in DC.FPFH_LADDER:
        R = DC.fpfh_ladder_reference(n, K, r)
        cnt = R["count"]
        assert len(R["pts"]) == n and cnt.max() == min(n, K)
        assert float(R["fragile"].mean()) <= FRAGILE_CAP
        np.testing.assert_allclose(np.linalg.norm(R["normals"], axis=1), 1.0, atol=1e-6)
        assert not R["f"][cnt == 1].any() and not R["fn"][cnt == 1].any()
        if K == 1:
            assert np.all(cnt == 1) and not R["f"].any()
        elif n >= K:
            assert R["f"][cnt > 1].any(1).all()  # a row with a pair is not empty
        if n > 5 and K > 3:
            assert (cnt == min(n, K)).mean() > 0.25
            full.add(int(cnt.max()))
    assert full == {63, 64, 65, 128}  # both sides of the first ballot round's 65, and the second round full


def test_fragility_grows_with_delta():
    """The mask is not empty by construction: at a margin far above the transcendental
    functions' error it marks rows, and their bound is positive."""
    R = DC.fpfh_reference("n300-K30")
    for delta, lo in ((1e-6, 0.0), (1e-4, 0.05)):
        fr, bound = DC.fpfh_fragility(R["pts"], R["normals"], R["radius"], R["max_nn"], delta=delta)
        print(f"n300-K30: fragile share {fr.mean():.2%} at delta {delta:g}")
        assert lo <= fr.mean() < 1.0 and np.all(bound[fr] > 0) and bound.max(initial=0) < 100.0


def test_fragile_bound_holds_for_real_bin_flips():
    """The per-row bound of fpfh_fragility against flips that really happen.  The normals are
    moved by 1e-5 (d^2 and with it every weight stay as they are; only binning and the frame
    swap can change), and the mask is taken at delta = 1e-3, a 100-fold margin over that
    move, with exact swap ties counted as well: between different inputs they can fall apart.  Rows do change, every changed row is marked fragile, and no bin moves by more
    than the row's bound."""
    R = DC.fpfh_reference("n700-K65")
    fr, bound = DC.fpfh_fragility(R["pts"], R["normals"], R["radius"], R["max_nn"], delta=1e-3, same_inputs=False)
    moved = (R["normals"].astype(np.float64) + 1e-5 * np.random.RandomState(4).randn(*R["normals"].shape)).astype(np.float32)
    f, _ = DO.compute_fpfh(R["pts"], moved, R["radius"], R["max_nn"])
    diff = np.abs(f - R["f"])
    changed = diff.max(1) > 0
    print(f"n700-K65: {int(changed.sum())} rows changed, {int(fr.sum())} fragile at delta 1e-3, "
          f"worst diff / bound {np.max(diff.max(1)[changed] / bound[changed]):.3f}")
    assert changed.sum() >= 20
    assert not changed[~fr].any()
    assert np.all(diff <= bound[:, None] * (1 + 1e-9) + 1e-9 * np.maximum(np.abs(R["f"]), 1.0))
    assert bound[fr].max() < 50.0  # ... and the bound is no blanket: far under a histogram's 100
