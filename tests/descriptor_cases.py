"""Small deterministic clouds that put the descriptor stage (pointdsc_amd/csrc/
descriptors.hip) on its edges, and -- from the CPU restatement oracle/
descriptors_oracle.py alone -- the facts the GPU tests rely on: that a tie, a
point on a boundary, a count equal to K or a histogram-bin placement really
occurs in a case (tests/test_descriptor_cases.py asserts every one of them on
the CPU, so tests/test_gpu_descriptor_edges.py cannot pass vacuously).

Coordinates are dyadic (small integers times a power of two, translated by
dyadic offsets) wherever a test needs exact ties: every difference, square and
sum of the fp64 d^2 is then exact, so "two neighbours at the same distance"
and "a neighbour at exactly d^2 == r^2" are statements about the input, not
about rounding.
"""
import functools

import numpy as np

from oracle import descriptors_oracle as DO

KNN_BINS = 1024  # descriptors.hip: the d^2 / r^2 histogram of the threshold search
KNN_CAP = 1024   # ... and the survivors it can sort per query
RANGE = 1 << DO.KEY_BITS
DELTA = 1e-12    # fragile-row margin of the FPFH cases (fpfh_fragility)

OFFSETS = {"zero": (0.0, 0.0, 0.0), "neg": (-37.0, -37.5, -36.875), "big": (900.0, 899.5, 901.125),
           "mixed": (-37.0, 900.0, 0.125)}


def _f32(p):
    """fp32 copy of fp64 coordinates that must survive the conversion unchanged."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    out = p.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), p), "coordinates are not fp32-representable"
    return out


def _shuffled(p, seed):
    """Rows in a seeded random order: the index tie-break must not follow the scan order."""
    return p[np.random.RandomState(seed).permutation(len(p))]


def lattice(m, k, offset, seed=0):
    """m^3 points at spacing 2^-k, translated by `offset`, in shuffled order."""
    g = np.arange(m, dtype=np.float64) * 2.0 ** -k
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(offset, np.float64)
    return _shuffled(_f32(p), seed)


# ------------------------------------------------------------------ radius kNN
_FILL = [(1, 0, 0), (0, 2, 0), (0, 0, 3), (4, 0, 0), (0, 5, 0), (3, 3, 3)]  # / 64: d^2 bins 0, 1, 2, 4, 6, 6
_OUT = [(65, 0, 0), (100, 100, 0), (-70, 0, 0), (0, -64, -1), (200, 3, 7)]   # / 64: outside r = 1
# name -> (K, in-radius neighbours of the query in units of 1/64 (r = 1), offset).  With the query the first
# K - 1 entries make K points; sum of squares / 4 is the K-th neighbour's d^2 / r^2 * 1024.
_DENSITY = {
    "count_eq_K": (8, _FILL + [(8, 0, 0)], "neg"),
    "count_eq_K_plus_1": (8, _FILL + [(8, 0, 0), (0, 8, 0)], "zero"),
    "kth_in_bin_0": (8, [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (1, 1, 1),
                         (8, 0, 0), (20, 5, 0), (64, 0, 0)], "big"),
    "kth_in_bin_15": (8, _FILL + [(6, 5, 0), (8, 0, 0), (0, 8, 0), (30, 0, 0)], "mixed"),
    "kth_in_bin_16": (8, _FILL[:5] + [(6, 5, 0), (8, 0, 0), (0, 8, 0), (30, 0, 0)], "neg"),
    "kth_in_bin_1023": (8, _FILL + [(63, 11, 2), (64, 0, 0), (0, 64, 0)], "zero"),
}
DENSITY_BINS = {"kth_in_bin_0": 0, "kth_in_bin_15": 15, "kth_in_bin_16": 16, "kth_in_bin_1023": 1023}


def density_case(name):
    """(points, radius 1, K, index of the query).  One query whose in-radius set is listed in _DENSITY."""
    K, inside, off = _DENSITY[name]
    p = np.array([(0, 0, 0)] + inside + _OUT, np.float64) / 64.0 + np.asarray(OFFSETS[off])
    p = _shuffled(_f32(p), 11)
    q = int(np.nonzero(np.all(p == _f32(OFFSETS[off])[0], 1))[0][0])
    return p, 1.0, K, q


def one_cell_case():
    """100 points of one grid cell (5 x 5 x 4 at spacing 1/8, r = 1, the cloud's minimum at the
    query) plus points outside the radius: a cell scanned in two 64-lane rounds."""
    g = [(i, j, l) for i in range(5) for j in range(5) for l in range(4)]
    p = np.array(g + [(9, 0, 0), (0, 17, 0), (30, 30, 30)], np.float64) / 8.0
    p = _shuffled(_f32(p), 5)
    return p, 1.0, int(np.nonzero(np.all(p == 0, 1))[0][0])


def coincident_case(copies, others_inside):
    """`copies` copies of one point c (r = 1) plus a few others.  others_inside: a
    tight group of five at 7/8 r from c -- its members find each other in d^2 bin 0,
    so with K <= 5 their threshold bin stays below the copies' bin; otherwise two
    isolated points at 1.5 r.  The copies' own rows keep exactly the `copies` points
    of bin 0: KNN_CAP of them is the most the LDS sort holds."""
    c = np.array([0.5, 0.25, -0.125]) + np.asarray(OFFSETS["neg"])
    if others_inside:
        o = c + np.array([(56, 0, 0), (57, 0, 0), (56, 1, 0), (56, 0, 1), (57, 1, 0)], np.float64) / 64.0
    else:
        o = c + np.array([(96, 0, 0), (0, -96, 0)], np.float64) / 64.0
    far = c + np.array([(640, 0, 0), (0, 0, 300)], np.float64) / 64.0
    return _shuffled(_f32(np.concatenate([np.repeat(c[None], copies, 0), o, far])), 3), 1.0


def dyadic_cloud(n, seed, offset="zero"):
    """n random points of the 1/64 lattice in the unit cube (exact d^2, natural ties)."""
    rng = np.random.RandomState(seed)
    return _f32(rng.randint(0, 64, (n, 3)) / 64.0 + np.asarray(OFFSETS[offset]))


# (n, max_nn, radius, offset): a covering subset of n x max_nn of the size ladder.  r = 2 puts
# the whole unit cube in every radius and in one cell, so count == n there.
KNN_LADDER = [
    (1, 1, 0.25, "zero"), (1, 128, 0.25, "big"), (2, 2, 2.0, "neg"), (3, 3, 2.0, "zero"), (4, 64, 2.0, "big"),
    (5, 128, 2.0, "neg"), (5, 1, 2.0, "mixed"), (63, 65, 0.5, "zero"), (64, 127, 0.5, "neg"), (64, 128, 2.0, "big"),
    (65, 1, 0.25, "zero"), (65, 64, 2.0, "mixed"), (65, 65, 2.0, "neg"), (129, 128, 2.0, "zero"),
    (255, 2, 0.25, "big"), (256, 3, 0.25, "neg"), (257, 64, 0.5, "mixed"), (1023, 65, 0.25, "zero"),
    (1023, 128, 0.5, "neg"),
]

# lattice(6, 3, .): spacing 1/8.  r = 1/4 (two steps): shells of 1, 6, 12, 8, 6 points at
# d^2 = 0, 1, 2, 3, 4 steps^2, the last at exactly r^2.  r = 3/8: up to 123 points within (120 in a 6^3 block), (3,0,0) and
# (2,2,1) at exactly r^2.  K cuts a shell (ties at the K-th place) or ends on one.
KNN_LATTICE = [
    ("zero", 0.25, 5), ("neg", 0.25, 33), ("big", 0.25, 64), ("mixed", 0.25, 19), ("neg", 0.375, 20),
    ("big", 0.375, 128), ("mixed", 0.375, 100),
]


@functools.lru_cache(maxsize=None)
def knn_cases():
    """name -> (points, radius, max_nn) of every radius-kNN case the GPU is held to bit-exactly."""
    out = {}
    for off, r, K in KNN_LATTICE:
        out[f"lattice-{off}-r{r}-K{K}"] = (lattice(6, 3, OFFSETS[off]), r, K)
    for name in _DENSITY:
        p, r, K, _ = density_case(name)
        out[f"density-{name}"] = (p, r, K)
    p, r, _ = one_cell_case()
    for K in (3, 64, 128):
        out[f"one-cell-K{K}"] = (p, r, K)
    for n, K, r, off in KNN_LADDER:
        out[f"ladder-n{n}-K{K}"] = (dyadic_cloud(n, 100 + n + K, off), r, K)
    p, r = range_case("knn_under")
    out["range-under"] = (p, r, 4)
    return out


@functools.lru_cache(maxsize=None)
def knn_reference(name):
    """The oracle's (nbr, dist2, count) of knn_cases()[name], computed once."""
    p, r, K = knn_cases()[name]
    return DO.radius_knn(p, r, K)


def knn_facts(pts, radius, K):
    """What a radius-kNN case exercises, from fp64 brute force: per query the in-radius
    count `total`, whether the K-th and (K+1)-th nearest are at the same d^2 (`tie`: the
    index decides who is kept), the K-th neighbour's histogram bin (int)(d2 / r2 * 1024)
    clamped like the kernel's (`kth_bin`, -1 where total < K); the number of (query,
    neighbour) pairs at exactly d^2 == r^2 (`on_radius`); the number of points on a
    grid-cell face other than the cloud's minimum (`on_face`); the largest cell population
    (`max_cell`)."""
    r = float(np.float32(radius))
    r2 = r * r
    n = len(pts)
    D = DO._d2(pts[:, None, :], pts[None, :, :])
    inr = D <= r2
    total = inr.sum(1)
    Ds = np.sort(np.where(inr, D, np.inf), 1)
    Ds = np.concatenate([Ds, np.full((n, max(0, K + 1 - n)), np.inf)], 1)
    kth = Ds[:, K - 1]
    with np.errstate(invalid="ignore"):
        kb = np.where(total >= K, np.minimum((np.where(total >= K, kth, 0.0) / r2 * KNN_BINS).astype(np.int64),
                                            KNN_BINS - 1), -1)
    x = (pts.astype(np.float64) - pts.astype(np.float64).min(0)) / r
    keys = DO.voxel_keys(pts, r, 0.0)
    return dict(total=total, tie=(total > K) & (Ds[:, K - 1] == Ds[:, K]), kth_bin=kb,
                on_radius=int((D == r2).sum()), on_face=int(np.any((x == np.floor(x)) & (x > 0), 1).sum()),
                max_cell=int(np.unique(keys, return_counts=True)[1].max()))


# ------------------------------------------------------------------ grid range
def range_case(kind):
    """(points, cell): two clusters 2^13 apart with cell = 2^-8, so extent / cell sits at
    2^21.  knn_*: the neighbour grid (half = 0), the far cluster's largest x at 2^13 - 2^-8
    (index 2^21 - 1, the last one) or at 2^13 (index 2^21).  voxel_*: the voxel grid (half =
    cell / 2), largest z at 2^13 - 2^-8 (index floor(2^21 - 1/2) = 2^21 - 1) or at 2^13 -
    2^-9 (index 2^21 -- half a cell earlier than the neighbour grid would refuse)."""
    cell, top = 2.0 ** -8, 2.0 ** 13
    axis = 0 if kind.startswith("knn") else 2
    hi = {"knn_under": top - cell, "knn_over": top, "voxel_under": top - cell, "voxel_over": top - cell / 2}[kind]
    a = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 2), (3, 3, 3), (0, 2, 0)], np.float64) * cell / 2
    b = np.array([(0, 0, 0), (-1, 0, 0), (-3, 1, 2), (-2, 2, 0), (-8, 0, 0)], np.float64) * cell / 2
    b = np.roll(b, axis, 1)
    b[:, axis] += hi
    return _shuffled(_f32(np.concatenate([a, b])), 2), cell


def max_cell_index(pts, cell, half):
    """The largest floor((p - (min - half)) / cell) over the cloud, in fp64 like the kernels."""
    p = pts.astype(np.float64)
    return int(np.floor((p - (p.min(0) - half)) / cell).max())


# ------------------------------------------------------------------ voxel grid
def _unit_normals(n, seed):
    v = np.random.RandomState(seed).randn(n, 3)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def voxel_cases():
    """name -> (points, voxel size, normals)."""
    out = {}
    p = lattice(6, 3, OFFSETS["mixed"], seed=4)  # v = 1/4, origin = min - 1/8: odd lattice steps lie on faces
    out["faces"] = (p, 0.25, _unit_normals(len(p), 1))
    rng = np.random.RandomState(6)
    p = _f32(rng.randint(0, 100, (50, 3)) / 1024.0 + np.asarray(OFFSETS["neg"]))  # extent < v / 2
    out["one-voxel"] = (p, 0.25, _unit_normals(50, 2))
    p = lattice(5, 0, OFFSETS["big"], seed=7)  # spacing 1, v = 1/2
    out["own-voxel"] = (p, 0.5, _unit_normals(len(p), 3))
    for m in (256, 257):  # m occupied voxels along x, three of them with two points
        x = np.concatenate([np.arange(m, dtype=np.float64), [10.125, 100.125, m - 1 + 0.125]])
        p = _shuffled(_f32(np.stack([x - 37.0, np.full_like(x, 0.5), np.full_like(x, 900.0)], 1)), 8)
        out[f"voxels-{m}"] = (p, 0.5, _unit_normals(len(p), m))
    p, nrm, _ = zero_sum_case()
    out["zero-sum"] = (p, 0.5, nrm)
    big = rng.randint(0, 500, (3000, 3)) / 4096.0  # extent < v / 2: one voxel of v = 1/4 (origin = min - v / 2)
    oth = rng.randint(0, 64, (20, 3)) / 8.0 + 1.0
    p = _shuffled(_f32(np.concatenate([big, oth]) + np.asarray(OFFSETS["neg"])), 9)
    out["big-voxel"] = (p, 0.25, _unit_normals(len(p), 5))
    for n, v, off in VOXEL_LADDER:
        out[f"ladder-n{n}-v{v}"] = voxel_ladder_case(n, v, off)
    return out


# (n, voxel size, offset): the size ladder through the voxel grid, on the 1/64 lattice of the unit
# cube (dyadic v: points on voxel faces, exact means).  v = 2 holds the cloud in one voxel, v =
# 1/64 gives nearly every point its own.
VOXEL_LADDER = [
    (1, 0.25, "zero"), (2, 2.0, "neg"), (2, 0.015625, "big"), (3, 0.25, "mixed"), (4, 0.5, "big"), (5, 0.015625, "neg"),
    (63, 0.25, "zero"), (64, 0.015625, "mixed"), (65, 0.5, "neg"), (255, 0.125, "big"), (256, 0.015625, "zero"),
    (257, 0.25, "neg"), (1023, 0.015625, "big"), (1023, 0.25, "mixed"),
]


def voxel_ladder_case(n, v, off):
    """(points, voxel size, normals) of a VOXEL_LADDER entry."""
    return dyadic_cloud(n, 300 + n + int(64 * v), off), v, _unit_normals(n, 400 + n)


def zero_sum_case():
    """(points, normals, index of the voxel whose normals are n and -n): spacing-1 points with
    v = 1/2, one voxel holding two points with opposite normals -- open3d's
    normalized() leaves the zero sum 0."""
    p = np.array([(0, 0, 0), (1, 0, 0), (1.125, 0, 0), (2, 1, 0), (0, 3, 1), (2, 1, 0.125)], np.float64)
    nrm = _unit_normals(len(p), 12)
    nrm[2] = -nrm[1]
    pts = _f32(p + np.asarray(OFFSETS["neg"]))
    keys = DO.voxel_keys(pts, 0.5, 0.25)
    return pts, nrm, int(np.nonzero(np.unique(keys) == keys[1])[0][0])


# --------------------------------------------------------------------- normals
def degenerate_normals_cloud():
    """(points, radius 1/4, labels): an isolated point (1 neighbour), a pair (2), five
    coincident points (zero covariance) and lines of seven points at spacing 1/8 along x, y
    and z with the other two coordinates 0 (a diagonal covariance with two zero entries:
    FastEigen3x3 takes its p1 == 0 branch, l1 = l2 = 0, and the product column is 0).  Small
    integers / 8 throughout, so every cumulant and every division by the count is exact."""
    t = 4.0 + np.arange(7) / 8.0
    z = np.zeros(7)
    parts = [("isolated", [(8, 8, 8)]), ("pair", [(-8, -8, -8), (-8, -8, -7.875)]),
             ("coincident", [(-4, 2, 1)] * 5), ("line-x", np.stack([t, z, z], 1)), ("line-y", np.stack([z, t, z], 1)),
             ("line-z", np.stack([z, z, t], 1))]
    pts = _f32(np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for _, p in parts]))
    labels = np.concatenate([[name] * len(p) for name, p in parts])
    perm = np.random.RandomState(13).permutation(len(pts))
    return pts[perm], 0.25, labels[perm]


def surface(n, seed, offset=(0.0, 0.0, 0.0), jitter=2e-3):
    """n points of a jittered smooth surface over the unit square (fp32, general position)."""
    rng = np.random.RandomState(seed)
    u, v = rng.rand(2, n)
    z = 0.2 * np.sin(3 * u) * np.cos(2 * v) + jitter * rng.randn(n)
    return (np.stack([u, v, z], 1) + np.asarray(offset, np.float64)).astype(np.float32)


def ladder_radius(n):
    """About 24 neighbours on the unit-square surface; the whole cloud for a handful of points."""
    return float(min(2.0, np.sqrt(24.0 / (np.pi * n))))


# (n, max_nn, orient): every max_nn >= 3 of the ladder and all three orientations
NORMALS_LADDER = [
    (3, 3, "open3d"), (4, 64, "viewpoint"), (5, 128, "centroid"), (63, 65, "open3d"), (64, 3, "centroid"),
    (65, 127, "viewpoint"), (255, 128, "centroid"), (256, 64, "open3d"), (257, 65, "viewpoint"),
    (1023, 127, "centroid"),
]
VIEWPOINT = np.array([0.3, 0.6, 1.5], np.float32)
# (n, max_nn, offset): the bottom of the ladder, where every point has under 3 neighbours and the
# normal is (0, 0, 1) up to the orientation's sign -- dyadic clouds with r = 2, so the centroid
# and both orientation products are exact and the comparison is bitwise
NORMALS_SMALL = [(1, 1, "zero"), (1, 128, "big"), (2, 1, "mixed"), (2, 2, "neg"), (2, 64, "big")]


def normals_small_case(n, max_nn, off):
    """(points, radius 2, max_nn) of a NORMALS_SMALL entry."""
    return dyadic_cloud(n, 500 + n + max_nn, off), 2.0, max_nn


def normals_ladder_case(n, max_nn, orient):
    """(points, radius, max_nn, orient, viewpoint fp32 | None, the point the sign looks at in fp64)."""
    p = surface(n, 200 + n)
    vp = VIEWPOINT if orient == "viewpoint" else None
    look = {"open3d": None, "viewpoint": VIEWPOINT.astype(np.float64),
            "centroid": p.astype(np.float64).mean(0)}[orient]
    return p, ladder_radius(n), max_nn, orient, vp, look


@functools.lru_cache(maxsize=None)
def normals_ladder_reference(n, max_nn, orient):
    p, r, K, orient, vp, _ = normals_ladder_case(n, max_nn, orient)
    return DO.estimate_normals(p, r, K, viewpoint=vp, orient=orient)


BIG_N, BIG_RADIUS, BIG_QUERIES = 70001, 0.012, 500


@functools.lru_cache(maxsize=None)
def big_centroid_case():
    """n = 70001 > 65536 (the cloud statistics take a second grid-stride pass), translated
    so that a centroid computed from the first pass alone lies far off the surface;
    (points, radius, query subset, oracle normals, eigenvalues) with orient='centroid'."""
    p = surface(BIG_N, 77, offset=(2.0, -1.0, 4.0), jitter=2e-4)
    q = np.sort(np.random.RandomState(1).choice(BIG_N, BIG_QUERIES, replace=False))
    ref, w = DO.estimate_normals(p, BIG_RADIUS, 30, queries=q, orient="centroid")
    return p, BIG_RADIUS, q, ref, w


# ------------------------------------------------------------------------ FPFH
# name -> (n surface points, seed, radius, max_nn).  The SPFH kernel takes neighbours 1..64 in
# a first ballot round and 65..127 in a second: max_nn 65 fills the first round's last lane,
# 66 puts one neighbour into the second, 128 fills it.
FPFH_CASES = {"n300-K30": (300, 31, 0.15, 30), "n700-K65": (700, 32, 0.2, 65), "n700-K66": (700, 34, 0.2, 66),
              "n1500-K128": (1500, 33, 0.2, 128)}


def fpfh_cloud(name):
    """(points, unit normals from the oracle, radius, max_nn): a jittered surface, four of its
    points duplicated (coincident neighbours: d = 0 is skipped) and three isolated points
    (count == 1: an all-zero row)."""
    n, seed, r, K = FPFH_CASES[name]
    s = surface(n, seed)
    far = np.array([(5, 5, 5), (-4, 0, 2), (0, 9, -3)], np.float32)
    p = _shuffled(np.concatenate([s, s[[3, 50, 51, n - 1]], far]), seed)
    nrm, _ = DO.estimate_normals(p, r, 30, orient="centroid")
    return p, nrm, r, K


def fpfh_fragility(pts, normals, radius, max_nn, delta=DELTA, same_inputs=True):
    """Which FPFH rows could legitimately differ between two correct fp64 evaluations,
    from the oracle's own pre-binning values.  A pair is fragile when
      * a scaled feature 11 (f0 + pi) / 2 pi, 11 (f1 + 1) / 2, 11 (f2 + 1) / 2 lies within
        delta of an interior bin edge 1..10 (device atan2 vs libm's could bin it either way);
      * the frame-swap test acos|angle1| > acos|angle2| is a near-tie, 0 < ||angle1| -
        |angle2|| < delta (equal values give equal acos on either side: no swap, not fragile);
      * f3 or |v| is within delta of 0 without being 0 (an exact 0 is the same correctly
        rounded sqrt of the same products on both sides and takes the same early return).
    A row is fragile when one of its own pairs is, or one of a neighbour whose SPFH row it
    reads.  Returns (fragile [n] bool, bound [n]): `bound` is the largest change of any bin
    of the row if every fragile pair flipped.  A flipped pair moves 100 / (c - 1) from one
    bin of a group to another, so SPFH_j changes by at most e_j = pairs_j 100 / (c_j - 1)
    per bin while its group sums stay 100.  The neighbours' rows are weighted by w_k = 1 /
    d2_k, the reciprocal of the SQUARED distance (the `dist2` column, as in the kernel; d2_k
    == 0 is skipped): the normaliser 100 / sum_k (group sum_k w_k) = 1 / sum_k w_k does not
    move, and FPFH_i = SPFH_i + that * sum_k SPFH_k w_k changes by at most e_i + (sum_k e_k
    w_k) / (sum_k w_k).

    same_inputs=False is for two evaluations whose normals differ a little (the CPU check of
    the bound itself): there an exact swap tie and an exact |v| == 0 can go either way too."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    nr = np.asarray(normals, np.float32).astype(np.float64)
    nbr, d2, cnt = DO.radius_knn(pts, radius, max_nn)
    n, K = nbr.shape
    pairs = np.zeros(n, np.int64)
    edges = np.arange(1, 11, dtype=np.float64)
    for k in range(1, K):
        i = np.nonzero(cnt > k)[0]
        if not len(i):
            continue
        j = nbr[i, k]
        f0, f1, f2, a1, a2, f3, vn = DO.pair_features(p[i], nr[i], p[j], nr[j], detail=True)
        x = np.stack([11 * (f0 + np.pi) / (2.0 * np.pi), 11 * (f1 + 1.0) * 0.5, 11 * (f2 + 1.0) * 0.5], 1)
        edge = (np.abs(x[:, :, None] - edges).min(2) < delta).any(1)
        gap = np.abs(np.abs(a1) - np.abs(a2))
        swap = ((gap > 0) | (not same_inputs)) & (gap < delta) & (f3 != 0)
        small = ((f3 > 0) & (f3 < delta)) | ((f3 != 0) & ((vn > 0) | (not same_inputs)) & (vn < delta))
        pairs[i] += edge | swap | small
    e = pairs * (100.0 / np.maximum(cnt - 1, 1))
    reads = (np.arange(K)[None, :] >= 1) & (np.arange(K)[None, :] < cnt[:, None]) & (d2 != 0.0)
    idx = np.where(reads, nbr, 0)
    w = np.where(reads, 1.0 / np.where(reads, d2, 1.0), 0.0)
    fragile = (pairs > 0) | (reads & (pairs[idx] > 0)).any(1)
    wsum = w.sum(1)
    bound = e + np.where(wsum > 0, (w * e[idx]).sum(1) / np.where(wsum > 0, wsum, 1.0), 0.0)
    return fragile, bound


# (n, max_nn, radius): the size ladder through SPFH / FPFH (one wave per point, four per block:
# n % 4 of 0, 1, 2 and 3 end the last block differently).  max_nn = 1 leaves count == 1 on every
# row (all zeros), 2 and 3 one and two pairs; r = 2 holds the whole surface, the other radii
# put about max_nn or more points within reach of an interior point.
FPFH_LADDER = [
    (1, 1, 2.0), (1, 128, 2.0), (2, 1, 2.0), (2, 2, 2.0), (3, 2, 2.0), (3, 3, 2.0), (4, 64, 2.0), (5, 3, 2.0),
    (5, 128, 2.0), (63, 65, 2.0), (64, 127, 2.0), (65, 1, 0.3), (65, 64, 2.0), (255, 2, 0.2), (256, 3, 0.2),
    (257, 128, 0.45), (1023, 1, 0.2), (1023, 65, 0.2),
]


def fpfh_ladder_cloud(n, max_nn, radius):
    """(points, unit normals from the oracle, radius, max_nn): n surface points in general
    position; under 3 points the oracle's normal is (0, 0, 1)."""
    p = surface(n, 600 + n + max_nn)
    nrm, _ = DO.estimate_normals(p, ladder_radius(n), 30, orient="centroid")
    return p, nrm, radius, max_nn


@functools.lru_cache(maxsize=None)
def fpfh_ladder_reference(n, max_nn, radius):
    return _fpfh_reference(*fpfh_ladder_cloud(n, max_nn, radius))


@functools.lru_cache(maxsize=None)
def fpfh_reference(name):
    """dict(pts, normals, radius, max_nn, f, fn, count, d2, fragile, bound) of an FPFH case, computed once."""
    return _fpfh_reference(*fpfh_cloud(name))


def _fpfh_reference(p, nrm, r, K):
    f, fn = DO.compute_fpfh(p, nrm, r, K)
    _, d2, cnt = DO.radius_knn(p, r, K)
    fragile, bound = fpfh_fragility(p, nrm, r, K)
    return dict(pts=p, normals=nrm, radius=r, max_nn=K, f=f, fn=fn, count=cnt, d2=d2, fragile=fragile, bound=bound)
