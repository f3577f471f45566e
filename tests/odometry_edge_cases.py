"""The edge cases of RGB-D odometry (include/pdsc.h f13, csrc/rgbd_odometry.hip),
shared by tests/test_odometry_edge_cases.py (CPU: every case's precondition, an
independent per-pixel restatement of step 1, and the defects the GPU assertions
reject) and tests/test_gpu_odometry_edges.py (the kernels against
tests/fragments_reference.py).  Everything here is numpy and deterministic; the
references are computed once and must not be modified by a test.

Shapes: the smallest at which each path can go wrong.
  8 x 8     level 2 is 2 x 2: every Sobel and Gaussian read there is a clamped read
  8 x 16    the smallest non-square frame
  12 x 20   levels 6 x 10 and 3 x 5: odd sizes
  16 x 16   exactly one 256-pixel chunk at level 0
  16 x 20   one full chunk and a tail of 64
  32 x 32   level 1 is exactly one chunk
  52 x 68   an odd level 2 of 13 x 17, chunk tails at every level
"""
import functools

import numpy as np

import fragments_reference as R

f32 = np.float32
MDD = 0.07
SHAPES = [(8, 8), (8, 16), (12, 20), (16, 16), (16, 20), (32, 32), (52, 68)]
DEPTH_BOUNDS = [(0.0, 4.0), (0.5, 2.5)]  # open3d's default and one with min_depth > 0
IMAGES = ("I", "D", "Idx", "Idy", "Ddx", "Ddy")


def shape_K(H, W):
    return (0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)


# ------------------------------------------------------------------ step 1: the pyramid
BOUND_FRAMES = ("min", "min-", "min+", "max", "max-", "max+")  # frames 4 .. 9 of a pyramid case


def bound_values(mn, mx):
    """The six depths of BOUND_FRAMES: each bound, one fp32 ulp below and one above."""
    mn, mx = f32(mn), f32(mx)
    return [mn, np.nextafter(mn, f32(-1)), np.nextafter(mn, f32(9)), mx, np.nextafter(mx, f32(-1)), np.nextafter(mx, f32(9))]


def bound_kept(val, mn, mx):
    """f13 step 1: d < min_depth, d > max_depth or d <= 0 is invalid; the bounds themselves stay."""
    return not (val < f32(mn) or val > f32(mx) or val <= 0)


@functools.lru_cache(maxsize=None)
def pyramid_case(H, W, mn, mx):
    """(intensity, depth) fp32 [10,H,W] for one call with min_depth = mn, max_depth = mx.
    Frame 0: random depth in [0.8, 2.2] with random holes, holes on the border and in two
    corners, and all six bound values; 1: no valid depth (0, negative, above max_depth,
    NaN); 2: one valid pixel; 3: a smooth surface with one corner hole, so that every
    level has finite pixels next to NaN ones; 4 .. 9: a valid random surface whose centre
    pixel is one of bound_values(mn, mx)."""
    rng = np.random.RandomState(H * 1000 + W + int(mn * 10))
    I = rng.rand(10, H, W).astype(f32)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    D = np.empty((10, H, W), f32)
    D[0] = (0.8 + 1.4 * rng.rand(H, W)).astype(f32)
    D[0][rng.rand(H, W) < 0.08] = 0.0
    for (r, c) in ((0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, 2), (3, W - 1)):
        D[0][r, c] = 0.0
    for k, val in enumerate(bound_values(mn, mx)):
        D[0][2 + k // 3 * 3, 1 + (k % 3) * 2] = val
    D[1] = np.array([0.0, -1.0, mx + 1.0, np.nan], f32)[rng.randint(0, 4, (H, W))]
    D[2] = 0.0
    D[2][H // 2 - 1, W // 2 + 1] = 1.25
    D[3] = (1.5 + 0.3 * np.sin(u / 5.0) + 0.2 * np.cos(v / 4.0)).astype(f32)
    D[3][0, 0] = 0.0
    for k, val in enumerate(bound_values(mn, mx)):
        D[4 + k] = (1.0 + 0.5 * rng.rand(H, W)).astype(f32)
        D[4 + k][H // 2, W // 2] = val
    return I, D


@functools.lru_cache(maxsize=None)
def pyramid_reference(H, W, mn, mx):
    """R.preprocess of every frame of pyramid_case: [frame][level] -> dict of the six images."""
    I, D = pyramid_case(H, W, mn, mx)
    return [R.preprocess(I[f], D[f], mn, mx) for f in range(len(I))]


def assert_images_bitwise(got, want, what=""):
    """Equal bits where `want` is finite, NaN at exactly the same pixels (a NaN's payload is not part of f13)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other pixels"
    bad = (got.view(np.int32) != want.view(np.int32)) & ~nan
    assert not bad.any(), f"{what}: {int(bad.sum())} finite pixels differ, first at {np.argwhere(bad)[0]}"


def ulps(got, want):
    """The largest distance in fp32 ulps over the pixels where both are finite (0 when none is)."""
    ok = np.isfinite(got) & np.isfinite(want)
    if not ok.any():
        return 0
    a, b = got[ok].view(np.int32).astype(np.int64), want[ok].view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max())


# ------------------------------------------------------------------ steps 2 .. 5: one linearisation
@functools.lru_cache(maxsize=None)
def lin_case(H, W):
    """(I [2,H,W], D [2,H,W], K, T).  A smooth surface; the target's holes sit in the top
    left corner region and the source's in the bottom right one, so that the 2 x 2 level
    of the 8 x 8 frame keeps finite pixels next to NaN ones; the bottom left quarter of
    the target is offset by about max_depth_diff in a pattern the filter smears (accepts
    and rejects, none pinned to the threshold: test_gpu_rgbd_odometry.py pins `<=`)."""
    rng = np.random.RandomState(H * 1000 + W + 7)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Ds = (1.5 + 0.3 * np.sin(u / 5.0) + 0.2 * np.cos(v / 4.0)).astype(f32)
    Dt = Ds.copy()
    low_left = (v >= H // 2) & (u < W // 2)
    Dt[low_left & (v % 3 == 1) & (u % 2 == 0)] += f32(MDD + 1e-3)
    Dt[low_left & (v % 3 == 0) & (u % 2 == 1)] -= f32(MDD - 1e-3)
    Dt[(rng.rand(H, W) < 0.15) & (v < H // 4) & (u < W // 4)] = 0.0
    Ds[(rng.rand(H, W) < 0.15) & (v >= H - H // 4) & (u >= W - W // 4)] = 0.0
    Dt[0, 0] = Dt[0, 2] = 0.0        # a corner and a border pixel
    Ds[H - 1, W - 1] = Ds[H - 1, W - 3] = 0.0
    I = rng.rand(2, H, W).astype(f32)
    T = R.exp6(np.array([0.01, -0.02, 0.015, 0.06, -0.03, 0.02]))
    return I, np.stack([Ds, Dt]), shape_K(H, W), T


@functools.lru_cache(maxsize=None)
def lin_reference(H, W, level):
    """(JtJ, Jtr, n, abs_JtJ, abs_Jtr, corr, (a_s, a_t)) of lin_case(H, W) at `level`."""
    I, D, K, T = lin_case(H, W)
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    a_s, a_t = R.intensity_scales(P[0][0], P[1][0], K, T, MDD)
    return R.linearize(P[0][level], P[1][level], R.level_K(K, level), T, MDD, a_s, a_t) + ((a_s, a_t),)


def projections(Ls, K, T):
    """Per source pixel: (finite depth and p.z > 0, uf, vf, p.z) in f13 step 3's operation order."""
    fx, fy, cx, cy = K
    H, W = Ls["D"].shape
    with np.errstate(invalid="ignore", divide="ignore"):
        d = Ls["D"].reshape(-1).astype(np.float64)
        i = np.arange(H * W)
        X, Y = (((i % W).astype(np.float64) - cx) * d) / fx, (((i // W).astype(np.float64) - cy) * d) / fy
        px, py, pz = R.apply_T(T, X, Y, d)
        ok = np.isfinite(d) & (pz > 0)
        return ok, (fx * px) / pz + cx + 0.5, (fy * py) / pz + cy + 0.5, pz


@functools.lru_cache(maxsize=None)
def rounding_case():
    """"The smallest p.z rounded to fp32": a fronto-parallel plane at depth 1 under a
    translation of 1 along z and a rotation of 1e-12 about y.  The image shrinks by two,
    so four source pixels land on one target pixel; p.z = 2 - 1e-12 X in fp64 falls with
    the column, and every p.z rounds to 2 in fp32.  The contract's key (fp32 bits, then
    the lowest index) keeps the lowest index, which has the LARGEST fp64 p.z of its four;
    a key on fp64 p.z keeps the right column.  (I, D, K, T); level 0."""
    H, W, K = 8, 16, (8.0, 8.0, 7.5, 3.5)
    I = np.random.RandomState(3).rand(2, H, W).astype(f32)
    D = np.stack([np.full((H, W), 1.0, f32), np.full((H, W), 2.0, f32)])
    T = R.exp6(np.array([0.0, 1e-12, 0.0, 0.0, 0.0, 1.0]))
    return I, D, K, T


@functools.lru_cache(maxsize=None)
def truncation_case():
    """int(uf) truncates toward 0: a plane at depth 1.5 seen from 0.125 closer, so the
    image grows by 12 / 11 about its centre: column 0 lands at uf = -0.18 (column 0, not
    -1), row 0 likewise, and the last column and row leave the image at uf >= W.
    (I, D, K, T); 16 x 16, level 0."""
    H, W, K = 16, 16, (14.4, 14.4, 7.5, 7.5)
    I = np.random.RandomState(11).rand(2, H, W).astype(f32)
    D = np.stack([np.full((H, W), 1.5, f32), np.full((H, W), 1.375, f32)])
    T = np.eye(4)
    T[2, 3] = -0.125
    return I, D, K, T


@functools.lru_cache(maxsize=None)
def map_reference(which):
    """corr of rounding_case / truncation_case at level 0 and the two level-0 pyramids."""
    I, D, K, T = {"rounding": rounding_case, "truncation": truncation_case}[which]()
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    return R.correspondences(P[0][0], P[1][0], K, T, MDD)[0], P


# ------------------------------------------------------------------ the renders: steps and batches
SCENE_K, SCENE_H, SCENE_W = (56.0, 56.0, 31.5, 23.5), 48, 64
BATCH_ITERATIONS = (3, 2, 1)  # not the default, and short: the one full run is in test_gpu_rgbd_odometry.py


@functools.lru_cache(maxsize=None)
def scene():
    """(I, D) fp32 [5,48,64]: test_gpu_rgbd_odometry.test_batch_independence's four renders,
    and frame 4 = frame 1's intensity without one valid depth (the failing pair's target)."""
    poses = [np.eye(4)]
    for k in range(3):
        poses.append(poses[-1] @ R.small_motion(0.003 * (k + 1), -0.004, 0.002 * k, (0.01, 0.004 * k, -0.006)))
    fr = [R.render(p, SCENE_K, SCENE_H, SCENE_W) for p in poses]
    I = np.stack([f[0] for f in fr] + [fr[1][0]])
    D = np.stack([f[1] for f in fr] + [np.zeros((SCENE_H, SCENE_W), f32)])
    return I, D


@functools.lru_cache(maxsize=None)
def scene_pyramids():
    I, D = scene()
    return [R.preprocess(I[f], D[f]) for f in range(len(I))]


INITS = [R.exp6(np.array([0.004, -0.003, 0.002, 0.01, -0.005, 0.004])),
         R.exp6(np.array([-0.006, 0.002, 0.005, -0.008, 0.006, -0.003])),
         R.exp6(np.array([0.002, 0.007, -0.004, 0.004, 0.009, 0.006]))]

# (name, pair, iterations, init or None): one iteration at one level -- iterations[k] is level 2 - k
STEP_CASES = [("level2", (0, 1), (1, 0, 0), None), ("level1", (0, 1), (0, 1, 0), None),
              ("level0", (0, 1), (0, 0, 1), None), ("level2_init", (1, 2), (1, 0, 0), INITS[0]),
              ("level0_init", (2, 3), (0, 0, 1), INITS[1])]
ZERO_CASES = [("none", (0, 1), None), ("none_init", (1, 2), INITS[2]), ("none_failing", (0, 4), INITS[0])]
STEP_LEVEL = {(1, 0, 0): 2, (0, 1, 0): 1, (0, 0, 1): 0}


@functools.lru_cache(maxsize=None)
def step_reference(name):
    """The restatement's (trans, info, success, n_corr_last, iterations_run) of a STEP_CASES / ZERO_CASES row."""
    P = scene_pyramids()
    for n, (s, t), its, init in STEP_CASES + [(n, p, (0, 0, 0), i) for n, p, i in ZERO_CASES]:
        if n == name:
            return R.odometry_pair(P[s], P[t], SCENE_K, init, MDD, its)
    raise KeyError(name)


FAILING = (0, 4)
GOOD_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 0)]


def failing_batch(position):
    """Five pairs with the failing one at `position`, and five different inits."""
    pairs = list(GOOD_PAIRS)
    pairs.insert(position, FAILING)
    inits = [R.aff_mul(INITS[k % 3], INITS[(k + 1) % 3]) if k >= 3 else INITS[k] for k in range(5)]
    return pairs, np.stack(inits)


FAILING_POSITIONS = (0, 2, 4)
INIT_BATCH = ([(0, 1), (1, 2), (0, 1)], np.stack(INITS))  # P = 3; pairs 0 and 2 differ only in their init
REVERSE_BATCH = [(1, 2), (2, 1)]
UNNAMED_PAIRS = [(0, 1), (3, 2), (1, 3)]


def unnamed_frames():
    """(I, D) [6,48,64]: the four renders, then a frame of NaN and a frame of +-Inf that no pair names."""
    I, D = scene()
    bad = np.full((2, SCENE_H, SCENE_W), np.nan, f32)
    bad[1] = np.inf
    bad[1, ::2] = -np.inf
    return np.concatenate([I[:4], bad]), np.concatenate([D[:4], bad])


# ------------------------------------------------------------------ conversion
CONVERT_SCALE, CONVERT_TRUNCS = 1000.0, (3.0, 100.0)


def convert_case():
    """(color uint8 [1,4,8,3], depth16 uint16 [1,4,8]): 0, 1, the int16 sign bit from both
    sides, 65535, exactly depth_trunc depth_scale (kept: the test is `>`) and one above;
    colours 0 and 255 in every channel combination."""
    d = np.array([0, 1, 32767, 32768, 65535, 3000, 3001, 2999] * 4, np.uint16).reshape(1, 4, 8)
    c = np.zeros((1, 4, 8, 3), np.uint8)
    for k in range(8):
        c[0, 0, k] = [255 * (k & 1), 255 * (k >> 1 & 1), 255 * (k >> 2 & 1)]
    c[0, 1:] = np.random.RandomState(9).randint(0, 256, (3, 8, 3))
    return c, d
