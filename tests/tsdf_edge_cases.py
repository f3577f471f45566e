"""The sparse TSDF volume's edge cases (DESIGN.md "Fragments: edge cases"), shared by
the CPU tests (test_tsdf_edge_cases.py) and the GPU tests (test_gpu_tsdf_edges.py,
test_gpu_tsdf.py).  Plain numpy: the reference is tests/fragments_reference.Volume.

Integrate cases (integrate_cases()): synthetic depth and colour frames built
directly.  Hash cases: hash_sets(), EXTREME, OUTSIDE and block_data().  Extraction
cases (extraction_cases()): states fabricated for write_blocks, listed in a write
order that is NOT the key order.  Every case asserts its own preconditions in
test_tsdf_edge_cases.py, on the restatement, so none passes vacuously.

The bars are test_gpu_tsdf.py's: block sets, weights and counts exact; tsdf and
colour within 2 fp32 ulps; extracted positions within 1e-6 voxel_length and
colours within 1e-6, row by row in the emitted order."""
import functools

import numpy as np

import fragments_reference as R

f32 = np.float32
NV = 4096
LIM = 1 << 20
OFF = np.stack([np.arange(NV) & 15, (np.arange(NV) >> 4) & 15, np.arange(NV) >> 8], 1)  # voxel index -> (x, y, z)


# ------------------------------------------------------------------ the bars
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def ulps(a, b):
    a, b = np.ascontiguousarray(_np(a), f32), np.ascontiguousarray(_np(b), f32)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def assert_blocks_equal(got, ref):
    """got: (coords, tsdf, weight, colour) sorted by key; ref: a Volume or such a tuple.
    Returns the worst ulp distance seen."""
    coords, tsdf, weight, colour = (_np(x) for x in got)
    rc, rt, rw, rcol = ref.sorted_blocks() if hasattr(ref, "sorted_blocks") else ref
    assert np.array_equal(coords, rc)
    assert np.array_equal(np.ascontiguousarray(weight).view(np.int32), np.ascontiguousarray(rw).view(np.int32))
    ut, uc = ulps(tsdf, rt), ulps(colour, rcol)
    assert ut <= 2 and uc <= 2, (ut, uc)
    return max(ut, uc)


def assert_blocks_bitwise(got, ref):
    for a, b in zip(got, ref):
        a, b = np.ascontiguousarray(_np(a)), np.ascontiguousarray(_np(b))
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_points_equal(p, c, rp, rc, vl):
    """Row by row, in the emitted order.  Returns (worst position error / voxel_length, worst colour error)."""
    p, c = _np(p), _np(c)
    assert p.shape == rp.shape and c.shape == rc.shape, (p.shape, rp.shape)
    if not len(rp):
        return 0.0, 0.0
    ep, ec = float(np.abs(p - rp).max()), float(np.abs(c - rc).max())
    assert ep <= 1e-6 * vl and ec <= 1e-6, (ep / vl, ec)
    return ep / vl, ec


# ------------------------------------------------------------------ integrate cases
class IntegrateCase:
    """frames: [(depth fp32 [H,W], colour uint8 [H,W,3], extrinsic fp64 [4,4])]; `error`:
    (frame index, "outside" | "full") for the one frame that must fail, or None."""

    def __init__(self, name, vl, trunc, K, frames, max_blocks=512, error=None):
        self.name, self.vl, self.trunc, self.K, self.frames = name, vl, trunc, K, frames
        self.max_blocks, self.error = max_blocks, error


POSE = R.exp6(np.array([0.02, -0.03, 0.01, -0.3, -0.2, -0.9]))  # the scene straddles the world origin


def _uv(H, W):
    return np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")


def _frame(H, W, seed, pose=POSE, slope=(0.013, -0.007), base=1.0, noise=0.004):
    """A tilted plane of depth with noise on the pixels the touch does not sample."""
    rng = np.random.default_rng(seed)
    v, u = _uv(H, W)
    depth = base + slope[0] * u + slope[1] * v
    jitter = rng.uniform(-noise, noise, (H, W))
    jitter[::4, ::4] = 0.0
    colour = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return (depth + jitter).astype(f32), colour, np.linalg.inv(pose)


def _K(H, W, f=24.0):
    return (f, f, W / 2.0, H / 2.0)


SIZES = ((1, 1), (3, 5), (4, 4), (5, 9), (7, 13), (24, 32))
SUBSET_DROPS = (0, 2, 4, 7, 9)  # frame k of subset5 has no depth at the first SUBSET_DROPS[k] sampled pixels


@functools.lru_cache(maxsize=None)
def integrate_cases():
    cases = []
    step = R.small_motion(0.01, -0.02, 0.01, (0.05, -0.02, 0.03))
    for H, W in SIZES:
        cases.append(IntegrateCase(f"size_{H}x{W}", 0.01, 0.04, _K(H, W),
                                   [_frame(H, W, 100 + H), _frame(H, W, 200 + H, POSE @ step)]))
    # voxel centres at uf, vf in (-1, 0): a rotated camera, depth everywhere, blocks that reach past every image edge
    tilt = POSE @ R.exp6(np.array([0.2, -0.15, 0.3, 0.0, 0.0, 0.0]))
    cases.append(IntegrateCase("edge_uv", 0.01, 0.04, _K(5, 9), [_frame(5, 9, 31, tilt), _frame(5, 9, 32, tilt @ step)]))
    # the camera inside the touched blocks: depth of 5 .. 9 cm under a 4 cm truncation
    cases.append(IntegrateCase("camera_inside", 0.01, 0.04, _K(8, 8, 6.0),
                               [_frame(8, 8, 41, base=0.05, slope=(0.004, 0.001), noise=0.002)]))
    # dyadic: depth 1 + 1/128, voxel 1/64, truncation 1/16, the identity pose, integer cx, cy: on the rays of the
    # pixel (2, 2) sdf is (64 - i) / 64 exactly, -sdf_trunc at the voxel plane i = 68 and +sdf_trunc at i = 60
    d = np.full((5, 5), 1.0 + 1.0 / 128.0, f32)
    col = np.random.default_rng(51).integers(0, 256, (5, 5, 3), dtype=np.uint8)
    cases.append(IntegrateCase("dyadic", 1.0 / 64, 1.0 / 16, (16.0, 16.0, 2.0, 2.0), [(d, col, np.eye(4)), (d, col, np.eye(4))]))
    # invalid depth of every kind, in sampled pixels and between them
    bad = _frame(7, 13, 61)
    bd = bad[0].copy()
    bd[0, 4], bd[4, 0], bd[4, 8], bd[0, 12] = 0.0, -1.0, np.nan, -np.inf
    bd[1, 1], bd[2, 5], bd[3, 9], bd[5, 6], bd[6, 11] = 0.0, -0.5, np.nan, np.nan, 0.0
    bd[2:4, 2:4] = 0.0
    cases.append(IntegrateCase("bad_depth", 0.01, 0.04, _K(7, 13), [bad, (bd, bad[1], bad[2]), (bd, bad[1], np.linalg.inv(POSE @ step))]))
    inf = _frame(7, 13, 62, POSE @ step @ step)
    fd = inf[0].copy()
    fd[4, 8] = np.inf
    cases.append(IntegrateCase("bad_depth_inf", 0.01, 0.04, _K(7, 13), [bad, (fd, inf[1], inf[2])], error=(1, "outside")))
    # a truncation wider than a block edge (0.25): every sample touches at least 3 x 3 x 3 blocks
    cases.append(IntegrateCase("big_trunc", 1.0 / 64, 0.3, _K(4, 8), [_frame(4, 8, 71), _frame(4, 8, 72, POSE @ step)]))
    cases.append(IntegrateCase("tiny_trunc", 0.01, 0.004, _K(7, 13), [_frame(7, 13, 81), _frame(7, 13, 82)]))
    cases.append(IntegrateCase("vl_0.023", 0.023, 0.05, _K(7, 13), [_frame(7, 13, 91), _frame(7, 13, 92, POSE @ step)]))
    # five frames from one pose; frame k loses the depth of more sampled pixels, so it touches a strict subset
    frames = []
    for k, drop in enumerate(SUBSET_DROPS):
        dk, ck, E = _frame(12, 16, 300 + k)
        for s in range(drop):
            dk[4 * (s // 4), 4 * (s % 4)] = 0.0
        frames.append((dk, ck, E))
    cases.append(IntegrateCase("subset5", 0.01, 0.04, _K(12, 16), frames))
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def overflow_case():
    """Two frames that fit, a third from another place that does not (max_blocks = 3 more than the two need),
    a fourth that touches only blocks the volume holds.  Returns (IntegrateCase, blocks after two frames)."""
    far = POSE @ R.exp6(np.array([0.0, 0.5, 0.0, 0.6, 0.1, 0.0]))
    frames = [_frame(12, 16, 401), _frame(12, 16, 402), _frame(12, 16, 403, far), _frame(12, 16, 404)]
    vol = R.Volume(0.01, 0.04)
    for d, c, E in frames[:2]:
        assert vol.integrate(d, c, _K(12, 16), E)
    n2 = len(vol.blocks)
    return IntegrateCase("overflow", 0.01, 0.04, _K(12, 16), frames, max_blocks=n2 + 3, error=(2, "full")), n2


def run_reference(case, cls=R.Volume):
    """The case through `cls`: (volume, [(touched or None, sorted_blocks() after the frame)]).  The failing
    frame of a case must raise / return False and is recorded with touched = None."""
    vol = cls(case.vl, case.trunc, case.max_blocks)
    snaps = []
    for k, (d, c, E) in enumerate(case.frames):
        if case.error and case.error[0] == k:
            if case.error[1] == "outside":
                try:
                    vol.integrate(d, c, case.K, E)
                    raise AssertionError("the frame must be out of range")
                except R.TsdfError as e:
                    assert "outside" in str(e)
            else:
                assert vol.integrate(d, c, case.K, E) is False
            snaps.append((None, vol.sorted_blocks()))
            continue
        touched = vol.touched(d, case.K, E)
        assert vol.integrate(d, c, case.K, E)
        snaps.append((touched, tuple(x.copy() for x in vol.sorted_blocks())))
    return vol, snaps


@functools.lru_cache(maxsize=None)
def reference_run(name):
    return run_reference(integrate_cases()[name])


# ------------------------------------------------------------------ hash and capacity cases
EXTREME = np.array([(-LIM, -LIM, -LIM), (LIM - 1, LIM - 1, LIM - 1), (-LIM, LIM - 1, -LIM), (LIM - 1, -LIM, LIM - 1),
                    (0, -LIM, LIM - 1), (LIM - 1, 0, -LIM)], dtype=np.int32)
OUTSIDE = np.array([(LIM, 0, 0), (0, -LIM - 1, 0), (0, 0, LIM), (-LIM - 1, -LIM - 1, -LIM - 1), (3, LIM, -LIM - 1)],
                   dtype=np.int32)


@functools.lru_cache(maxsize=None)
def hash_sets():
    """40 sets of 16 distinct block coordinates: 20 from the cube [-2, 2)^3, 20 from the whole range."""
    rng = np.random.default_rng(7)
    sets = []
    cube = np.stack(np.meshgrid(*[np.arange(-2, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for _ in range(20):
        sets.append(cube[rng.permutation(64)[:16]].astype(np.int32))
    for _ in range(20):
        while True:
            s = rng.integers(-LIM, LIM, (16, 3))
            if len({tuple(r) for r in s.tolist()}) == 16:
                break
        sets.append(s.astype(np.int32))
    return sets


N_WRAP_SETS = 600


@functools.lru_cache(maxsize=None)
def wrap_sets():
    """N_WRAP_SETS more sets of 16 distinct coordinates from the whole range, for the wrap at the table's end.
    Under any hash that spreads such keys evenly over the 64 entries, two or more of a set's 16 keys have the LAST
    entry as their home with probability 1 - (63/64)^16 - 16 (1/64) (63/64)^15 = 0.0253, and the second of them
    must then probe from entry 63 to entry 0.  With the 20 whole-range sets of hash_sets() that is 620 sets: no
    wrap in any of them has probability 0.9747^620 < 2e-7 (chains that merely reach the last entry make it smaller)."""
    rng = np.random.default_rng(70)
    sets = []
    while len(sets) < N_WRAP_SETS:
        s = rng.integers(-LIM, LIM, (16, 3))
        if len({tuple(r) for r in s.tolist()}) == 16:
            sets.append(s.astype(np.int32))
    return sets


def block_data(n, seed):
    """(tsdf, weight, colour) for n blocks: tsdf in [-1, 1], weights 0 .. 5, colours in [0, 255]."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, NV)).astype(f32), rng.integers(0, 6, (n, NV)).astype(f32),
            rng.uniform(0, 255, (n, NV, 3)).astype(f32))


# ------------------------------------------------------------------ extraction cases
class ExtractCase:
    """A state for write_blocks: coords int32 [n,3] in WRITE order (not key order), tsdf / weight [n,4096],
    colour [n,4096,3]."""

    def __init__(self, name, vl, coords, tsdf, weight, colour, seed=0):
        order = np.random.default_rng(1000 + seed).permutation(len(coords))
        self.name, self.vl = name, vl
        self.coords = np.asarray(coords, np.int32).reshape(-1, 3)[order]
        self.tsdf, self.weight, self.colour = tsdf[order], weight[order], colour[order]

    def without(self, i, name):
        keep = [j for j in range(len(self.coords)) if j != i]
        c = ExtractCase.__new__(ExtractCase)
        c.name, c.vl = name, self.vl
        c.coords, c.tsdf, c.weight, c.colour = self.coords[keep], self.tsdf[keep], self.weight[keep], self.colour[keep]
        return c

    def volume(self, cls=R.Volume, max_blocks=32):
        vol = cls(self.vl, 4 * self.vl, max_blocks)
        vol.write_blocks(self.coords, self.tsdf, self.weight, self.colour)
        return vol


GROUP = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
# both surfaces pass through all 8 blocks and cut the three centre faces obliquely; the origin is inside the sphere
PLANE_N = np.array([0.15, 0.1, 1.0]) / np.linalg.norm([0.15, 0.1, 1.0])
SPHERE_C, SPHERE_R = np.array([5.3, -4.4, 3.2]), 11.3


def _centres(coords):
    """voxel centres in voxel units, [n, 4096, 3]"""
    return (np.asarray(coords)[:, None, :] * 16 + OFF[None]).astype(np.float64) + 0.5


def _field(kind, coords):
    c = _centres(coords)
    dist = c @ PLANE_N - 0.3 if kind == "plane" else np.linalg.norm(c - SPHERE_C, axis=-1) - SPHERE_R
    return np.clip(dist / 4.0, -1.0, 1.0).astype(f32)


def _state(coords, tsdf, seed):
    rng = np.random.default_rng(seed)
    n = len(coords)
    return tsdf, rng.integers(1, 6, (n, NV)).astype(f32), rng.uniform(0, 255, (n, NV, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def extraction_cases():
    vl = 0.01
    cases = []
    for kind in ("plane", "sphere"):
        full = ExtractCase(f"group_{kind}", vl, GROUP, *_state(GROUP, _field(kind, GROUP), 5), seed=len(kind))
        cases.append(full)
        for i in range(8):
            cases.append(full.without(i, f"group_{kind}_minus_{i}"))
    for seed in (1, 2, 3):
        t, w, c = _state(GROUP, _field("sphere", GROUP), 5)
        w[np.random.default_rng(50 + seed).random(w.shape) < 0.05] = 0.0
        cases.append(ExtractCase(f"group_sphere_w0_seed{seed}", vl, GROUP, t, w, c, seed=seed))
    # the centre corner alone: voxel (0, 0, 0) of block (0, 0, 0) is negative under positive -x and -y neighbours,
    # and has weight 0, so every cube around the centre is invalid through its corner in ANOTHER block
    t, w, c = _state(GROUP, _field("plane", GROUP), 5)
    t[GROUP.index((0, 0, 0)), 0] = -0.9
    w[GROUP.index((0, 0, 0)), 0] = 0.0
    cases.append(ExtractCase("group_centre_w0", vl, GROUP, t, w, c, seed=9))
    # signed zeros beside both signs: a random field over {-0.5, 0.5, 0.0, -0.0}
    rng = np.random.default_rng(77)
    t = np.array([-0.5, 0.5, 0.0, -0.0], f32)[rng.integers(0, 4, (8, NV))]
    cases.append(ExtractCase("group_zeros", vl, GROUP, *_state(GROUP, t, 6), seed=7))
    # one block alone
    one = [(3, -2, 5)]
    t = np.clip((np.linalg.norm(_centres(one) - (np.array(one[0]) * 16 + 8.2), axis=-1) - 9.7) / 4.0, -1, 1).astype(f32)
    cases.append(ExtractCase("single_block", vl, one, *_state(one, t, 8)))
    # extreme coordinates: a lone block at the lowest corner, and a pair along x at the highest x whose shared face the
    # surface crosses (the pair's +y neighbours are out of range: absent)
    ext = [(-LIM, -LIM, -LIM), (LIM - 2, LIM - 1, -LIM), (LIM - 1, LIM - 1, -LIM)]
    local = np.stack([OFF + 0.5] * 3).astype(np.float64)
    local[2, :, 0] += 16.0
    t = np.stack([np.clip((np.linalg.norm(local[0] - 7.7, axis=-1) - 5.2) / 4.0, -1, 1),
                  np.clip((local[1] @ np.array([1.0, 0.08, -0.05]) - 16.2) / 4.0, -1, 1),
                  np.clip((local[2] @ np.array([1.0, 0.08, -0.05]) - 16.2) / 4.0, -1, 1)]).astype(f32)
    cases.append(ExtractCase("extreme", vl, ext, *_state(ext, t, 10), seed=3))
    # in key order: a sparse block, a block that emits nothing, then a group whose first block flags all three axes
    # of every voxel (a checkerboard over the block and the first layer of its +x, +y, +z neighbours)
    coords = [(-3, 0, 0), (-2, 5, 5)] + GROUP
    g = np.asarray(coords)[:, None, :] * 16 + OFF[None]
    mag = np.random.default_rng(12).uniform(0.2, 0.9, g.shape[:2])
    t = np.where(np.all((g >= -16) & (g <= 0), -1), mag * (1 - 2 * (g.sum(-1) & 1)), 0.7)
    t[0] = np.clip((np.linalg.norm(_centres(coords[:1])[0] - (np.array(coords[0]) * 16 + 7.6), axis=-1) - 4.4) / 4.0, -1, 1)
    t[1] = 0.7
    cases.append(ExtractCase("dense_checker", vl, coords, *_state(coords, t.astype(f32), 13), seed=5))
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def reference_extract(name):
    """(volume, points, colours, keys [n,3] = (block key, voxel index, axis)) of the restatement."""
    vol = extraction_cases()[name].volume()
    p, c, _ = vol.extract()
    return vol, p, c, vol.last_keys
