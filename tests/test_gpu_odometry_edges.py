"""RGB-D odometry on the GPU (csrc/rgbd_odometry.hip, include/pdsc.h f13) stage by
stage at the edge cases of tests/odometry_edge_cases.py, against the numpy
restatement tests/fragments_reference.py.  tests/test_odometry_edge_cases.py asserts
each case's precondition, pins the restatement's step 1 to a per-pixel loop and shows
that these assertions reject single-rule defects.

Bars.  Pyramid: 0 ulps where finite, NaN at exactly the same pixels -- the library
is built without contraction and f13 fixes the order of every fp32 operation.
Linearise: corr and the count exact, scales rtol 1e-12, sums within 1e-9 sum |terms|
(test_gpu_rgbd_odometry.py's bars).  One step: |trans - T_ref| <= 1e-6 per entry,
iterations_run == 1, n_corr_last equal, info rtol = atol = 1e-9, with the correspondence
map at that level under init asserted identical first.  Batch: bitwise against the
pair's run alone.  Conversion: exact.

Left out: a failure that first occurs at a finer level.  NaN only grows toward the
coarser levels, so depth holes alone give no pair that has correspondences at level
2 and none at level 1."""
import numpy as np
import pytest
import torch

import fragments_reference as R
import odometry_edge_cases as C
from pointdsc_amd import fragments as F

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


# ------------------------------------------------------------------ step 1
@pytest.mark.parametrize("mn,mx", C.DEPTH_BOUNDS)
@pytest.mark.parametrize("H,W", C.SHAPES)
def test_pyramid(gpu_device, H, W, mn, mx):
    I, D = C.pyramid_case(H, W, mn, mx)
    ref = C.pyramid_reference(H, W, mn, mx)
    gI, gD = _t(I, gpu_device), _t(D, gpu_device)
    worst, bad = 0, []
    for level in range(3):
        got = F.rgbd_odometry_pyramid(gI, gD, level, mn, mx)
        for name in C.IMAGES:
            g = got[name].cpu().numpy()
            assert g.shape == (len(I), H >> level, W >> level)
            for f in range(len(I)):
                worst = max(worst, C.ulps(g[f], ref[f][level][name]))
                try:
                    C.assert_images_bitwise(g[f], ref[f][level][name], f"frame {f} L{level} {name}")
                except AssertionError as e:
                    bad.append(str(e))
    print(f"pyramid {H}x{W} [{mn}, {mx}]: worst {worst} ulps, {len(bad)} images differ")
    assert not bad, "\n".join(bad[:10])


def test_pyramid_null_outputs(gpu_device):
    """Any of the six may be NULL: D alone is the D of the full call, and a guard row behind it stays."""
    from pointdsc_amd._call import call
    I, D = C.pyramid_case(8, 16, 0.0, 4.0)
    gI, gD = _t(I, gpu_device), _t(D, gpu_device)
    full = F.rgbd_odometry_pyramid(gI, gD, 1)
    out = torch.full((len(I) + 1, 4, 8), -7.0, dtype=torch.float32, device=gpu_device)
    call("pdsc_rgbd_odometry_pyramid", gI, gD, len(I), 8, 16, 0.0, 4.0, 1, None, out, None, None, None, None,
         device=gpu_device, ws=("pdsc_rgbd_odometry_workspace_bytes", len(I), 8, 16, 1))
    C.assert_images_bitwise(out[:-1].cpu().numpy(), full["D"].cpu().numpy())
    assert bool((out[-1] == -7.0).all())


# ------------------------------------------------------------------ steps 2 .. 5, one linearisation
def _assert_linearisation(got, ref, tag):
    g_corr, g_JtJ, g_Jtr, g_n, g_sc = got
    JtJ, Jtr, n, aJJ, aJr, corr, scales = ref
    assert np.array_equal(g_corr[0].cpu().numpy().astype(np.int64), corr), tag
    assert int(g_n[0]) == n, tag
    np.testing.assert_allclose(g_sc[0].cpu().numpy(), scales, rtol=1e-12)
    dJ, dr = np.abs(g_JtJ[0].cpu().numpy() - JtJ), np.abs(g_Jtr[0].cpu().numpy() - Jtr)
    ratio = max(np.max(dJ / np.maximum(1e-9 * aJJ, 1e-300)), np.max(dr / np.maximum(1e-9 * aJr, 1e-300)))
    print(f"{tag}: n={n} of {len(corr)}, worst sums ratio to the bar {ratio:.2e}")
    assert np.all(dJ <= 1e-9 * aJJ) and np.all(dr <= 1e-9 * aJr), tag


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("H,W", C.SHAPES)
def test_linearise(gpu_device, H, W, level):
    I, D, K, T = C.lin_case(H, W)
    got = F.rgbd_odometry_linearize(_t(I, gpu_device), _t(D, gpu_device), K, [(0, 1)], _t(T[None], gpu_device), level,
                                    C.MDD)
    _assert_linearisation(got, C.lin_reference(H, W, level), f"{H}x{W} L{level}")


@pytest.mark.parametrize("which", ["rounding", "truncation"])
def test_map_rules(gpu_device, which):
    """The smallest p.z ROUNDED TO FP32 with ties to the lowest index; int(uf) truncates toward 0."""
    I, D, K, T = {"rounding": C.rounding_case, "truncation": C.truncation_case}[which]()
    corr, _ = C.map_reference(which)
    g_corr = F.rgbd_odometry_linearize(_t(I, gpu_device), _t(D, gpu_device), K, [(0, 1)], _t(T[None], gpu_device), 0,
                                       C.MDD)[0][0].cpu().numpy()
    assert np.array_equal(g_corr, corr)


# ------------------------------------------------------------------ one step per level, and none
def _scene(dev):
    I, D = C.scene()
    return _t(I, dev), _t(D, dev)


def _init(init, dev):
    return None if init is None else _t(np.asarray(init)[None], dev)


@pytest.mark.parametrize("name", [c[0] for c in C.STEP_CASES])
def test_one_step(gpu_device, name):
    _, (s, t), its, init = next(c for c in C.STEP_CASES if c[0] == name)
    level = C.STEP_LEVEL[its]
    I, D = _scene(gpu_device)
    P = C.scene_pyramids()
    T0 = np.eye(4) if init is None else init
    # the same correspondences under init at that level, or a difference of the step says nothing
    a_s, a_t = R.intensity_scales(P[s][0], P[t][0], C.SCENE_K, T0, C.MDD)
    lin = R.linearize(P[s][level], P[t][level], R.level_K(C.SCENE_K, level), T0, C.MDD, a_s, a_t)
    _assert_linearisation(F.rgbd_odometry_linearize(I, D, C.SCENE_K, [(s, t)], _init(init, gpu_device), level, C.MDD),
                          lin + ((a_s, a_t),), f"{name} under init")
    T_ref, info_ref, ok, n_ref, runs = C.step_reference(name)
    trans, info, success, status = F.rgbd_odometry(I, D, C.SCENE_K, [(s, t)], init=_init(init, gpu_device),
                                                   max_depth_diff=C.MDD, iterations=its, want_status=True)
    st = status[0].cpu().numpy()
    dT = np.abs(trans[0].cpu().numpy() - T_ref).max()
    print(f"{name}: max |dT| {dT:.2e}, n_corr {st[1]} vs {n_ref}")
    assert ok and bool(success[0]) and st[0] == 1 and st[2] == runs == 1 and st[1] == n_ref == lin[2]
    assert dT <= 1e-6
    np.testing.assert_allclose(info[0].cpu().numpy(), info_ref, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("name", [c[0] for c in C.ZERO_CASES])
def test_no_iteration(gpu_device, name):
    """iterations = (0, 0, 0): init bit for bit, and what odometry_pair gives for the rest
    (success: no iteration failed; n_corr_last 0; the information of the level-0 map under init)."""
    _, (s, t), init = next(c for c in C.ZERO_CASES if c[0] == name)
    I, D = _scene(gpu_device)
    T_ref, info_ref, ok, n_ref, runs = C.step_reference(name)
    trans, info, success, status = F.rgbd_odometry(I, D, C.SCENE_K, [(s, t)], init=_init(init, gpu_device),
                                                   max_depth_diff=C.MDD, iterations=(0, 0, 0), want_status=True)
    assert np.array_equal(_bits(trans[0]), T_ref.view(np.int64))
    assert status[0].cpu().tolist() == [int(ok), n_ref, runs, 0] == [1, 0, 0, 0] and bool(success[0])
    np.testing.assert_allclose(info[0].cpu().numpy(), info_ref, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ batches
def _run(I, D, pairs, inits, dev):
    init = None if inits is None else _t(np.asarray(inits), dev)
    return F.rgbd_odometry(I, D, C.SCENE_K, pairs, init=init, max_depth_diff=C.MDD, iterations=C.BATCH_ITERATIONS,
                           want_status=True)


def _assert_pair_is(batch, p, alone):
    assert np.array_equal(_bits(batch[0][p]), _bits(alone[0][0])), f"pair {p}: trans"
    assert np.array_equal(_bits(batch[1][p]), _bits(alone[1][0])), f"pair {p}: info"
    assert torch.equal(batch[3][p], alone[3][0]), f"pair {p}: status"


@pytest.mark.parametrize("position", C.FAILING_POSITIONS)
def test_failing_pair_in_a_batch(gpu_device, position):
    I, D = _scene(gpu_device)
    pairs, inits = C.failing_batch(position)
    batch = _run(I, D, pairs, inits, gpu_device)
    again = _run(I, D, pairs, inits, gpu_device)
    for x, y in zip(batch, again):
        assert torch.equal(x, y)
    for p, pair in enumerate(pairs):
        if pair == C.FAILING:
            assert np.array_equal(_bits(batch[0][p]), inits[p].view(np.int64))
            assert batch[3][p].cpu().tolist() == [0, 0, 0, 0] and not bool(batch[2][p])
            assert float(batch[1][p].abs().max()) == 0.0
        else:
            assert batch[3][p].cpu().tolist()[::2] == [1, sum(C.BATCH_ITERATIONS)]
            _assert_pair_is(batch, p, _run(I, D, [pair], inits[p:p + 1], gpu_device))


def test_per_pair_init(gpu_device):
    I, D = _scene(gpu_device)
    pairs, inits = C.INIT_BATCH
    batch = _run(I, D, pairs, inits, gpu_device)
    for p, pair in enumerate(pairs):
        _assert_pair_is(batch, p, _run(I, D, [pair], inits[p:p + 1], gpu_device))
        assert batch[3][p].cpu().tolist()[::2] == [1, sum(C.BATCH_ITERATIONS)]
    assert not np.array_equal(_bits(batch[0][0]), _bits(batch[0][2]))  # the same pair under two inits


def test_a_pair_and_its_reverse(gpu_device):
    I, D = _scene(gpu_device)
    batch = _run(I, D, C.REVERSE_BATCH, None, gpu_device)
    for p, pair in enumerate(C.REVERSE_BATCH):
        _assert_pair_is(batch, p, _run(I, D, [pair], None, gpu_device))
        assert bool(batch[2][p])
    assert not np.array_equal(_bits(batch[0][0]), _bits(batch[0][1]))


def test_unnamed_nan_frames_change_nothing(gpu_device):
    I, D = _scene(gpu_device)
    I6, D6 = (_t(x, gpu_device) for x in C.unnamed_frames())
    clean = _run(I[:4], D[:4], C.UNNAMED_PAIRS, None, gpu_device)
    dirty = _run(I6, D6, C.UNNAMED_PAIRS, None, gpu_device)
    for x, y in zip(clean, dirty):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    assert bool(clean[2].all())
    lin_c = F.rgbd_odometry_linearize(I[:4], D[:4], C.SCENE_K, C.UNNAMED_PAIRS, None, 2, C.MDD)
    lin_d = F.rgbd_odometry_linearize(I6, D6, C.SCENE_K, C.UNNAMED_PAIRS, None, 2, C.MDD)
    for x, y in zip(lin_c, lin_d):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ conversion
@pytest.mark.parametrize("trunc", C.CONVERT_TRUNCS)
def test_conversion_values(gpu_device, trunc):
    c, d = C.convert_case()
    inten, dep = F.rgbd_from_color_and_depth(_t(c, gpu_device), _t(d.view(np.int16), gpu_device), C.CONVERT_SCALE, trunc)
    ri, rd = R.rgbd_from_color_and_depth(c, d, C.CONVERT_SCALE, trunc)
    assert np.array_equal(inten.cpu().numpy().view(np.int32), ri.view(np.int32))
    assert np.array_equal(dep.cpu().numpy().view(np.int32), rd.view(np.int32))
