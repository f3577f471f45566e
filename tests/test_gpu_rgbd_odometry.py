"""RGB-D odometry on the GPU (include/pdsc.h f13, pointdsc_amd/fragments.py) against
the numpy restatement tests/fragments_reference.py.

Bounds.  Correspondence maps: exact (fp64 geometry in the contract's operation
order, so the restatement and the kernel decide every accept and reject on the
same bits; test_depth_diff_threshold pins the `<=` itself on values that are exact
in fp32 after the filter).  Sums of one
linearisation: 1e-9 sum |terms| per entry (only the summation order differs: the
true gap is at most n 2^-53 sum |terms|).  Full run: 1e-6 per entry of trans when
the last correspondence counts agree, and rotation / translation errors against the
true motion at most 1.25 x the restatement's ("Fragments")."""
import numpy as np
import pytest
import torch

import fragments_reference as R
from pointdsc_amd import fragments as F

pytestmark = pytest.mark.gpu

MDD = 0.07
_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _edge_case(H, W):
    """Two frames with depth holes, points leaving the image and |dz| spread around
    max_depth_diff (offsets of MDD +- 1e-3 on the raw depth, which the filter and the
    motion then smear: accepts and rejects of every kind, none of them pinned to the
    threshold -- test_depth_diff_threshold does that; the tie has a test of its own)."""
    rng = np.random.RandomState(H * 1000 + W)
    K = (0.9 * W, 0.9 * W, W / 2 - 0.5, H / 2 - 0.5)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Ds = (1.5 + 0.3 * np.sin(u / 5.0) + 0.2 * np.cos(v / 4.0)).astype(np.float32)
    Dt = Ds.copy()
    Dt[1::3, ::2] += np.float32(MDD + 1e-3)
    Dt[::3, 1::2] -= np.float32(MDD - 1e-3)
    Ds[rng.rand(H, W) < 0.1] = 0.0            # holes
    Dt[rng.rand(H, W) < 0.1] = 0.0
    Is, It = rng.rand(H, W).astype(np.float32), rng.rand(H, W).astype(np.float32)
    T = R.exp6(np.array([0.01, -0.02, 0.015, 0.12, -0.05, 0.02]))  # the border columns leave the image
    return np.stack([Is, It]), np.stack([Ds, Dt]), K, T


@pytest.mark.parametrize("H,W", [(8, 16), (48, 64), (52, 68)])
@pytest.mark.parametrize("level", [0, 1])
def test_correspondence_map_and_sums(gpu_device, H, W, level):
    I, D, K, T = _edge_case(H, W)
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    a_s, a_t = R.intensity_scales(P[0][0], P[1][0], K, T, MDD)
    JtJ, Jtr, n, aJJ, aJr, corr = R.linearize(P[0][level], P[1][level], R.level_K(K, level), T, MDD, a_s, a_t)
    g_corr, g_JtJ, g_Jtr, g_n, g_sc = F.rgbd_odometry_linearize(_t(I, gpu_device), _t(D, gpu_device), K, [(0, 1)],
                                                                _t(T[None], gpu_device), level, MDD)
    assert n >= 1 and (corr < 0).sum() > 0  # 2 correspondences on the 8 x 4 level
    assert np.array_equal(g_corr[0].cpu().numpy().astype(np.int64), corr)
    assert int(g_n[0]) == n
    np.testing.assert_allclose(g_sc[0].cpu().numpy(), [a_s, a_t], rtol=1e-12)
    dJ, dr = np.abs(g_JtJ[0].cpu().numpy() - JtJ), np.abs(g_Jtr[0].cpu().numpy() - Jtr)
    print(f"{H}x{W} L{level}: n={n} max dJtJ/abs={np.max(dJ / np.maximum(aJJ, 1e-300)):.2e} "
          f"dJtr/abs={np.max(dr / np.maximum(aJr, 1e-300)):.2e}")
    assert np.all(dJ <= 1e-9 * aJJ) and np.all(dr <= 1e-9 * aJr)


def test_depth_diff_threshold(gpu_device):
    """|p.z - D_t| exactly at, one fp32 ulp-of-2^-20 above and below max_depth_diff,
    on the FILTERED level-0 depth: constant regions of values the 3x3 filter
    reproduces exactly (1, 1.0625 and 1.0625 -+ 2^-20: every product and sum of the
    filter is exact for them), T = identity, max_depth_diff = 0.0625.  Inside a
    region `<=` accepts the first and the last and rejects the middle one."""
    H, W, K, mdd, e = 16, 48, (40.0, 40.0, 23.5, 7.5), 0.0625, 2.0 ** -20
    Ds = np.ones((H, W), np.float32)
    Dt = np.empty((H, W), np.float32)
    Dt[:, :16], Dt[:, 16:32], Dt[:, 32:] = 1.0 + mdd, 1.0 + mdd + e, 1.0 + mdd - e
    I, D = np.random.RandomState(1).rand(2, H, W).astype(np.float32), np.stack([Ds, Dt])
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    inner = np.zeros((H, W), bool)
    for c0 in (0, 16, 32):
        inner[:, c0 + 2:c0 + 14] = True
    assert np.array_equal(P[1][0]["D"][inner], Dt[inner]) and np.array_equal(P[0][0]["D"], Ds)
    corr, _ = R.correspondences(P[0][0], P[1][0], K, np.eye(4), mdd)
    corr2 = corr.reshape(H, W)
    ident = np.arange(H * W).reshape(H, W)
    assert np.array_equal(corr2[:, 2:14], ident[:, 2:14])      # exactly at the threshold: accepted
    assert np.all(corr2[:, 18:30] == -1)                        # 2^-20 above: rejected
    assert np.array_equal(corr2[:, 34:46], ident[:, 34:46])    # 2^-20 below: accepted
    g_corr = F.rgbd_odometry_linearize(_t(I, gpu_device), _t(D, gpu_device), K, [(0, 1)], None, 0, mdd)[0][0]
    assert np.array_equal(g_corr.cpu().numpy(), corr)


def test_tie_lower_index_wins(gpu_device):
    """A fronto-parallel plane at depth 1 pushed to depth 2 by t_z = 1: p.z is equal
    for every pixel and the image shrinks by two, so several source pixels land on
    one target pixel with equal p.z.  The lowest source index must win."""
    H, W = 8, 16
    K = (8.0, 8.0, 7.5, 3.5)
    Ds = np.full((H, W), 1.0, np.float32)
    Dt = np.full((H, W), 2.0, np.float32)
    I = np.random.RandomState(3).rand(2, H, W).astype(np.float32)
    T = np.eye(4)
    T[2, 3] = 1.0
    D = np.stack([Ds, Dt])
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    corr, (px, py, pz) = R.correspondences(P[0][0], P[1][0], K, T, MDD)
    j = np.nonzero(corr >= 0)[0]
    assert len(np.unique(pz.astype(np.float32))) == 1 and len(j) < H * W / 2  # several sources per target, all tied
    g_corr = F.rgbd_odometry_linearize(_t(I, gpu_device), _t(D, gpu_device), K, [(0, 1)], _t(T[None], gpu_device), 0,
                                       MDD)[0][0].cpu().numpy()
    assert np.array_equal(g_corr, corr)
    # the lowest source index of each target pixel, from the definition
    fx, fy, cx, cy = K
    i = np.arange(H * W)
    ut = ((fx * px) / pz + cx + 0.5).astype(np.int64)
    vt = ((fy * py) / pz + cy + 0.5).astype(np.int64)
    for jj in j:
        assert corr[jj] == i[(vt * W + ut) == jj].min()


# ------------------------------------------------------------------ the rendered scene
SCENE_K, SCENE_H, SCENE_W = (140.0, 140.0, 79.5, 59.5), 120, 160
# the restatement's errors on this scene (tests/test_fragments_reference.py prints and checks them)
REF_ROT_ERR, REF_TRANS_ERR = 6.71e-4, 5.545e-3


def _scene():
    pose1 = R.small_motion()
    f0, f1 = R.render(np.eye(4), SCENE_K, SCENE_H, SCENE_W), R.render(pose1, SCENE_K, SCENE_H, SCENE_W)
    I, D = np.stack([f0[0], f1[0]]), np.stack([f0[1], f1[1]])
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    return I, D, np.linalg.inv(pose1), R.odometry_pair(P[0], P[1], SCENE_K, max_depth_diff=MDD)


def test_full_run_on_rendered_scene(gpu_device):
    I, D, T_true, (T_ref, info_ref, ok, n_ref, runs) = _once("scene", _scene)
    trans, info, success, status = F.rgbd_odometry(_t(I, gpu_device), _t(D, gpu_device), SCENE_K, [(0, 1)],
                                                   max_depth_diff=MDD, want_status=True)
    st = status[0].cpu().numpy()
    T = trans[0].cpu().numpy()
    rot, tr = R.pose_errors(T, T_true)
    r_rot, r_tr = R.pose_errors(T_ref, T_true)
    print(f"gpu: rot {rot:.3e} trans {tr:.3e}; restatement: rot {r_rot:.3e} trans {r_tr:.3e}; "
          f"n_corr {st[1]} vs {n_ref}; max |dT| {np.abs(T - T_ref).max():.2e}")
    assert ok and bool(success[0]) and st[2] == runs == 35
    if st[1] == n_ref:
        assert np.abs(T - T_ref).max() <= 1e-6
        np.testing.assert_allclose(info[0].cpu().numpy(), info_ref, rtol=1e-9, atol=1e-9)
    assert rot <= 1.25 * REF_ROT_ERR and tr <= 1.25 * REF_TRANS_ERR


def test_batch_independence(gpu_device):
    poses = [np.eye(4)]
    for k in range(3):
        poses.append(poses[-1] @ R.small_motion(0.003 * (k + 1), -0.004, 0.002 * k, (0.01, 0.004 * k, -0.006)))
    K, H, W = (56.0, 56.0, 31.5, 23.5), 48, 64
    fr = [R.render(p, K, H, W) for p in poses]
    I, D = _t(np.stack([f[0] for f in fr]), gpu_device), _t(np.stack([f[1] for f in fr]), gpu_device)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]
    alone = [F.rgbd_odometry(I, D, K, [p], max_depth_diff=MDD, want_status=True) for p in pairs]
    for P in (1, 2, 5):
        a = F.rgbd_odometry(I, D, K, pairs[:P], max_depth_diff=MDD, want_status=True)
        b = F.rgbd_odometry(I, D, K, pairs[:P], max_depth_diff=MDD, want_status=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        for p in range(P):
            assert np.array_equal(_bits(a[0][p]), _bits(alone[p][0][0]))
            assert np.array_equal(_bits(a[1][p]), _bits(alone[p][1][0]))
            assert torch.equal(a[3][p], alone[p][3][0]) and bool(a[2][p])


def test_degenerate_inputs(gpu_device):
    H, W, K = 16, 24, (20.0, 20.0, 11.5, 7.5)
    rng = np.random.RandomState(5)
    I = rng.rand(2, H, W).astype(np.float32)
    init = R.exp6(np.array([0.01, 0.02, -0.01, 0.03, 0.0, -0.02]))
    # all depth invalid
    tr, info, ok = F.rgbd_odometry(_t(I, gpu_device), torch.zeros((2, H, W), device=gpu_device), K, [(0, 1)],
                                   init=_t(init[None], gpu_device))
    assert not bool(ok[0]) and np.array_equal(tr[0].cpu().numpy(), init) and float(info.abs().max()) == 0.0
    # identical frames: the identity
    f = R.render(np.eye(4), (56.0, 56.0, 31.5, 23.5), 48, 64)
    I2, D2 = _t(np.stack([f[0], f[0]]), gpu_device), _t(np.stack([f[1], f[1]]), gpu_device)
    tr, info, ok = F.rgbd_odometry(I2, D2, (56.0, 56.0, 31.5, 23.5), [(0, 1)])
    assert bool(ok[0]) and np.abs(tr[0].cpu().numpy() - np.eye(4)).max() <= 1e-9
    # constant intensity, a fronto-parallel plane: J^T J has zero rows, exactly
    Ic, Dc = torch.full((2, H, W), 0.5, device=gpu_device), torch.full((2, H, W), 1.5, device=gpu_device)
    tr, info, ok = F.rgbd_odometry(Ic, Dc, K, [(0, 1)])
    assert not bool(ok[0]) and bool(torch.isfinite(tr).all())
    assert np.array_equal(tr[0].cpu().numpy(), np.eye(4))


def test_rgbd_conversion(gpu_device):
    rng = np.random.RandomState(9)
    c = rng.randint(0, 256, (2, 12, 20, 3)).astype(np.uint8)
    d = rng.randint(0, 5000, (2, 12, 20)).astype(np.uint16)
    inten, dep = F.rgbd_from_color_and_depth(_t(c, gpu_device), _t(d.view(np.int16), gpu_device), 1000.0, 3.0)
    ri, rd = R.rgbd_from_color_and_depth(c, d, 1000.0, 3.0)
    assert np.array_equal(inten.cpu().numpy(), ri) and np.array_equal(dep.cpu().numpy(), rd)
    assert (rd == 0).sum() > 0
