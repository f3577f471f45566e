"""tests/fragments_reference.py held to analytic truth, so that it can serve as the
reference of the GPU tests (no GPU, no library)."""
import numpy as np

import fragments_reference as R

K, H, W = (140.0, 140.0, 79.5, 59.5), 120, 160
_CACHE = {}


def _scene():
    if "s" not in _CACHE:
        pose1 = R.small_motion()
        f0, f1 = R.render(np.eye(4), K, H, W), R.render(pose1, K, H, W)
        _CACHE["s"] = (R.preprocess(f0[0], f0[1]), R.preprocess(f1[0], f1[1]), np.linalg.inv(pose1))
    return _CACHE["s"]


def test_tsdf_of_a_tilted_plane_is_the_stated_formula():
    n, d = R.PLANES[0]
    Kc, Hc, Wc = (30.0, 30.0, 15.5, 11.5), 24, 32
    _, depth, colour = R.render(np.eye(4), Kc, Hc, Wc, [R.PLANES[0]])
    vol = R.Volume(0.01, 0.04)
    assert vol.integrate(depth, colour, Kc, np.eye(4))
    checked = 0
    for key, (t, w, c) in vol.blocks.items():
        for vi in range(0, 4096, 37):
            p = ((np.array(key) * 16 + [vi & 15, (vi >> 4) & 15, vi >> 8]) + 0.5) * 0.01
            u, v = int(30.0 * p[0] / p[2] + 15.5 + 0.5), int(30.0 * p[1] / p[2] + 11.5 + 0.5)
            inside = p[2] > 0 and 30.0 * p[0] / p[2] + 16.0 > -1 and 30.0 * p[1] / p[2] + 12.0 > -1 and u < Wc and v < Hc
            if not inside or not depth[v, u] > 0:
                assert w[vi] == 0
                continue
            sdf = (float(depth[v, u]) - p[2]) * np.sqrt(((u - 15.5) / 30.0) ** 2 + ((v - 11.5) / 30.0) ** 2 + 1.0)
            if sdf > -0.04:
                assert w[vi] == 1 and t[vi] == np.float32(min(1.0, sdf / 0.04)) and np.array_equal(c[vi], colour[v, u])
                checked += 1
            else:
                assert w[vi] == 0
    assert checked > 500


def test_extracted_vertices_lie_on_a_synthetic_plane():
    """A volume whose tsdf is the exact signed distance of a plane (fp32): linear
    interpolation is exact for it, so every vertex is on the plane to fp32 rounding."""
    n, d, vl, trunc = np.array([0.3, -0.5, 0.81]), 0.05, 0.01, 0.04
    n = n / np.linalg.norm(n)
    vol = R.Volume(vl, trunc)
    vi = np.arange(4096)
    off = np.stack([vi & 15, (vi >> 4) & 15, vi >> 8], 1)
    for key in [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]:
        p = ((np.array(key) * 16 + off) + 0.5) * vl
        sd = (d - p @ n) / trunc
        w = (np.abs(sd) < 1.0).astype(np.float32)
        vol.blocks[key] = [np.clip(sd, -1, 1).astype(np.float32), w, np.full((4096, 3), 100.0, np.float32)]
    pts, cols, fsum = vol.extract()
    assert len(pts) > 500
    assert np.abs(pts @ n - d).max() <= 8 * np.finfo(np.float32).eps * 1.0 * trunc + 1e-12
    assert np.abs(cols - 100.0 / 255.0).max() <= 1e-12
    del vol.blocks[(0, 0, 0)]
    assert 0 < len(vol.extract()[0]) < len(pts)


def test_jacobian_rows_equal_central_differences():
    Ps, Pt, _ = _scene()
    T = R.small_motion(0.002, -0.003, 0.001, (0.004, -0.002, 0.003))
    # a smooth analytic target (no pixel lookups): r(T) is evaluated with the SAME correspondences and
    # target values linearised by the rows' own gradients, so the rows must match d r / d xi of
    # r_D = D_t(pi(p)) - p.z with D_t taken locally linear: checked on the geometric part
    JI, JD, rI, rD, corr = R.rows(Ps[0], Pt[0], K, T, 0.07)
    j = np.nonzero(corr >= 0)[0]
    i = corr[j]
    fx, fy, cx, cy = K
    d = Ps[0]["D"].reshape(-1)[i].astype(np.float64)
    X = np.stack([((i % W) - cx) * d / fx, ((i // W) - cy) * d / fy, d, np.ones_like(d)], 0)
    gd = [np.nan_to_num(Pt[0][k].reshape(-1)[j].astype(np.float64)) * R.SOBEL_SCALE for k in ("Ddx", "Ddy")]
    gi = [np.nan_to_num(Pt[0][k].reshape(-1)[j].astype(np.float64)) * R.SOBEL_SCALE for k in ("Idx", "Idy")]

    def res(Tm):  # the residuals with the target images linear around the projected point
        p = Tm @ X
        u, v = fx * p[0] / p[2], fy * p[1] / p[2]
        return (np.sqrt(1 - R.LAMBDA_DEP) * (gi[0] * u + gi[1] * v),
                np.sqrt(R.LAMBDA_DEP) * (gd[0] * u + gd[1] * v - p[2]))

    eps = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = eps
        (ip, dp), (im, dm) = res(R.exp6(e) @ T), res(R.exp6(-e) @ T)
        assert np.abs((ip - im) / (2 * eps) - JI[:, k]).max() <= 1e-6 * max(1.0, np.abs(JI[:, k]).max())
        assert np.abs((dp - dm) / (2 * eps) - JD[:, k]).max() <= 1e-6 * max(1.0, np.abs(JD[:, k]).max())


def test_odometry_recovers_a_known_small_motion():
    Ps, Pt, T_true = _scene()
    T, info, ok, n, runs = R.odometry_pair(Ps, Pt, K)
    rot, tr = R.pose_errors(T, T_true)
    rot0, tr0 = R.pose_errors(np.eye(4), T_true)
    print(f"restatement odometry error: rot {rot:.4e} rad, trans {tr:.4e} m (motion: {rot0:.3e} rad, {tr0:.3e} m)")
    assert ok and runs == 35 and n > 10000
    assert rot < 0.1 * rot0 and tr < 0.35 * tr0
    # the figures DESIGN.md "Fragments" and tests/test_gpu_rgbd_odometry.py record
    assert abs(rot - 6.71e-4) < 1e-5 and abs(tr - 5.545e-3) < 1e-5
    assert np.allclose(info, info.T) and info[5, 5] > 10000
