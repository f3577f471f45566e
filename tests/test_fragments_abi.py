"""Host-side argument checks of the fragment entry points (include/pdsc.h f13,
f14).  Every check happens before any device work, so the calls below pass dummy
non-null pointers that are never dereferenced -- no GPU needed."""
import ctypes
import math

import pytest

from pointdsc_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
P = ctypes.c_void_p(256)  # a non-null "device pointer"; never read


def odo(lib, F=4, H=48, W=64, k=(50.0, 50.0, 31.5, 23.5), pairs=((0, 1), (1, 2)), mdd=0.07, mn=0.0, mx=4.0,
        iters=(20, 10, 5), intensity=P, depth=P, options=True, trans=P, info=P, status=P, ws=P, ws_bytes=None,
        null_pairs=False, linearize=False, level=0):
    n = len(pairs)
    src = (ctypes.c_int32 * max(n, 1))(*[p[0] for p in pairs])
    tgt = (ctypes.c_int32 * max(n, 1))(*[p[1] for p in pairs])
    opt = _lib.PdscRgbdOdometryOptions(mdd, mn, mx, (ctypes.c_int32 * 3)(*iters), 0)
    nb = lib.pdsc_rgbd_odometry_workspace_bytes(F, H, W, n) if ws_bytes is None else ws_bytes
    o = ctypes.byref(opt) if options else None
    s, t = (None, None) if null_pairs else (src, tgt)
    if linearize:
        return lib.pdsc_rgbd_odometry_linearize(intensity, depth, F, H, W, *k, s, t, n, None, o, level, None, trans,
                                                None, ws, nb, None)
    return lib.pdsc_rgbd_odometry(intensity, depth, F, H, W, *k, s, t, n, None, o, trans, info, status, ws, nb, None)


@pytest.mark.parametrize("lin", [False, True])
def test_odometry_errors(lin):
    lib = _lib.load()
    for name in ("intensity", "depth", "trans", "ws") + (() if lin else ("info", "status")):
        assert odo(lib, linearize=lin, **{name: None}) == ERR_ARG and b"null" in lib.pdsc_last_error(), name
    assert odo(lib, linearize=lin, options=False) == ERR_ARG and odo(lib, linearize=lin, null_pairs=True) == ERR_ARG
    for H, W in ((4, 64), (48, 4), (50, 64), (48, 66), (7, 7)):
        assert odo(lib, H=H, W=W, linearize=lin, ws_bytes=1 << 40) == ERR_ARG
        assert b"divisible by 4" in lib.pdsc_last_error()
    assert odo(lib, pairs=(), linearize=lin, ws_bytes=1 << 40) == ERR_ARG
    for pairs in (((0, 4),), ((-1, 0),), ((2, 2),), ((0, 1), (3, 7))):
        assert odo(lib, pairs=pairs, linearize=lin) == ERR_ARG and b"pair" in lib.pdsc_last_error()
    for bad in (0.0, -1.0, math.nan, math.inf):
        for i in range(4):
            k = [50.0, 50.0, 31.5, 23.5]
            k[i] = bad
            assert odo(lib, k=tuple(k), linearize=lin) == ERR_ARG and b"intrinsics" in lib.pdsc_last_error()
        assert odo(lib, mdd=bad, linearize=lin) == ERR_ARG and b"max_depth_diff" in lib.pdsc_last_error()
    assert odo(lib, mn=2.0, mx=1.0, linearize=lin) == ERR_ARG and b"min_depth" in lib.pdsc_last_error()
    assert odo(lib, iters=(20, -1, 5), linearize=lin) == ERR_ARG and b"iterations" in lib.pdsc_last_error()
    nb = lib.pdsc_rgbd_odometry_workspace_bytes(4, 48, 64, 2)
    assert odo(lib, linearize=lin, ws_bytes=nb - 1) == ERR_ARG and b"workspace too small" in lib.pdsc_last_error()
    if lin:
        for level in (-1, 3):
            assert odo(lib, linearize=True, level=level) == ERR_ARG and b"level" in lib.pdsc_last_error()
    assert odo(lib, F=70000, pairs=((0, 1),), linearize=lin, ws_bytes=1 << 40) == ERR_UNSUPPORTED
    assert odo(lib, H=8192, W=8196, linearize=lin, ws_bytes=1 << 50) == ERR_UNSUPPORTED and b"2^26" in lib.pdsc_last_error()


def pyr(lib, F=2, H=48, W=64, mn=0.0, mx=4.0, level=0, intensity=P, depth=P, outs=(P, P, P, P, P, P), ws=P,
        ws_bytes=None):
    nb = lib.pdsc_rgbd_odometry_workspace_bytes(F, H, W, 1) if ws_bytes is None else ws_bytes
    return lib.pdsc_rgbd_odometry_pyramid(intensity, depth, F, H, W, mn, mx, level, *outs, ws, nb, None)


def test_pyramid_errors():
    """The frame checks of pdsc_rgbd_odometry, message for message (one predicate), and no pair checks."""
    lib = _lib.load()
    for name in ("intensity", "depth", "ws"):
        assert pyr(lib, **{name: None}) == ERR_ARG and b"null" in lib.pdsc_last_error(), name
    assert pyr(lib, F=0, ws_bytes=1 << 40) == ERR_ARG and b"F=0 P=1" in lib.pdsc_last_error()
    for H, W in ((4, 64), (48, 4), (50, 64), (48, 66), (7, 7)):
        assert pyr(lib, H=H, W=W, ws_bytes=1 << 40) == ERR_ARG
        msg = lib.pdsc_last_error()
        assert odo(lib, H=H, W=W, ws_bytes=1 << 40) == ERR_ARG and lib.pdsc_last_error() == msg
    for mn, mx in ((2.0, 1.0), (-1.0, 4.0), (math.nan, 4.0), (0.0, math.inf), (1.0, 1.0)):
        assert pyr(lib, mn=mn, mx=mx) == ERR_ARG
        msg = lib.pdsc_last_error()
        assert odo(lib, mn=mn, mx=mx) == ERR_ARG and lib.pdsc_last_error() == msg and b"min_depth" in msg
    for level in (-1, 3):
        assert pyr(lib, level=level) == ERR_ARG and b"level" in lib.pdsc_last_error()
    nb = lib.pdsc_rgbd_odometry_workspace_bytes(2, 48, 64, 1)
    assert pyr(lib, ws_bytes=nb - 1) == ERR_ARG and b"workspace too small" in lib.pdsc_last_error()
    assert pyr(lib, F=70000, ws_bytes=1 << 40) == ERR_UNSUPPORTED
    assert pyr(lib, H=8192, W=8196, ws_bytes=1 << 50) == ERR_UNSUPPORTED and b"2^26" in lib.pdsc_last_error()
    assert pyr(lib, F=1, level=3) == ERR_ARG and b"level" in lib.pdsc_last_error()  # one frame is enough: no pair is needed


def test_odometry_workspace_is_monotone():
    q = _lib.load().pdsc_rgbd_odometry_workspace_bytes
    assert q(0, 48, 64, 1) == 0 and q(2, 48, 64, 0) == 0 and q(2, 6, 64, 1) == 0 and q(2, 48, 62, 1) == 0
    assert q(70000, 48, 64, 1) == 0 and q(2, 8192, 8196, 1) == 0 and q(2, 8192, 8192, 1) > 0
    base = q(2, 48, 64, 1)
    assert base >= 2 * 48 * 64 * 4 * 6 + 48 * 64 * 8
    assert q(3, 48, 64, 1) > base and q(2, 52, 64, 1) > base and q(2, 48, 68, 1) > base and q(2, 48, 64, 2) > base
    assert q(100, 480, 640, 99) > q(100, 480, 640, 50) > q(50, 480, 640, 50)


def test_conversion_errors():
    lib = _lib.load()
    f = lib.pdsc_rgbd_from_color_and_depth
    assert f(None, P, 1, 8, 8, 1000.0, 3.0, P, P, None) == ERR_ARG and b"null" in lib.pdsc_last_error()
    assert f(P, P, 1, 8, 8, 1000.0, 3.0, P, None, None) == ERR_ARG
    assert f(P, P, 0, 8, 8, 1000.0, 3.0, P, P, None) == ERR_ARG
    assert f(P, P, 1, 8, 8, 0.0, 3.0, P, P, None) == ERR_ARG and b"depth_scale" in lib.pdsc_last_error()
    assert f(P, P, 1, 8, 8, 1000.0, -1.0, P, P, None) == ERR_ARG


def integrate(lib, H=24, W=32, k=(30.0, 30.0, 15.5, 11.5), vl=0.01, trunc=0.04, mb=64, depth=P, colour=P, ext=P, ws=P,
              ws_bytes=None):
    nb = lib.pdsc_tsdf_workspace_bytes(mb) if ws_bytes is None else ws_bytes
    return lib.pdsc_tsdf_integrate(depth, colour, H, W, *k, ext, vl, trunc, mb, ws, nb, None)


def test_tsdf_errors():
    lib = _lib.load()
    for name in ("depth", "colour", "ext", "ws"):
        assert integrate(lib, **{name: None}) == ERR_ARG and b"null" in lib.pdsc_last_error(), name
    assert integrate(lib, H=0) == ERR_ARG and integrate(lib, W=0) == ERR_ARG
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert integrate(lib, k=(bad, 30.0, 15.5, 11.5)) == ERR_ARG and b"intrinsics" in lib.pdsc_last_error()
        assert integrate(lib, vl=bad) == ERR_ARG and b"voxel_length" in lib.pdsc_last_error()
        assert integrate(lib, trunc=bad) == ERR_ARG and b"sdf_trunc" in lib.pdsc_last_error()
    assert integrate(lib, mb=0, ws_bytes=1 << 40) == ERR_ARG and b"max_blocks" in lib.pdsc_last_error()
    assert integrate(lib, mb=(1 << 17) + 1, ws_bytes=1 << 50) == ERR_UNSUPPORTED
    nb = lib.pdsc_tsdf_workspace_bytes(64)
    assert integrate(lib, ws_bytes=nb - 1) == ERR_ARG and b"workspace too small" in lib.pdsc_last_error()
    n = ctypes.c_int64(0)
    assert lib.pdsc_tsdf_reset(64, None, nb, None) == ERR_ARG
    assert lib.pdsc_tsdf_reset(64, P, nb - 1, None) == ERR_ARG
    assert lib.pdsc_tsdf_count_surface_points(64, None, P, nb, None) == ERR_ARG
    assert lib.pdsc_tsdf_count_surface_points(64, ctypes.byref(n), P, nb - 1, None) == ERR_ARG
    assert lib.pdsc_tsdf_emit_surface_points(0.0, 64, P, P, 10, P, nb, None) == ERR_ARG
    assert lib.pdsc_tsdf_emit_surface_points(0.01, 64, P, P, 10, P, nb - 1, None) == ERR_ARG
    assert lib.pdsc_tsdf_emit_surface_points(0.01, 64, None, P, 10, P, nb, None) == ERR_ARG and b"null" in lib.pdsc_last_error()
    assert lib.pdsc_tsdf_emit_surface_points(0.01, 64, P, P, -1, P, nb, None) == ERR_ARG and b"capacity" in lib.pdsc_last_error()
    assert lib.pdsc_tsdf_read_blocks(64, -1, P, P, P, P, P, nb, None) == ERR_ARG
    assert lib.pdsc_tsdf_write_blocks(P, 0, P, P, P, 64, P, nb, None) == ERR_ARG
    assert lib.pdsc_tsdf_write_blocks(P, 2, None, P, P, 64, P, nb, None) == ERR_ARG


def test_tsdf_workspace_is_monotone():
    q = _lib.load().pdsc_tsdf_workspace_bytes
    assert q(0) == 0 and q(-1) == 0 and q((1 << 17) + 1) == 0 and q(1 << 17) > 0
    sizes = [q(m) for m in (1, 2, 63, 64, 65, 1000, 32768)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert q(1000) >= 1000 * 4096 * 5 * 4  # 80 KB of voxels per block
    assert ctypes.sizeof(_lib.PdscRgbdOdometryOptions) == 40 and ctypes.sizeof(_lib.PdscRgbdOdometryStatus) == 16
