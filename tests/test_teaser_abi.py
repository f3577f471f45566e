"""Host-side argument checks of the TEASER++ entry points (include/pdsc.h f9):
pdsc_gnc_tls_rotation, pdsc_tls_translation, pdsc_teaser_solve.  Every check
happens before any device work, so the calls below pass dummy non-null
pointers that are never dereferenced -- no GPU needed."""
import ctypes
import math

import pytest

from pointdsc_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
P = ctypes.c_void_p(256)  # a non-null "device pointer"; never read


def rot(lib, K=100, nb=0.3, factor=1.4, iters=100, thr=1e-16, a=P, b=P, R=P, w=P, inl=P, info=P):
    return lib.pdsc_gnc_tls_rotation(a, b, K, nb, factor, iters, thr, R, w, inl, info, None)


def tls(lib, K=100, nb=0.3, src=P, dst=P, t=P, inl=P, ws=P, ws_bytes=None):
    n = lib.pdsc_tls_translation_workspace_bytes(K) if ws_bytes is None else ws_bytes
    return lib.pdsc_tls_translation(src, dst, K, nb, t, inl, ws, n, None)


def solve(lib, N=100, nb=0.3, factor=1.4, iters=100, thr=1e-16, budget=0, src=P, tgt=P, result=P, t32=P, labels=P,
          ws=P, ws_bytes=None):
    n = lib.pdsc_teaser_solve_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return lib.pdsc_teaser_solve(src, tgt, N, nb, factor, iters, thr, budget, result, t32, labels, ws, n, None)


CALLS = {"rot": rot, "tls": tls, "solve": solve}


@pytest.mark.parametrize("which", sorted(CALLS))
def test_size_limits(which):
    lib = _lib.load()
    f = CALLS[which]
    kw = {} if which == "rot" else dict(ws_bytes=1 << 40)
    assert f(lib, 0, **kw) == ERR_ARG
    assert f(lib, -3, **kw) == ERR_ARG
    assert f(lib, 8193, **kw) == ERR_UNSUPPORTED
    assert b"8192" in lib.pdsc_last_error()
    assert lib.pdsc_tls_translation_workspace_bytes(0) == 0 and lib.pdsc_tls_translation_workspace_bytes(8193) == 0
    assert lib.pdsc_teaser_solve_workspace_bytes(0) == 0 and lib.pdsc_teaser_solve_workspace_bytes(8193) == 0


@pytest.mark.parametrize("which", sorted(CALLS))
@pytest.mark.parametrize("nb", [0.0, -0.3, math.nan, math.inf, -math.inf])
def test_noise_bound(which, nb):
    lib = _lib.load()
    assert CALLS[which](lib, nb=nb) == ERR_ARG
    assert b"noise_bound" in lib.pdsc_last_error()


@pytest.mark.parametrize("which", ["rot", "solve"])
def test_gnc_parameters(which):
    lib = _lib.load()
    f = CALLS[which]
    for factor in (1.0, 0.5, -1.4, math.nan, math.inf):
        assert f(lib, factor=factor) == ERR_ARG
        assert b"gnc_factor" in lib.pdsc_last_error()
    for iters in (0, -1):
        assert f(lib, iters=iters) == ERR_ARG
        assert b"max_iterations" in lib.pdsc_last_error()
    assert f(lib, thr=math.nan) == ERR_ARG


def test_solve_negative_budget():
    lib = _lib.load()
    assert solve(lib, budget=-1) == ERR_ARG
    assert b"node_budget" in lib.pdsc_last_error()


@pytest.mark.parametrize("which,name", [("rot", "a"), ("rot", "b"), ("rot", "R"), ("tls", "src"), ("tls", "dst"),
                                        ("tls", "t"), ("tls", "ws"), ("solve", "src"), ("solve", "tgt"),
                                        ("solve", "result"), ("solve", "ws")])
def test_null_pointers(which, name):
    lib = _lib.load()
    assert CALLS[which](lib, **{name: None}) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()


@pytest.mark.parametrize("N", [1, 64, 65, 300, 4096, 4097, 8192])
def test_workspace_one_byte_short(N):
    lib = _lib.load()
    for f, q in ((tls, lib.pdsc_tls_translation_workspace_bytes), (solve, lib.pdsc_teaser_solve_workspace_bytes)):
        nb = q(N)
        assert nb > 0
        assert f(lib, N, ws_bytes=nb - 1) == ERR_ARG
        assert b"workspace too small" in lib.pdsc_last_error()


def test_solve_workspace_holds_graph_and_clique():
    lib = _lib.load()
    prev = 0
    for N in (1, 2, 63, 64, 65, 1000, 4096, 4097, 8192):
        nb = lib.pdsc_teaser_solve_workspace_bytes(N)
        W = (N + 63) // 64
        assert nb >= prev
        assert nb >= lib.pdsc_max_clique_workspace_bytes(N) + N * W * 8 + N * 24 + 4 * N * 24
        prev = nb
    assert prev < 512 << 20


def test_struct_sizes():
    assert ctypes.sizeof(_lib.PdscGncInfo) == 24
    assert ctypes.sizeof(_lib.PdscTeaserResult) == 160
