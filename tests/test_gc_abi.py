"""Host-side argument checks of the GC-RANSAC entry points (include/pdsc.h f10):
pdsc_gc_grid, pdsc_gc_label, pdsc_gc_ransac.  Every check happens before any
device work, so the calls below pass dummy non-null pointers that are never
dereferenced -- no GPU needed."""
import ctypes
import math

import pytest

from pointdsc_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
P = ctypes.c_void_p(256)  # a non-null "device pointer"; never read
MAX_ROWS = 262144


def grid(lib, N=100, G=20, src=P, tgt=P, order=P, cell_start=P, cell_of=P, n_cells=P, ws=P, ws_bytes=None):
    n = lib.pdsc_gc_grid_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return lib.pdsc_gc_grid(src, tgt, N, G, order, cell_start, cell_of, n_cells, ws, n, None)


def label(lib, N=100, eps=0.1, lam=0.1, pose=P, src=P, tgt=P, order=P, cell_start=P, n_cells=P, labels=P, count=P,
          ws=P, ws_bytes=None):
    n = lib.pdsc_gc_label_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return lib.pdsc_gc_label(pose, src, tgt, N, order, cell_start, n_cells, eps, lam, labels, count, None, ws, n, None)


def solve(lib, N=100, eps=0.1, lam=0.1, G=20, H=1000, conf=0.99, lo=1, src=P, tgt=P, ws=P, ws_bytes=None):
    n = lib.pdsc_gc_ransac_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return lib.pdsc_gc_ransac(src, tgt, N, eps, lam, G, H, conf, 0, lo, P, P, P, None, ws, n, None)


CALLS = {"grid": grid, "label": label, "solve": solve}


def test_round_and_bounds():
    lib = _lib.load()
    assert lib.pdsc_gc_ransac_round() > 0 and lib.pdsc_gc_ransac_round() == lib.pdsc_ransac_round()
    assert (lib.pdsc_gc_cell_bound(0), lib.pdsc_gc_cell_bound(1), lib.pdsc_gc_cell_bound(2)) == (64, 1024, 0)


@pytest.mark.parametrize("which", sorted(CALLS))
def test_size_limits(which):
    lib = _lib.load()
    f = CALLS[which]
    assert f(lib, 0, ws_bytes=1 << 40) == ERR_ARG
    assert f(lib, -3, ws_bytes=1 << 40) == ERR_ARG
    assert f(lib, MAX_ROWS + 1, ws_bytes=1 << 40) == ERR_UNSUPPORTED
    assert b"262144" in lib.pdsc_last_error()
    for q in (lib.pdsc_gc_grid_workspace_bytes, lib.pdsc_gc_label_workspace_bytes, lib.pdsc_gc_ransac_workspace_bytes):
        assert q(0) == 0 and q(MAX_ROWS + 1) == 0 and q(MAX_ROWS) > 0


def test_solver_needs_three_rows():
    lib = _lib.load()
    assert solve(lib, 2, ws_bytes=1 << 40) == ERR_ARG
    assert lib.pdsc_gc_ransac_workspace_bytes(2) == 0 and lib.pdsc_gc_ransac_workspace_bytes(3) > 0


@pytest.mark.parametrize("which", ["grid", "solve"])
@pytest.mark.parametrize("G", [0, -1, 1025])
def test_grid_size(which, G):
    lib = _lib.load()
    assert CALLS[which](lib, G=G) == ERR_ARG
    assert b"neighborhood_size" in lib.pdsc_last_error()


@pytest.mark.parametrize("which", ["label", "solve"])
def test_model_parameters(which):
    lib = _lib.load()
    f = CALLS[which]
    for eps in (0.0, -0.1, math.nan, math.inf):
        assert f(lib, eps=eps) == ERR_ARG
        assert b"threshold" in lib.pdsc_last_error()
    for lam in (-0.01, 1.01, math.nan, math.inf):
        assert f(lib, lam=lam) == ERR_ARG
        assert b"spatial_coherence_weight" in lib.pdsc_last_error()


def test_solver_parameters():
    lib = _lib.load()
    for H in (0, -5):
        assert solve(lib, H=H) == ERR_ARG
        assert b"max_iteration" in lib.pdsc_last_error()
    for conf in (0.0, -0.5, 1.5, math.nan):
        assert solve(lib, conf=conf) == ERR_ARG
        assert b"confidence" in lib.pdsc_last_error()
    # local optimisation off: lambda and G are still checked
    assert solve(lib, lam=2.0, lo=0) == ERR_ARG and solve(lib, G=0, lo=0) == ERR_ARG


@pytest.mark.parametrize("which,name", [("grid", "src"), ("grid", "tgt"), ("grid", "order"), ("grid", "cell_start"),
                                        ("grid", "cell_of"), ("grid", "n_cells"), ("grid", "ws"), ("label", "pose"),
                                        ("label", "src"), ("label", "tgt"), ("label", "order"),
                                        ("label", "cell_start"), ("label", "n_cells"), ("label", "labels"),
                                        ("label", "count"), ("label", "ws"), ("solve", "src"), ("solve", "tgt"),
                                        ("solve", "ws")])
def test_null_pointers(which, name):
    lib = _lib.load()
    assert CALLS[which](lib, **{name: None}) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()


@pytest.mark.parametrize("N", [3, 64, 65, 1024, 1025, 4097, MAX_ROWS])
def test_workspace_one_byte_short(N):
    lib = _lib.load()
    for f, q in ((grid, lib.pdsc_gc_grid_workspace_bytes), (label, lib.pdsc_gc_label_workspace_bytes),
                 (solve, lib.pdsc_gc_ransac_workspace_bytes)):
        nb = q(N)
        assert nb > 0
        assert f(lib, N, ws_bytes=nb - 1) == ERR_ARG
        assert b"workspace too small" in lib.pdsc_last_error()


def test_solver_workspace_holds_its_parts():
    lib = _lib.load()
    prev = 0
    for N in (3, 63, 64, 65, 1000, 4097, MAX_ROWS):
        nb = lib.pdsc_gc_ransac_workspace_bytes(N)
        assert nb >= prev
        assert nb >= (lib.pdsc_ransac_workspace_bytes(N) + lib.pdsc_gc_grid_workspace_bytes(N)
                      + lib.pdsc_gc_label_workspace_bytes(N) + 4 * N * 4)
        prev = nb


def test_struct_sizes():
    assert ctypes.sizeof(_lib.PdscGcRansacResult) == 160
    assert ctypes.sizeof(_lib.PdscGcLabelDebug) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.PdscGcRansacDebug) == 4 * ctypes.sizeof(ctypes.c_void_p)
