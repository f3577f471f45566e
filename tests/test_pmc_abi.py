"""Host-side argument checks of the PMC entry points (include/pdsc.h f8):
pdsc_consistency_graph, pdsc_max_clique, pdsc_greedy_clique.  Every check
happens before any device work, so the calls below pass dummy non-null
pointers that are never dereferenced -- no GPU needed."""
import ctypes
import math

import pytest

from pointdsc_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
SQUARED, LENGTH = _lib.EDGE_MODES["squared"], _lib.EDGE_MODES["length"]
P = ctypes.c_void_p(256)  # a non-null "device pointer"; never read


def graph(lib, N, thr=0.1, mode=SQUARED, corr=P, adj=P, degree=P):
    return lib.pdsc_consistency_graph(corr, N, thr, mode, adj, degree, None)


def clique(lib, N, budget=0, adj=P, members=P, result=P, labels=P, ws=P, ws_bytes=None):
    nb = lib.pdsc_max_clique_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return lib.pdsc_max_clique(adj, N, budget, members, result, labels, ws, nb, None)


def test_graph_size_limits():
    lib = _lib.load()
    assert graph(lib, 0) == ERR_ARG
    assert graph(lib, -5) == ERR_ARG
    assert graph(lib, 8193) == ERR_UNSUPPORTED
    assert b"8192" in lib.pdsc_last_error()


@pytest.mark.parametrize("thr", [0.0, -0.1, math.nan, math.inf, -math.inf])
def test_graph_threshold(thr):
    lib = _lib.load()
    for mode in (SQUARED, LENGTH):
        assert graph(lib, 100, thr=thr, mode=mode) == ERR_ARG
        assert b"threshold" in lib.pdsc_last_error()


@pytest.mark.parametrize("mode", [-1, 2, 7])
def test_graph_unknown_mode(mode):
    lib = _lib.load()
    assert graph(lib, 100, mode=mode) == ERR_ARG
    assert b"mode" in lib.pdsc_last_error()


def test_graph_null_pointers():
    lib = _lib.load()
    assert graph(lib, 100, corr=None) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()
    assert graph(lib, 100, adj=None) == ERR_ARG


def test_clique_size_limits():
    lib = _lib.load()
    assert clique(lib, 0, ws_bytes=1 << 20) == ERR_ARG
    assert clique(lib, 8193, ws_bytes=1 << 40) == ERR_UNSUPPORTED
    assert lib.pdsc_max_clique_workspace_bytes(0) == 0
    assert lib.pdsc_max_clique_workspace_bytes(8193) == 0
    assert lib.pdsc_greedy_clique(P, 0, P, P, P, P, 1 << 20, None) == ERR_ARG
    assert lib.pdsc_greedy_clique(P, 8193, P, P, P, P, 1 << 40, None) == ERR_UNSUPPORTED


def test_clique_negative_budget():
    lib = _lib.load()
    assert clique(lib, 100, budget=-1) == ERR_ARG
    assert b"node_budget" in lib.pdsc_last_error()
    assert clique(lib, 100, budget=-(1 << 40)) == ERR_ARG


@pytest.mark.parametrize("which", ["adj", "members", "result", "ws"])
def test_clique_null_pointers(which):
    lib = _lib.load()
    assert clique(lib, 100, **{which: None}) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()
    args = dict(adj=P, members=P, result=P, ws=P)
    args[which] = None
    nb = lib.pdsc_max_clique_workspace_bytes(100)
    assert lib.pdsc_greedy_clique(args["adj"], 100, args["members"], args["result"], P, args["ws"], nb, None) == ERR_ARG


@pytest.mark.parametrize("N", [1, 64, 65, 300, 4096, 4097, 8192])
def test_clique_workspace_one_byte_short(N):
    lib = _lib.load()
    nb = lib.pdsc_max_clique_workspace_bytes(N)
    assert nb > 0
    assert clique(lib, N, ws_bytes=nb - 1) == ERR_ARG
    assert b"workspace too small" in lib.pdsc_last_error()
    assert lib.pdsc_greedy_clique(P, N, P, P, P, P, nb - 1, None) == ERR_ARG


def test_clique_workspace_monotone_and_bounded():
    """The query grows with N (so a workspace sized for the largest N of a run
    serves every smaller one), holds at least the relabelled graph and one
    stack of pdsc_max_clique_depth() levels, and stays under 256 MiB."""
    lib = _lib.load()
    depth = lib.pdsc_max_clique_depth()
    assert depth >= 256
    assert lib.pdsc_max_clique_default_budget() >= 1
    prev = 0
    for N in range(1, 8193):
        nb = lib.pdsc_max_clique_workspace_bytes(N)
        W = (N + 63) // 64
        assert nb >= prev, N
        assert nb >= N * W * 8 + min(N, depth) * W * 8, N
        prev = nb
    assert prev < 256 << 20
