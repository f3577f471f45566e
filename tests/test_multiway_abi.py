"""Host-side argument checks of the multiway entry points (include/pdsc.h f11,
f12): pdsc_information_matrix, pdsc_pose_graph_optimize,
pdsc_pose_graph_linearize.  Every check happens before any device work, so the
calls below pass dummy non-null pointers that are never dereferenced -- no GPU
needed."""
import ctypes
import math

import pytest

from pointdsc_amd import _lib

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
P = ctypes.c_void_p(256)  # a non-null "device pointer"; never read
MAX_N, MAX_E = 256, 32768


def info(lib, Ns=100, Nt=150, r=0.07, source=P, target=P, result=P, ws=P, ws_bytes=None):
    n = lib.pdsc_information_matrix_workspace_bytes(Ns, Nt) if ws_bytes is None else ws_bytes
    return lib.pdsc_information_matrix(source, Ns, target, Nt, None, r, result, None, ws, n, None)


def optimize(lib, n=8, E=16, ref=0, dist=0.07, pref=20.0, prune=0.25, poses=P, edge_src=P, edge_tgt=P, edge_trans=P,
             edge_info=P, edge_uncertain=P, options=True, criteria=None, confidence=P, edge_keep=P, result=P, ws=P,
             ws_bytes=None):
    nb = lib.pdsc_pose_graph_workspace_bytes(n, E) if ws_bytes is None else ws_bytes
    opt = _lib.PdscPoseGraphOptions(dist, prune, pref, ref, 0)
    return lib.pdsc_pose_graph_optimize(poses, n, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain, E,
                                        ctypes.byref(opt) if options else None,
                                        ctypes.byref(criteria) if criteria is not None else None, confidence,
                                        edge_keep, result, ws, nb, None)


def linearize(lib, n=8, E=16, ref=0, mu=1.0, poses=P, edge_src=P, edge_tgt=P, edge_trans=P, edge_info=P,
              edge_uncertain=P, residual=P, objective=P, H=P, b=P, ws=P, ws_bytes=None):
    nb = lib.pdsc_pose_graph_workspace_bytes(n, E) if ws_bytes is None else ws_bytes
    return lib.pdsc_pose_graph_linearize(poses, n, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain, E, None,
                                         mu, ref, residual, objective, H, b, ws, nb, None)


GRAPH = {"optimize": optimize, "linearize": linearize}


def test_information_matrix_sizes_and_radius():
    lib = _lib.load()
    q = lib.pdsc_information_matrix_workspace_bytes
    assert q(0, 10) == 0 and q(10, 0) == 0 and q(1, 1) > 0 and q(5000, 7500) > q(1000, 1500)
    for ns, nt in ((0, 10), (10, 0), (-1, 10)):
        assert info(lib, ns, nt, ws_bytes=1 << 30) == ERR_ARG
        assert b"need >= 1" in lib.pdsc_last_error()
    for r in (0.0, -0.1, math.nan, math.inf):
        assert info(lib, r=r) == ERR_ARG
        assert b"max_distance" in lib.pdsc_last_error()


@pytest.mark.parametrize("name", ["source", "target", "result", "ws"])
def test_information_matrix_null_pointers(name):
    lib = _lib.load()
    assert info(lib, **{name: None}) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()


@pytest.mark.parametrize("Ns,Nt", [(1, 1), (255, 383), (256, 384), (257, 385), (5000, 7500)])
def test_information_matrix_workspace_one_byte_short(Ns, Nt):
    lib = _lib.load()
    nb = lib.pdsc_information_matrix_workspace_bytes(Ns, Nt)
    assert info(lib, Ns, Nt, ws_bytes=nb - 1) == ERR_ARG
    assert b"workspace too small" in lib.pdsc_last_error()
    # the grid of the target and 10 doubles per 256-point source chunk
    assert nb >= 80 * ((Ns + 255) // 256)


@pytest.mark.parametrize("which", sorted(GRAPH))
def test_graph_size_limits(which):
    lib = _lib.load()
    f = GRAPH[which]
    for n, E in ((0, 1), (-1, 1), (4, -1)):
        assert f(lib, n, E, ws_bytes=1 << 40) == ERR_ARG
        assert b"need n >= 1" in lib.pdsc_last_error()
    for n, E in ((MAX_N + 1, 10), (10, MAX_E + 1)):
        assert f(lib, n, E, ws_bytes=1 << 40) == ERR_UNSUPPORTED
        assert b"256" in lib.pdsc_last_error() and b"32768" in lib.pdsc_last_error()
    q = lib.pdsc_pose_graph_workspace_bytes
    assert q(0, 0) == 0 and q(MAX_N + 1, 1) == 0 and q(1, MAX_E + 1) == 0 and q(1, -1) == 0
    assert q(1, 0) > 0 and q(MAX_N, MAX_E) >= 2 * 8 * (6 * MAX_N) ** 2


@pytest.mark.parametrize("which", sorted(GRAPH))
@pytest.mark.parametrize("ref", [-1, 8, 100])
def test_reference_node_range(which, ref):
    lib = _lib.load()
    assert GRAPH[which](lib, ref=ref) == ERR_ARG
    assert b"reference_node" in lib.pdsc_last_error()
    assert GRAPH[which](lib, n=101, ref=100, ws_bytes=0) == ERR_ARG  # in range: the next check speaks
    assert b"workspace too small" in lib.pdsc_last_error()


@pytest.mark.parametrize("which,name", [(w, p) for w in sorted(GRAPH) for p in
                                        ("poses", "edge_src", "edge_tgt", "edge_trans", "edge_info", "edge_uncertain",
                                         "ws")]
                         + [("optimize", p) for p in ("confidence", "edge_keep", "result")]
                         + [("linearize", p) for p in ("residual", "objective", "H", "b")])
def test_graph_null_pointers(which, name):
    lib = _lib.load()
    assert GRAPH[which](lib, **{name: None}) == ERR_ARG
    assert b"null" in lib.pdsc_last_error()


def test_edge_arrays_may_be_null_without_edges():
    lib = _lib.load()
    none = dict(edge_src=None, edge_tgt=None, edge_trans=None, edge_info=None, edge_uncertain=None)
    # the argument checks pass: the next one (the workspace) speaks
    assert optimize(lib, 1, 0, confidence=None, edge_keep=None, ws_bytes=0, **none) == ERR_ARG
    assert b"workspace too small" in lib.pdsc_last_error()
    assert linearize(lib, 1, 0, residual=None, ws_bytes=0, **none) == ERR_ARG
    assert b"workspace too small" in lib.pdsc_last_error()


def test_optimize_options():
    lib = _lib.load()
    assert optimize(lib, options=False) == ERR_ARG and b"options" in lib.pdsc_last_error()
    for d in (0.0, -1.0, math.nan, math.inf):
        assert optimize(lib, dist=d) == ERR_ARG
        assert b"max_correspondence_distance" in lib.pdsc_last_error()
    for p in (-1.0, math.nan, math.inf):
        assert optimize(lib, pref=p) == ERR_ARG
        assert b"preference_loop_closure" in lib.pdsc_last_error()
    assert optimize(lib, prune=math.nan) == ERR_ARG and b"edge_prune_threshold" in lib.pdsc_last_error()
    bad = _lib.PdscPoseGraphCriteria(-1, 20, 1e-6, 1e-6, 1e-6, 1e-6)
    assert optimize(lib, criteria=bad) == ERR_ARG and b"max_iteration" in lib.pdsc_last_error()
    for mu in (-1.0, math.nan, math.inf):
        assert linearize(lib, mu=mu) == ERR_ARG and b"mu" in lib.pdsc_last_error()


@pytest.mark.parametrize("n,E", [(1, 0), (2, 1), (33, 100), (60, 900), (MAX_N, MAX_E)])
def test_graph_workspace_one_byte_short(n, E):
    lib = _lib.load()
    nb = lib.pdsc_pose_graph_workspace_bytes(n, E)
    assert nb > 0
    for f in (optimize, linearize):
        assert f(lib, n, E, ws_bytes=nb - 1) == ERR_ARG
        assert b"workspace too small" in lib.pdsc_last_error()


def test_struct_sizes_and_defaults():
    assert ctypes.sizeof(_lib.PdscInformationResult) == 36 * 8 + 8
    assert ctypes.sizeof(_lib.PdscPoseGraphOptions) == 32
    assert ctypes.sizeof(_lib.PdscPoseGraphCriteria) == 40
    assert ctypes.sizeof(_lib.PdscPoseGraphResult) == 48
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "pdsc.h")).read()
    got = dict(re.findall(r"#define PDSC_PG_(\w+) (\S+)", src))
    assert got == {"MAX_ITERATION": "100", "MAX_ITERATION_LM": "20", "MIN_RELATIVE_INCREMENT": "1e-6",
                   "MIN_RELATIVE_RESIDUAL_INCREMENT": "1e-6", "MIN_RIGHT_TERM": "1e-6", "MIN_RESIDUAL": "1e-6"}
