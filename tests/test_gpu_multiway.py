"""Multiway registration on the GPU (include/pdsc.h f11 / f12,
pointdsc_amd/multiway.py) against the fp64 restatement
tests/posegraph_reference.py.

Bounds.  Sums (the information matrix; e, F, H, b of one linearisation): (terms +
2) 2^-53 sum |terms| per entry, from the restatement's own term counts -- any
order of summing `terms` products stays inside it.  Indices, counts, edge_keep:
exact (the known-answer graphs keep every confidence 0.05 away from the
threshold; tests/test_posegraph_reference.py checks that on the CPU).  Optimised
poses: the GPU and the restatement may take a different number of LM steps, so
the bound is measured on the restatement: 10 x the larger of (the pose gap
between its Cholesky and its numpy.linalg.solve runs, the gap of either to the
fixed-l Gauss-Newton minimiser).  Measured: n = 3: 6.7e-8, n = 8: 1.5e-6, n = 33:
2.5e-5 (the Gauss-Newton gap; the solver gap is below 1e-15), so the bounds are
6.7e-7, 1.5e-5 and 2.5e-4 ("Multiway registration").  The ATE bound of
the n = 8 graph, 10 x the restatement's own ATE of 0.266 cm, is 2.66 cm."""
import numpy as np
import pytest
import torch

import icp_reference as ir
import posegraph_reference as P

pytestmark = pytest.mark.gpu

DIST = 0.05 * 1.4
KNOWN = {3: (1, 3, 1, 1), 8: (1, 8, 5, 4), 33: (1, 33, 40, 28)}
_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ----------------------------------------------------------------------- f11
def _info_case(ns):
    src, tgt, init, _ = ir.make_case(11, ns, ns * 3 // 2)
    return src, tgt, init


def _info_gpu(dev, src, tgt, T, r):
    from pointdsc_amd.multiway import information_matrix
    info, n, corr = information_matrix(_t(src, dev), _t(tgt, dev), r, None if T is None else _t(T, dev),
                                       want_correspondences=True)
    return info.cpu().numpy(), n, corr.cpu().numpy()


def _check_info(got, ref):
    info, n, corr = got
    assert n == ref["n_corr"] and np.array_equal(corr, ref["corr"])
    err, bound = np.abs(info - ref["info"]), (ref["cnt"] + 2) * P.U * ref["abs"]
    print("info: max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert _bits(np.array([info[5, 5]]))[0] == _bits(np.array([float(n)]))[0]


@pytest.mark.parametrize("ns", [1, 255, 256, 257, 513])
def test_information_matrix(ns, gpu_device):
    from pointdsc_amd.icp import registration_icp
    src, tgt, init = _info_case(ns)
    ref = _once(("info", ns), lambda: P.information_matrix(src, tgt, init, 0.1))
    a = _info_gpu(gpu_device, src, tgt, init, 0.1)
    _check_info(a, ref)
    assert ns == 1 or ref["n_corr"] > ns // 4
    icp = registration_icp(_t(src, gpu_device), _t(tgt, gpu_device), 0.1, _t(init, gpu_device), max_iteration=0)
    assert icp.n_corr == a[1]
    b = _info_gpu(gpu_device, src, tgt, init, 0.1)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_information_matrix_no_correspondence_and_identity(gpu_device):
    src, tgt, init = _info_case(257)
    far = init.copy()
    far[:3, 3] += 100.0
    info, n, corr = _info_gpu(gpu_device, src, tgt, far, 0.1)
    assert n == 0 and np.all(corr == -1) and np.array_equal(_bits(info), np.zeros((6, 6), np.int64))
    ref = P.information_matrix(tgt[:200], tgt, None, 0.05)  # trans NULL: the identity
    _check_info(_info_gpu(gpu_device, tgt[:200], tgt, None, 0.05), ref)
    assert ref["n_corr"] == 200


def test_information_matrix_exact_tie(gpu_device):
    """A source point exactly between two target points (coordinates exact in fp32 and
    in every fp64 difference): the lower target index wins."""
    tgt = np.array([[5.0, 5.0, 5.0], [1.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)
    src = np.array([[0.75, 0.0, 0.0], [0.25, 0.25, 0.0]], np.float32)
    ref = P.information_matrix(src, tgt, None, 0.5)
    got = _info_gpu(gpu_device, src, tgt, None, 0.5)
    assert list(got[2]) == [1, 2] == list(ref["corr"])
    _check_info(got, ref)


# ------------------------------------------------------------------ linearise
def _graph(key):
    return _once(("graph", key), lambda: P.make_graph(*key))


def _graph_tensors(g, dev):
    return (_t(g["src"], dev), _t(g["tgt"], dev), _t(g["trans"], dev), _t(g["info"], dev), _t(g["unc"], dev))


@pytest.mark.parametrize("key,ref_node", [((2, 2, 0, 0), 0), ((2, 3, 1, 0), 0), ((1, 33, 40, 28), 0),
                                          ((1, 33, 40, 28), 17), ((2, 3, 1, 0), 2)])
def test_linearize(key, ref_node, gpu_device):
    from pointdsc_amd.multiway import pose_graph_linearize
    g = _graph(key)
    E = len(g["src"])
    assert E == {2: 1, 3: 3, 33: 100}[key[1]]
    poses = P.perturbed(g["init"], 3)
    rng = np.random.RandomState(4)
    l = np.where(g["unc"] != 0, rng.rand(E), 1.0)
    mu = 7.5
    ref = _once(("lin", key, ref_node), lambda: P.linearize(poses, g, l, mu, ref_node, bounds=True))
    e, F, H, b = pose_graph_linearize(_t(poses, gpu_device), *_graph_tensors(g, gpu_device), _t(l, gpu_device), mu,
                                      ref_node)
    e, H, b = e.cpu().numpy(), H.cpu().numpy(), b.cpu().numpy()
    for name, got, want, ab, cnt in (("e", e, ref["e"], ref["e_abs"], ref["e_cnt"]),
                                     ("F", np.array(F), np.array(ref["F"]), ref["F_abs"], ref["F_cnt"]),
                                     ("H", H, ref["H"], ref["H_abs"], ref["H_cnt"]),
                                     ("b", b, ref["b"], ref["b_abs"], ref["b_cnt"])):
        err, bound = np.abs(got - want), (cnt + 2) * P.U * ab
        print(name, "max err", float(err.max()), "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), name
    assert np.array_equal(_bits(H), _bits(H.T.copy()))
    R = slice(6 * ref_node, 6 * ref_node + 6)
    want = np.zeros((6, H.shape[1]))
    want[:, R] = np.eye(6)
    assert np.array_equal(_bits(H[R] + 0.0), _bits(want)) and not b[R].any()


# ------------------------------------------------------------------- optimise
def _reference_runs(n):
    def run():
        g = _graph(KNOWN[n])
        a = P.optimize(g, g["init"], DIST)
        b = P.optimize(g, g["init"], DIST, solver="solve")
        gn = P.gauss_newton_fixed_l(g, a["poses"], a["confidence"] * a["keep"], a["mu"][1], a["keep"])
        gaps = (P.pose_gap(a["poses"], b["poses"]), P.pose_gap(a["poses"], gn), P.pose_gap(b["poses"], gn))
        return g, a, 10.0 * max(gaps), gaps
    return _once(("opt", n), run)


def _optimize_gpu(g, poses, dev, **kw):
    from pointdsc_amd.multiway import pose_graph_optimize
    p, conf, keep, res = pose_graph_optimize(_t(poses, dev), *_graph_tensors(g, dev), DIST, **kw)
    return p.cpu().numpy(), conf.cpu().numpy(), keep.cpu().numpy(), res


@pytest.mark.parametrize("n", [3, 8, 33])
def test_optimize_known_answer(n, gpu_device):
    g, ref, bound, gaps = _reference_runs(n)
    unc = g["unc"].astype(bool)
    assert np.abs(ref["confidence"][unc] - 0.25).min() > 0.05
    assert np.array_equal(ref["keep"][unc], ~g["false"][unc])
    poses, conf, keep, res = _optimize_gpu(g, g["init"], gpu_device)
    print("n", n, "reference gaps (solver, gn, gn)", gaps, "bound", bound, "gpu gap", P.pose_gap(poses, ref["poses"]),
          "iterations", list(res.iterations), ref["iterations"], "objective", list(res.objective), ref["objective"])
    assert res.solver_failed == 0
    assert np.array_equal(keep.astype(bool), ref["keep"]) and res.edges_kept == int(ref["keep"].sum())
    assert P.pose_gap(poses, ref["poses"]) <= bound
    assert np.all(conf[~unc] == 1.0) and np.all((conf[unc] > 0.25) == ref["keep"][unc])
    again = _optimize_gpu(g, g["init"], gpu_device)
    assert np.array_equal(_bits(poses), _bits(again[0])) and np.array_equal(_bits(conf), _bits(again[1]))
    assert np.array_equal(keep, again[2]) and list(res.objective) == list(again[3].objective)


def test_optimize_degenerate(gpu_device):
    from pointdsc_amd.multiway import pose_graph_optimize
    dev = gpu_device
    pose = ir.rigid([1, 1, 0], 20.0, [1, 2, 3])[None]
    none = dict(src=np.zeros(0, np.int32), tgt=np.zeros(0, np.int32), trans=np.zeros((0, 4, 4)),
                info=np.zeros((0, 6, 6)), unc=np.zeros(0, np.int32))
    p, conf, keep, res = _optimize_gpu(none, pose, dev)
    assert np.array_equal(_bits(p), _bits(pose)) and list(res.iterations) == [0, 0] and res.solver_failed == 0
    # no uncertain edge: mu = 0, plain LM to the min_residual stop
    g = _graph((5, 6, 0, 0))
    start = P.perturbed(g["init"], 0)
    ref = P.optimize(g, start, DIST)
    p, conf, keep, res = _optimize_gpu(g, start, dev)
    assert list(res.mu) == [0.0, 0.0] and np.all(conf == 1.0) and keep.all() and res.solver_failed == 0
    assert res.objective[1] < 1e-6 and P.pose_gap(p, g["gt"]) < 1e-2 * P.pose_gap(start, g["gt"])
    assert list(res.iterations) == ref["iterations"]
    bad = {k: v.copy() for k, v in g.items()}
    bad["tgt"][2] = bad["src"][2]
    with pytest.raises(RuntimeError, match="source == target"):
        pose_graph_optimize(_t(start, dev), *_graph_tensors(bad, dev), DIST)
    bad["tgt"][2] = 6
    with pytest.raises(RuntimeError, match="outside"):
        pose_graph_optimize(_t(start, dev), *_graph_tensors(bad, dev), DIST)


# --------------------------------------------------------------------- Python
def test_multi_scale_icp_recovers_offset(gpu_device):
    """The 513-point pair of icp_reference.make_case (init about 2 degrees and 3 cm
    off): held to tests/test_gpu_icp.py's bound for that case, both pose errors
    below the initial ones; the information matrix is the last scale's."""
    from pointdsc_amd.multiway import multi_scale_icp, local_refinement
    src, tgt, init, true = ir.make_case(0, 513, 600)
    T, info = multi_scale_icp(_t(src, gpu_device), _t(tgt, gpu_device), [0.05, 0.025, 0.0125], [50, 30, 14],
                              _t(init, gpu_device), max_distance=0.1)
    T = T.cpu().numpy()
    e0, e1 = ir.pose_error(init, true), ir.pose_error(T, true)
    print("pose error (deg, m): init", e0, "refined", e1)
    assert e1[0] < e0[0] and e1[1] < e0[1]
    info = info.cpu().numpy()
    assert info.shape == (6, 6) and info[5, 5] > 0 and np.array_equal(info, info.T)
    T2, _ = local_refinement(_t(src, gpu_device), _t(tgt, gpu_device), _t(T, gpu_device))
    assert T2.shape == (4, 4) and T2.dtype == torch.float64


def test_global_optimization_and_ate(gpu_device):
    from pointdsc_amd import multiway as M
    g, ref, _, _ = _reference_runs(8)
    bound = 10.0 * P.ate_cm(g["gt"], ref["poses"])
    graph = M.PoseGraph(gpu_device)
    for T in g["init"]:
        graph.add_node(_t(T, gpu_device))
    for k in range(len(g["src"])):
        graph.add_edge(int(g["src"][k]), int(g["tgt"][k]), _t(g["trans"][k], gpu_device), _t(g["info"][k], gpu_device),
                       bool(g["unc"][k]))
    out = M.global_optimization(graph, DIST)
    assert out.n_nodes == 8 and out.n_edges == int(ref["keep"].sum()) == out.result.edges_kept
    assert np.array_equal(out.edge_src.cpu().numpy(), g["src"][ref["keep"]])
    ate, err = M.absolute_trajectory_error(_t(g["gt"], gpu_device), out.nodes)
    print("ATE cm: gpu", ate, "restatement", bound / 10.0, "bound", bound)
    assert ate <= bound and err.shape == (8,)
    info = _t(g["info"][0], gpu_device)
    assert M.loop_edge_ok(info, 100, 150, _t(g["trans"][0], gpu_device)) == (float(info[5, 5]) / 100 >= 0.30)
    assert not M.loop_edge_ok(info, 1, 1, torch.eye(4, dtype=torch.float64, device=gpu_device))
