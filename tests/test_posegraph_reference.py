"""The fp64 restatement of tests/posegraph_reference.py on the CPU: its own
properties, before tests/test_gpu_multiway.py holds the kernels to it, and the
preconditions of the GPU's known-answer graphs (a seed that prunes the wrong
edge, or lands near the threshold, fails here and not on the GPU)."""
import numpy as np
import pytest

import icp_reference as ir
import posegraph_reference as P

# (seed, n, n_loops, n_false) of tests/test_gpu_multiway.py
KNOWN = [(1, 3, 1, 1), (1, 8, 5, 4), (1, 33, 40, 28)]
DIST = 0.05 * 1.4


def _consistent(seed, n=6):
    """A graph every edge of which agrees with the poses exactly (up to rounding)."""
    g = P.make_graph(seed, n, 4, 0, rot_noise_deg=0.0, trans_noise=0.0)
    return g, g["gt"]


def test_information_matrix_is_gtg_of_the_correspondences():
    src, tgt, init, _ = ir.make_case(3, 257, 385)
    r = P.information_matrix(src, tgt, init, 0.1)
    c = r["corr"]
    assert r["n_corr"] == int((c >= 0).sum()) > 50 and r["info"][5, 5] == r["n_corr"]
    t = tgt.astype(np.float64)[c[c >= 0]]
    assert np.allclose(r["info"][3:, 3:], r["n_corr"] * np.eye(3), rtol=0, atol=0)
    assert np.allclose(r["info"][0, 0], (t[:, 1] ** 2 + t[:, 2] ** 2).sum(), rtol=1e-13)
    assert np.allclose(r["info"], r["info"].T, rtol=0, atol=0)
    far = ir.rigid([0, 0, 1], 0.0, [100.0, 0, 0])
    z = P.information_matrix(src, tgt, far, 0.1)
    assert z["n_corr"] == 0 and not z["info"].any()


def test_residual_vanishes_at_consistent_poses():
    g, poses = _consistent(0)
    lz = P.linearize(poses, g)
    assert np.abs(lz["e"]).max() < 1e-14 and lz["F"] < 1e-24


def test_jacobians_match_finite_differences_at_consistent_poses():
    """Js and Jt are the derivatives of e under pose <- Exp(d) pose ONLY where e = 0:
    lin6 and vec6 agree to first order at the identity and nowhere else, so the
    comparison is made at poses consistent with every edge.  Central differences
    with step h: the truncation term is h^2 / 6 times the third derivative of
    entries of Exp, which are products of sines and cosines of h with unit-scale
    poses, so at most ~ 8 h^2 with the translation arms of 2 m; the rounding term
    is u |e-scale| / h with e's terms of size <= 4 (|X^-1| |Tt^-1| |Ts| entries).
    h = (3 u 4 / 16)^(1/3) ~ 4.4e-6 balances them; the bound is their sum at that h
    with a factor 4 for the 6-term sums."""
    g, poses = _consistent(0)
    lz = P.linearize(poses, g)
    u = 2.0 ** -53
    h = (3 * u * 4 / 16) ** (1.0 / 3.0)
    bound = 4 * (8 * h * h + 4 * u / h)
    assert bound < 1e-8  # sanity: the derived bound is about 1e-9
    for k in (0, 3, len(g["src"]) - 1):
        s, t = int(g["src"][k]), int(g["tgt"][k])
        for node, sign in ((s, 1.0), (t, -1.0)):
            fd = np.zeros((6, 6))
            for i in range(6):
                d = np.zeros(6)
                d[i] = h
                pp, pm = poses.copy(), poses.copy()
                pp[node], pm[node] = P.mul(P.exp6(d), poses[node]), P.mul(P.exp6(-d), poses[node])
                ep = P.edge_residual(pp[s], pp[t], g["trans"][k])[0]
                em = P.edge_residual(pm[s], pm[t], g["trans"][k])[0]
                fd[:, i] = (ep - em) / (2 * h)
            assert np.abs(fd - sign * lz["J"][k]).max() <= bound, (k, node)


def test_line_process_minimises_objective_at_fixed_poses():
    g = P.make_graph(2, 8, 5, 4)
    poses = g["init"]
    q = P.linearize(poses, g)["q"]
    mu = 20.0 * DIST ** 2 * g["info"][g["unc"] != 0][:, 5, 5].mean()
    l = P.line_process(q, g["unc"], mu)
    F = P.objective(l, q, g["unc"], mu)
    assert np.all(l[g["unc"] == 0] == 1.0) and np.all((l > 0) & (l <= 1))
    rng = np.random.RandomState(0)
    for _ in range(50):
        l2 = l.copy()
        unc = np.flatnonzero(g["unc"])
        l2[unc] = np.clip(l[unc] + rng.randn(len(unc)) * 10.0 ** rng.uniform(-6, -1), 0.0, 1.0)
        assert P.objective(l2, q, g["unc"], mu) >= F * (1 - 1e-14)


def test_linearize_bounds_cover_a_permuted_sum():
    g = P.make_graph(4, 8, 5, 4)
    poses = np.array([P.mul(ir.rigid([1, 2, 3], 0.5, [0.01, -0.01, 0.02]), T) for T in g["init"]])
    a = P.linearize(poses, g, bounds=True)
    perm = np.random.RandomState(0).permutation(len(g["src"]))
    gp = {k: (v[perm] if k in ("src", "tgt", "trans", "info", "unc") else v) for k, v in g.items()}
    b = P.linearize(poses, gp)
    assert np.all(np.abs(a["H"] - b["H"]) <= (a["H_cnt"] + 2) * P.U * a["H_abs"])
    assert np.all(np.abs(a["b"] - b["b"]) <= (a["b_cnt"] + 2) * P.U * a["b_abs"])
    assert abs(a["F"] - b["F"]) <= (a["F_cnt"] + 2) * P.U * a["F_abs"]
    assert np.array_equal(a["H"], a["H"].T) and np.array_equal(a["H"][:6, :6], np.eye(6))


@pytest.mark.parametrize("seed,n,n_loops,n_false", KNOWN)
def test_known_answer_graphs(seed, n, n_loops, n_false):
    """Every false loop edge is dropped and every true one kept, with no confidence
    within 0.05 of the threshold; both linear solvers agree on it."""
    g = P.make_graph(seed, n, n_loops, n_false)
    assert len(g["src"]) == n - 1 + n_loops + n_false
    unc = g["unc"].astype(bool)
    for solver in ("cholesky", "solve"):
        r = P.optimize(g, g["init"], DIST, solver=solver)
        assert r["solver_failed"] == 0
        assert np.array_equal(r["keep"][unc], ~g["false"][unc]) and r["keep"][~unc].all()
        assert np.abs(r["confidence"][unc] - 0.25).min() > 0.05
        assert P.ate_cm(g["gt"], r["poses"]) < 1.0


def test_degenerate_graphs():
    one = dict(src=np.zeros(0, np.int32), tgt=np.zeros(0, np.int32), trans=np.zeros((0, 4, 4)),
               info=np.zeros((0, 6, 6)), unc=np.zeros(0, np.int32))
    pose = ir.rigid([1, 1, 0], 20.0, [1, 2, 3])[None]
    r = P.optimize(one, pose, DIST)
    assert np.array_equal(r["poses"], pose) and r["iterations"] == [0, 0]
    g = P.make_graph(5, 6, 0, 0)
    start = P.perturbed(g["init"], 0)
    r = P.optimize(g, start, DIST)
    assert r["mu"] == [0.0, 0.0] and np.all(r["confidence"] == 1.0) and r["keep"].all()
    # exact odometry: the minimum is F = 0 at the ground truth; plain LM runs to its min_residual stop
    assert r["objective"][1] < P.DEFAULT_CRITERIA["min_residual"]
    assert P.pose_gap(r["poses"], g["gt"]) < 1e-2 * P.pose_gap(start, g["gt"])
