"""numpy fp64 restatement of the multiway-registration semantics of
include/pdsc.h: f11 (the information matrix, by brute-force nearest neighbours)
and f12 (the pose-graph optimiser, by numpy.linalg.cholesky) -- the yardstick of
tests/test_gpu_multiway.py.  For every sum it forms it also returns the sum of
the absolute terms and the term count, from which the GPU tests take their
rounding bounds ((terms + 2) 2^-53 sum |terms|: any summation order of `terms`
products of a few factors stays inside it).

The rigid-transform products repeat the library's order, ((a0 b0 + a1 b1) +
a2 b2) (+ a3), so the residuals and Jacobians of the two differ only by the
rounding of atan2."""
import numpy as np

import icp_reference as ir

U = 2.0 ** -53
DEFAULT_CRITERIA = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6,
                        min_relative_residual_increment=1e-6, min_right_term=1e-6, min_residual=1e-6)


# ------------------------------------------------------------------------ f11
def information_matrix(src, tgt, T, r):
    """dict: info [6,6], n_corr, corr [Ns], and per entry of info the sum of the
    absolute terms (abs) and the number of terms (cnt)."""
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    corr = ir.evaluate(src, tgt, T, r)[0]
    t = np.asarray(tgt, np.float64)[corr[corr >= 0]]
    n = len(t)
    info, ab, cnt = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6), np.int64)
    for x, y, z in t:
        G = np.array([[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]], np.float64)
        info += G.T @ G
        ab += np.abs(G).T @ np.abs(G)
        cnt += (G != 0).T.astype(np.int64) @ (G != 0).astype(np.int64)
    return dict(info=info, n_corr=n, corr=corr, abs=ab, cnt=np.maximum(cnt, n))


# ------------------------------------------------------- rigid transforms [4,4]
def inv(T):
    """(R^T, -R^T t), the translation as -((a0 b0 + a1 b1) + a2 b2)."""
    I = np.eye(4)
    I[:3, :3] = T[:3, :3].T
    R, t = I[:3, :3], T[:3, 3]
    I[:3, 3] = -((R[:, 0] * t[0] + R[:, 1] * t[1]) + R[:, 2] * t[2])
    return I


def mul(A, B):
    """A B for rigid A, B in the library's order."""
    C = np.eye(4)
    C[:3, :] = (A[:3, 0:1] * B[0:1, :] + A[:3, 1:2] * B[1:2, :]) + A[:3, 2:3] * B[2:3, :]
    C[:3, 3] += A[:3, 3]
    return C


def vec6(M):
    sy = np.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
    if not sy < 1e-6:
        r = [np.arctan2(M[2, 1], M[2, 2]), np.arctan2(-M[2, 0], sy), np.arctan2(M[1, 0], M[0, 0])]
    else:
        r = [np.arctan2(-M[1, 2], M[1, 1]), np.arctan2(-M[2, 0], sy), 0.0]
    return np.array(r + [M[0, 3], M[1, 3], M[2, 3]])


def lin6(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2.0, (M[0, 2] - M[2, 0]) / 2.0, (M[1, 0] - M[0, 1]) / 2.0,
                     M[0, 3], M[1, 3], M[2, 3]])


def generator(i):
    D = np.zeros((4, 4))
    if i < 3:
        a, b = (i + 1) % 3, (i + 2) % 3
        D[a, b], D[b, a] = -1.0, 1.0
    else:
        D[i - 3, 3] = 1.0
    return D


def exp6(d):
    """Rz(d2) Ry(d1) Rx(d0) with translation d3..5."""
    cx, sx, cy, sy, cz, sz = np.cos(d[0]), np.sin(d[0]), np.cos(d[1]), np.sin(d[1]), np.cos(d[2]), np.sin(d[2])
    E = np.eye(4)
    E[:3, :3] = [[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                 [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                 [-sy, cy * sx, cy * cx]]
    E[:3, 3] = d[3:6]
    return E


def edge_residual(Ts, Tt, X):
    """(e [6], A = X^-1 Tt^-1, the entrywise |X^-1| |Tt^-1| |Ts| behind e's error bound)."""
    Xi, Ti = inv(X), inv(Tt)
    A = mul(Xi, Ti)
    return vec6(mul(A, Ts)), A, np.abs(Xi) @ np.abs(Ti) @ np.abs(Ts)


def edge_jacobian(A, Ts):
    """Js [6,6]: column i = lin6(A D_i Ts); Jt = -Js."""
    J = np.zeros((6, 6))
    for i in range(6):
        G = generator(i) @ Ts  # a selection of rows: exact
        M = np.zeros((4, 4))
        M[:3, :] = (A[:3, 0:1] * G[0:1, :] + A[:3, 1:2] * G[1:2, :]) + A[:3, 2:3] * G[2:3, :]
        J[:, i] = lin6(M)
    return J


# ------------------------------------------------------------------------ f12
def line_process(q, unc, mu):
    den = mu + q
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(den > 0, mu / np.where(den > 0, den, 1.0), 1.0)
    return np.where(unc != 0, f * f, 1.0)


def objective(l, q, unc, mu):
    return float((l * q).sum() + mu * ((np.sqrt(l[unc != 0]) - 1.0) ** 2).sum())


def linearize(poses, g, l=None, mu=0.0, ref=0, active=None, bounds=False):
    """One linearisation at `poses` [n,4,4] of graph g (dict: src, tgt, trans, info,
    unc) under the line process l (None: 1): dict e [E,6], q [E], F, H, b, J
    [E,6,6]; with bounds also {e,F,H,b}_abs and {e,F,H,b}_cnt."""
    n, E = len(poses), len(g["src"])
    l = np.ones(E) if l is None else np.asarray(l, np.float64)
    act = np.ones(E, bool) if active is None else np.asarray(active, bool)
    e, q, J = np.zeros((E, 6)), np.zeros(E), np.zeros((E, 6, 6))
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    out = {}
    if bounds:
        Ha, ba, ea = np.zeros_like(H), np.zeros_like(b), np.zeros((E, 6))
        Hc, bc = np.zeros(H.shape, np.int64), np.zeros(b.shape, np.int64)
        Fa = 0.0
    for k in range(E):
        if not act[k]:
            continue
        s, t = int(g["src"][k]), int(g["tgt"][k])
        L = g["info"][k]
        e[k], A, Mabs = edge_residual(poses[s], poses[t], g["trans"][k])
        J[k] = edge_jacobian(A, poses[s])
        q[k] = e[k] @ L @ e[k]
        B = J[k].T @ L @ J[k]
        B = np.triu(B) + np.triu(B, 1).T
        gk = J[k].T @ (L @ e[k])
        S, T = slice(6 * s, 6 * s + 6), slice(6 * t, 6 * t + 6)
        H[S, S] += l[k] * B
        H[T, T] += l[k] * B
        H[S, T] -= l[k] * B
        H[T, S] -= l[k] * B
        b[S] -= l[k] * gk
        b[T] += l[k] * gk
        if bounds:
            Ba = l[k] * (np.abs(J[k]).T @ np.abs(L) @ np.abs(J[k]))
            ga = l[k] * (np.abs(J[k]).T @ (np.abs(L) @ np.abs(e[k])))
            for P in (S, T):
                for Q in (S, T):
                    Ha[P, Q] += Ba
                    Hc[P, Q] += 36
                ba[P] += ga
                bc[P] += 36
            Fa += l[k] * (np.abs(e[k]) @ np.abs(L) @ np.abs(e[k]))
            # e: products of three rigid transforms (16 terms an entry); the rotation
            # entries are atan2 of unit-scale entries of that product, 1-Lipschitz in them
            ea[k, 3:] = Mabs[:3, 3]
            ea[k, :3] = 2.0 * Mabs[:3, :3].max()
    F = objective(l[act], q[act], np.asarray(g["unc"])[act], mu) if E else 0.0
    R = slice(6 * ref, 6 * ref + 6)
    H[R, :] = 0.0
    H[:, R] = 0.0
    H[R, R] = np.eye(6)
    b[R] = 0.0
    out.update(e=e, q=q, F=F, H=H, b=b, J=J)
    if bounds:
        for M in (Ha, Hc):
            M[R, :] = 0
            M[:, R] = 0
        ba[R] = 0
        bc[R] = 0
        unc = np.asarray(g["unc"])[act] != 0
        Fa += mu * ((np.sqrt(l[act][unc]) - 1.0) ** 2).sum()
        out.update(e_abs=ea, e_cnt=16, F_abs=Fa, F_cnt=36 * int(act.sum()) + int(unc.sum()), H_abs=Ha, H_cnt=Hc,
                   b_abs=ba, b_cnt=bc)
    return out


def stacked_vec6(poses):
    return np.concatenate([vec6(P) for P in poses])


def _solve(H, lam, b, solver):
    """(delta, ok): ok False on a Cholesky failure."""
    A = H + lam * np.eye(len(b))
    if solver == "solve":
        return np.linalg.solve(A, b), True
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, False
    return np.linalg.solve(L.T, np.linalg.solve(L, b)), True


def optimize(g, poses, max_correspondence_distance, edge_prune_threshold=0.25, preference_loop_closure=20.0,
             reference_node=0, criteria=None, solver="cholesky"):
    """The two-pass optimisation of include/pdsc.h f12.  dict: poses [n,4,4],
    confidence [E], keep [E], iterations [2], objective [2], mu [2], solver_failed."""
    c = dict(DEFAULT_CRITERIA, **(criteria or {}))
    poses = np.array(poses, np.float64)
    n, E = len(poses), len(g["src"])
    unc = np.asarray(g["unc"]).astype(bool) if E else np.zeros(0, bool)
    conf, keep = np.ones(E), np.ones(E, bool)
    res = dict(iterations=[0, 0], objective=[0.0, 0.0], mu=[0.0, 0.0], solver_failed=0)
    for ps in range(2):
        act = np.ones(E, bool) if ps == 0 else keep.copy()
        au = act & unc
        mu = (preference_loop_closure * max_correspondence_distance ** 2 * np.mean(g["info"][au][:, 5, 5])
              if au.any() else 0.0)

        def relin(P):
            lz = linearize(P, g, None, 0.0, reference_node, act)
            l = np.where(act, line_process(lz["q"], unc, mu), 1.0)
            lz = linearize(P, g, l, mu, reference_node, act)
            return l, lz

        l, lz = relin(poses)
        F, H, b = lz["F"], lz["H"], lz["b"]
        lam, nu = 1e-5 * max(0.0, H.diagonal().max()), 2.0
        stop = b.max() < c["min_right_term"] or F < c["min_residual"]
        it = 0
        while not stop and it < c["max_iteration"]:
            lm, rho = 0, 0.0
            while True:
                d, ok = _solve(H, lam, b, solver)
                if not ok:
                    res["solver_failed"] = 1
                    stop = True
                    break
                xn = np.linalg.norm(stacked_vec6(poses))
                if np.linalg.norm(d) < c["min_relative_increment"] * (xn + c["min_relative_increment"]):
                    stop = True
                else:
                    trial = np.array([mul(exp6(d[6 * i:6 * i + 6]), poses[i]) for i in range(n)])
                    Fn = linearize(trial, g, l, mu, reference_node, act)["F"]
                    rho = (F - Fn) / (d @ (lam * d + b) + 1e-3)
                    if rho > 0:
                        if F - Fn < c["min_relative_residual_increment"] * F:
                            stop = True
                        else:
                            poses = trial
                            l, lz = relin(poses)
                            F, H, b = lz["F"], lz["H"], lz["b"]
                            lam *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                            nu = 2.0
                            if b.max() < c["min_right_term"]:
                                stop = True
                    else:
                        lam *= nu
                        nu *= 2.0
                lm += 1
                if lm > c["max_iteration_lm"]:
                    stop = True
                if rho > 0 or stop:
                    break
            it += 1
            if F < c["min_residual"]:
                stop = True
        conf = np.where(act, l, conf)
        if ps == 0:
            keep = ~unc | (conf > edge_prune_threshold)
        res["iterations"][ps], res["objective"][ps], res["mu"][ps] = it, F, mu
        if res["solver_failed"]:
            break
    res.update(poses=poses, confidence=conf, keep=keep)
    return res


def gauss_newton_fixed_l(g, poses, l, mu, active, reference_node=0, steps=50):
    """The minimiser of F at fixed l over the active edges: plain Gauss-Newton from
    `poses` until the step is below 1e-13 (the ground truth the optimiser's poses
    are measured against)."""
    poses = np.array(poses, np.float64)
    for _ in range(steps):
        lz = linearize(poses, g, l, mu, reference_node, active)
        d = np.linalg.solve(lz["H"], lz["b"])
        poses = np.array([mul(exp6(d[6 * i:6 * i + 6]), poses[i]) for i in range(len(poses))])
        if np.linalg.norm(d) < 1e-13:
            break
    return poses


def pose_gap(A, B):
    """The largest entrywise difference of two pose stacks (rotation entries and metres alike)."""
    return float(np.abs(np.asarray(A)[:, :3, :] - np.asarray(B)[:, :3, :]).max())


# ---------------------------------------------------------------- test inputs
def make_graph(seed, n, n_loops, n_false, rot_noise_deg=0.2, trans_noise=0.002, cloud=150, r=0.07):
    """A known-answer graph: ground-truth poses on a closed loop (radius 2 m, the
    heading turning with the position, a slow tilt); exact odometry edges i -> i +
    1 (certain); n_loops true loop edges s -> t, t >= s + 2, with pose noise
    (rot_noise_deg about a random axis, trans_noise metres), uncertain; n_false
    false loop edges (s > t, a random rotation of 30 .. 180 degrees and 0.5 .. 1.5 m),
    uncertain.  Every edge's information matrix is the f11 restatement's on a
    synthetic cloud pair that overlaps under the edge's own transformation (a
    random 60 .. 100 % of `cloud` points, 1 mm noise), radius r.  Initial poses:
    the chained odometry.  dict: src, tgt, trans [E,4,4], info [E,6,6], unc, false
    [E] bool, gt [n,4,4], init [n,4,4]."""
    rng = np.random.RandomState(seed)
    gt = []
    for i in range(n):
        a = 2 * np.pi * i / max(n, 3)
        T = ir.rigid([0, 0, 1], np.degrees(a) + 90.0, [2 * np.cos(a), 2 * np.sin(a), 0.1 * np.sin(2 * a)])
        gt.append(T @ ir.rigid([1, 0, 0], 10.0 * np.sin(a), [0, 0, 0]))
    gt = np.array(gt)
    base = rng.rand(cloud, 3) * 2.0 - 1.0
    src, tgt, trans, unc, false = [], [], [], [], []
    for i in range(n - 1):
        src.append(i), tgt.append(i + 1), unc.append(0), false.append(False)
        trans.append(mul(inv(gt[i + 1]), gt[i]))
    pairs = [(s, t) for s in range(n) for t in range(s + 2, n)]
    for k in rng.permutation(len(pairs))[:n_loops]:
        s, t = pairs[k]
        d = rng.randn(3)
        noise = ir.rigid(rng.randn(3), rot_noise_deg, trans_noise * d / np.linalg.norm(d))
        src.append(s), tgt.append(t), unc.append(1), false.append(False)
        trans.append(mul(noise, mul(inv(gt[t]), gt[s])))
    back = [(s, t) for s in range(n) for t in range(s)]
    for k in rng.permutation(len(back))[:n_false]:
        s, t = back[k]
        d = rng.randn(3)
        src.append(s), tgt.append(t), unc.append(1), false.append(True)
        trans.append(ir.rigid(rng.randn(3), 30.0 + 150.0 * rng.rand(), (0.5 + rng.rand()) * d / np.linalg.norm(d)))
    assert len(src) == n - 1 + n_loops + n_false, "not enough node pairs for the edges asked for"
    info = []
    for X in trans:
        sel = rng.rand(cloud) < 0.6 + 0.4 * rng.rand()
        tg = (base + rng.randn(cloud, 3) * 0.001).astype(np.float32)
        sc = ir.transform(inv(X), base[sel]).astype(np.float32)
        info.append(information_matrix(sc, tg, X, r)["info"])
    init = [gt[0]]
    for i in range(n - 1):
        init.append(mul(init[i], inv(trans[i])))
    return dict(src=np.array(src, np.int32), tgt=np.array(tgt, np.int32), trans=np.array(trans).reshape(-1, 4, 4),
                info=np.array(info).reshape(-1, 6, 6), unc=np.array(unc, np.int32), false=np.array(false, bool),
                gt=gt, init=np.array(init))


def perturbed(poses, seed, deg=1.0, shift=0.02):
    """Every pose but the first moved by its own random motion of `deg` degrees and `shift` metres."""
    rng = np.random.RandomState(seed)
    out = [poses[0]]
    for T in poses[1:]:
        d = rng.randn(3)
        out.append(mul(ir.rigid(rng.randn(3), deg, shift * d / np.linalg.norm(d)), T))
    return np.array(out)


def ate_cm(gt, est):
    """multiway/test_multi_ate.py:31-51, 268-287 in fp64: align the gt positions
    onto the estimated ones (Kabsch), the RMSE of what is left in cm."""
    a, b = np.asarray(gt)[:, :3, 3], np.asarray(est)[:, :3, 3]
    T = ir.kabsch(a, b)
    err = np.linalg.norm(ir.transform(T, a) - b, axis=1) * 100.0
    return float(np.sqrt(np.mean(err ** 2)))
