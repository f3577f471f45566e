"""numpy fp64 restatement of include/pdsc.h f9 (TEASER++ after the clique): the
GNC-TLS rotation loop as the header writes it, the scalar TLS estimate the
SEQUENTIAL way (sorted event loop, running sums -- not the kernel's windows and
prefix sums), the CHAIN TIMs, the solve on given clique members and
Grid_Prioritized_Filter(BB_first=True) along the reference's lines.  It shares
no code with the library.  tests/test_teaser_reference.py holds it to brute
force and planted truths on the CPU; tests/test_gpu_teaser.py holds the kernels
to it.

svd_rot is a9's Jacobi solve restated operation by operation (eigenvectors of
H^T H by cyclic Jacobi, u = H v, the deterministic completion where H has rank
< 2), so that rank-deficient inputs (K = 1, two opposite TIMs) have ONE answer;
test_teaser_reference checks it against numpy's SVD wherever the data determine
the rotation."""
import numpy as np

import fr_reference as F

INF = float("inf")


# ------------------------------------------------------------------- rotation
def _jrot(a, p, q, r, V):
    """One Jacobi rotation zeroing a[p][q] of the symmetric 3x3 a (r the third index)."""
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] -= t * apq
    a[q][q] += t * apq
    a[p][q] = a[q][p] = 0.0
    rp, rq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * rp - s * rq
    a[r][q] = a[q][r] = s * rp + c * rq
    vp, vq = V[:, p].copy(), V[:, q].copy()
    V[:, p] = c * vp - s * vq
    V[:, q] = s * vp + c * vq


def _orthogonal(a):
    x = np.abs(a)
    e = np.array([1.0, 0, 0]) if (x[0] <= x[1] and x[0] <= x[2]) else (np.array([0, 1.0, 0]) if x[1] <= x[2]
                                                                       else np.array([0, 0, 1.0]))
    o = np.cross(a, e)
    return o / np.sqrt(o @ o)


def svd_rot(H):
    """R = V diag(1, 1, det(V U^T)) U^T for H = U S V^T (H = sum w a b^T: b ~ R a)."""
    H = np.asarray(H, np.float64)
    if not np.abs(H).max() > 0:
        return np.eye(3)
    a = [[float(sum(H[k][i] * H[k][j] for k in range(3))) for j in range(3)] for i in range(3)]
    V = np.eye(3)
    for _ in range(10):
        off = a[0][1] ** 2 + a[0][2] ** 2 + a[1][2] ** 2
        dia = a[0][0] ** 2 + a[1][1] ** 2 + a[2][2] ** 2
        if off <= 1e-26 * dia or off == 0.0:
            break
        _jrot(a, 0, 1, 2, V)
        _jrot(a, 0, 2, 1, V)
        _jrot(a, 1, 2, 0, V)
    lam = [a[0][0], a[1][1], a[2][2]]
    for (i, j) in ((0, 1), (0, 2), (1, 2)):
        if lam[i] < lam[j]:
            lam[i], lam[j] = lam[j], lam[i]
            V[:, [i, j]] = V[:, [j, i]]
    v0, v1, v2 = V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()
    u0, u1 = H @ v0, H @ v1
    n0 = np.sqrt(u0 @ u0)
    u0 = u0 / n0 if n0 > 0 else u0
    if not n0 > 1e-300:
        u0 = _orthogonal(v0)
    u1 = u1 - (u1 @ u0) * u0
    n1 = np.sqrt(u1 @ u1)
    u1 = u1 / n1 if n1 > 0 else u1
    if not n1 > 1e-12 * n0:
        u1 = _orthogonal(u0)
    u2 = np.cross(u0, u1)
    d = -1.0 if v0 @ np.cross(v1, v2) < 0 else 1.0
    return np.outer(v0, u0) + np.outer(v1, u1) + d * np.outer(v2, u2)


def svd_rot_lapack(H):
    """The same rotation from numpy's SVD (defined where H has rank >= 2)."""
    U, _, Vt = np.linalg.svd(np.asarray(H, np.float64))
    V = Vt.T
    if np.linalg.det(U) * np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    return V @ U.T


def gnc_tls_rotation(a, b, noise_bound, gnc_factor=1.4, max_iterations=10000, cost_threshold=1e-16, trace=None):
    """dict: R [3,3], weights [K], inliers bool [K], iterations, cost, mu,
    stop_reason, residuals (the last pass's r_j).  trace (a list) receives per
    pass the numbers of weights set by the three branches (zero, one, middle)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    K = len(a)
    nb2 = noise_bound * noise_bound
    w = np.ones(K)
    prev, mu, cost, reason, it = INF, 0.0, 0.0, 0, 0
    R, r = np.eye(3), np.zeros(K)
    for i in range(max_iterations):
        wa = w[:, None] * a
        # sequential sums in TIM order (cumsum adds one row after the other)
        H = np.cumsum((wa[:, :, None] * b[:, None, :]).reshape(K, 9), axis=0)[-1].reshape(3, 3)
        R = svd_rot(H)
        it = i + 1
        d_ = b - np.stack([(R[k, 0] * a[:, 0] + R[k, 1] * a[:, 1]) + R[k, 2] * a[:, 2] for k in range(3)], 1)
        r = (d_[:, 0] * d_[:, 0] + d_[:, 1] * d_[:, 1]) + d_[:, 2] * d_[:, 2]
        cost = float(np.cumsum(w * r)[-1])
        if i == 0:
            d = 2.0 * r.max() / nb2 - 1.0
            if d <= 0:
                reason = 1
                break
            mu = 1.0 / d
        th1, th2 = (mu + 1.0) / mu * nb2, mu / (mu + 1.0) * nb2
        zero, one = r >= th1, (r <= th2) & ~(r >= th1)
        mid = ~zero & ~one
        w = np.where(zero, 0.0, 1.0)
        w[mid] = np.sqrt(nb2 * mu * (mu + 1.0) / r[mid]) - mu
        if trace is not None:
            trace.append((int(zero.sum()), int(one.sum()), int(mid.sum())))
        diff = abs(cost - prev)
        mu *= gnc_factor
        prev = cost
        if diff < cost_threshold:
            reason = 2
            break
    return dict(R=R, weights=w, inliers=w >= 0.5, iterations=it, cost=cost, mu=mu, stop_reason=reason, residuals=r)


# ---------------------------------------------------------------- translation
def tls_events(x, beta):
    """The 2K events sorted by (value, tag): arrays (value, tag)."""
    x = np.asarray(x, np.float64)
    K = len(x)
    val = np.concatenate([x - beta, x + beta])
    tag = np.concatenate([np.arange(1, K + 1), -np.arange(1, K + 1)])
    o = np.lexsort((tag, val))
    return val[o], tag[o]


def tls_scalar(x, beta, detail=False):
    """The scalar TLS estimate by adaptive voting, sequentially: running n, sum x,
    sum x^2 over the event loop; xhat of the first event of minimal cost.  detail:
    also (best cost, the runner-up cost among events whose consensus set is a
    different window, by (n, min, max) of the set)."""
    x = np.asarray(x, np.float64)
    K = len(x)
    _, tag = tls_events(x, beta)
    n, sx, sxx = 0, 0.0, 0.0
    best, best_x, rows = INF, None, []
    inside = np.zeros(K, bool)
    for tg in tag:
        j = abs(int(tg)) - 1
        if tg > 0:
            n, sx, sxx = n + 1, sx + x[j], sxx + x[j] * x[j]
            inside[j] = True
        else:
            n, sx, sxx = n - 1, sx - x[j], sxx - x[j] * x[j]
            inside[j] = False
        if n == 0:
            sx, sxx = 0.0, 0.0  # an empty set carries no rounding residue on
            continue
        xh = sx / n
        cost = (n * xh * xh + sxx - 2.0 * xh * sx) + beta * (K - n)
        if detail:
            xs = x[inside]
            rows.append((cost, (n, xs.min(), xs.max())))
        if cost < best:
            best, best_x = cost, xh
    if not detail:
        return best_x
    k = int(np.argmin([c for c, _ in rows]))
    other = [c for c, sig in rows if sig != rows[k][1]]
    return best_x, rows[k][0], (min(other) if other else INF)


def tls_scalar_brute(x, beta):
    """O(K^2): every event's consensus set enumerated, mean and cost from scratch."""
    x = np.asarray(x, np.float64)
    K = len(x)
    _, tag = tls_events(x, beta)
    best, best_x = INF, None
    for e in range(len(tag)):
        inside = np.zeros(K, bool)
        for tg in tag[:e + 1]:
            inside[abs(int(tg)) - 1] = tg > 0
        if not inside.any():
            continue
        xs = x[inside]
        xh = xs.mean()
        cost = ((xs - xh) ** 2).sum() + beta * (K - len(xs))
        if cost < best:
            best, best_x = cost, xh
    return best_x


def tls_translation(src, dst, beta):
    """(t [3], inliers bool [K]) for rotated src and dst, [K,3] fp64."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    x = dst - src
    t = np.array([tls_scalar(x[:, c], beta) for c in range(3)])
    return t, (np.abs(x - t) <= beta).all(1)


# ---------------------------------------------------------------------- solve
def chain_tims(src, tgt, members):
    """CHAIN TIMs over members c_0 < ... (fp64 differences of the fp32 points)."""
    m = np.asarray(members, np.int64)
    nxt = np.roll(m, -1)
    s, t = np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)
    return s[nxt] - s[m], t[nxt] - t[m]


def solve_on_members(src, tgt, members, noise_bound, tim_perm=None, **gnc):
    """pdsc_teaser_solve after step 2, on given clique members: dict with trans
    [4,4], valid, labels [N], gnc (the rotation's dict), t_inliers.  tim_perm: the
    order in which the rotation stage sums the chain's TIMs (the spread under it
    is the yardstick of the GPU comparison)."""
    N = len(src)
    m = np.sort(np.asarray(members, np.int64))
    out = dict(trans=np.eye(4), valid=0, labels=np.zeros(N, np.float32), gnc=None, t_inliers=np.zeros(0, bool))
    if len(m) <= 1:
        return out
    a, b = chain_tims(src, tgt, m)
    if tim_perm is not None:
        a, b = a[tim_perm], b[tim_perm]
    g = gnc_tls_rotation(a, b, noise_bound, **gnc)
    R = g["R"]
    s = np.asarray(src, np.float32).astype(np.float64)[m]
    rot = np.stack([(R[i, 0] * s[:, 0] + R[i, 1] * s[:, 1]) + R[i, 2] * s[:, 2] for i in range(3)], 1)
    t, inl = tls_translation(rot, np.asarray(tgt, np.float32).astype(np.float64)[m], noise_bound)
    out["trans"][:3, :3], out["trans"][:3, 3] = R, t
    out["labels"][m[inl]] = 1.0
    out.update(valid=1, gnc=g, t_inliers=inl)
    return out


def length_graph(src, tgt, thr):
    """f8's PDSC_EDGE_LENGTH predicate on the rows [src_i, tgt_i]: fp32 squares
    summed ((x + y) + z), correctly rounded fp32 roots, |diff| < thr in fp64."""
    s, t = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    ds, dt = s[:, None] - s[None], t[:, None] - t[None]
    a = np.sqrt(((ds[..., 0] * ds[..., 0] + ds[..., 1] * ds[..., 1]) + ds[..., 2] * ds[..., 2]).astype(np.float32))
    b = np.sqrt(((dt[..., 0] * dt[..., 0] + dt[..., 1] * dt[..., 1]) + dt[..., 2] * dt[..., 2]).astype(np.float32))
    adj = np.abs((a - b).astype(np.float32)).astype(np.float64) < thr
    np.fill_diagonal(adj, False)
    return adj


def greedy_clique(adj):
    """A (not necessarily maximum) clique for the CPU-only whole-solve check: from
    the vertex of the highest degree, add the candidate of the highest degree."""
    deg = adj.sum(1)
    v = int(np.argmax(deg))
    C, P = [v], adj[v].copy()
    while P.any():
        cand = np.flatnonzero(P)
        u = int(cand[np.argmax(deg[cand])])
        C.append(u)
        P &= adj[u]
    return np.sort(np.array(C))


# --------------------------------------------------------------------- filter
def gpf_bb_first(f0, f1, xyz0, grid, max_matches):
    """Grid_Prioritized_Filter(BB_first=True), matching.py:112-116 and on: dict
    idx0, idx1 of the kept pairs and early (True: all mutual pairs returned)."""
    nn = F.nn2(f0, f1)
    i0 = np.flatnonzero(nn["rev"][nn["nn1"]] == np.arange(len(f0)))
    i1, i2 = nn["nn1"][i0], nn["nn2"][i0]
    if max_matches >= len(i0):
        return dict(idx0=i0, idx1=i1, early=True)
    a, b = np.asarray(f0, np.float64)[i0], np.asarray(f1, np.float64)
    fd = np.sqrt(((a - b[i1]) ** 2).sum(1)) / (np.sqrt(((a - b[i2]) ** 2).sum(1)) + 1e-6)
    m, M = fd.min(), fd.max()
    norm = (fd - m) / (M - m) if M > m else np.zeros_like(fd)
    g = F.gpf_select(np.asarray(xyz0, np.float32)[i0], norm, max_matches, grid, 1.0)
    return dict(idx0=i0[g["kept"]], idx1=i1[g["kept"]], early=False, norm=norm, gpf=g)


# ----------------------------------------------------------------- test inputs
def rotation_from(rng):
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    th = 0.2 + 2.5 * rng.rand()
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def tim_case(K, seed, noise_bound=0.3, outliers=0.3, noise=0.3):
    """(a, b [K,3] fp64, R planted, outlier mask): TIMs of a few metres, noise
    `noise` * noise_bound per axis, `outliers` of them with an unrelated b."""
    rng = np.random.RandomState(100003 * K + seed)
    R = rotation_from(rng)
    a = rng.randn(K, 3) * 3.0
    b = a @ R.T + noise * noise_bound * rng.randn(K, 3) / np.sqrt(3.0)
    out = np.zeros(K, bool)
    out[rng.permutation(K)[:int(round(outliers * K))]] = True
    b[out] = rng.randn(int(out.sum()), 3) * 3.0
    return a, b, R, out


def offset_case(K, seed, beta=0.3, dup=False):
    """(src, dst [K,3] fp64, t planted): 70 % of dst - src within 0.3 beta (per
    axis, Gaussian) of t, 30 % uniform in +-8.  dup: values drawn from a coarse
    lattice, so many x repeat exactly."""
    rng = np.random.RandomState(7001 * K + seed)
    t = rng.uniform(-2, 2, 3)
    src = rng.randn(K, 3) * 5.0
    x = t + 0.3 * beta * rng.randn(K, 3)
    out = rng.permutation(K)[:int(0.3 * K)]  # K <= 3: none (two far singletons would tie at cost beta)
    x[out] = rng.uniform(-8, 8, (len(out), 3))
    if dup:
        x = np.round(x * 8.0) / 8.0
        src = np.round(src * 8.0) / 8.0  # dst - src is then exact
    return src, src + x, t
