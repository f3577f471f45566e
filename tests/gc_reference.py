"""numpy fp64 restatement of GC-RANSAC as include/pdsc.h (f10) defines it: the
grid neighbourhood, the per-cell minimiser of the graph-cut energy (with a brute
force over all 2^n labellings to hold it against), the MSAC score and the solver
with its local optimisation at round granularity -- the yardstick of
tests/test_gpu_gc.py.  The sampler and the extended-precision Kabsch are
tests/ransac_reference.py's.  pygcransac is not installed and its source is not
in the reference tree: parity with the library itself is unpinned; this file
follows the header's comment step by step.

Diagnostics say whether a case is free of near-ties, so that the GPU's fused
multiply-adds, its exp and its summation order cannot flip a decision.  The
margins for distances, sigma ratios, the stop rule and score gaps are
ransac_reference.tie_free's (1e-7, 1e-5, 1 %, 1e-9).  The energy-gap margin comes
from a measured rounding envelope (measure_envelope below): perturbing every K
of a cell by one ulp up or down at random moves E(m) by at most 1.6e-16 relative
to max(1, max_m |E(m)|) (300 random cells of 2 .. 1025 rows, lambda in {0, 0.1,
0.975, 1}, 8 perturbations each; measured 2026-10-20).  The GPU's K can be off
by more than one ulp -- its d^2 differs from this file's by about 1e-15
absolute, which eps = 0.1 turns into 5e-14 relative in K -- so the margin is
ENERGY_MARGIN = 1e-9 of that scale: seven orders over the one-ulp envelope, four
over the d^2 effect.
"""
import functools
import itertools

import numpy as np

import ransac_reference as RR

ROUND = RR.ROUND  # pdsc_gc_ransac_round(); tests assert the library's value equals it
WAVE_CELL, LDS_CELL = 64, 1024  # pdsc_gc_cell_bound(0 / 1); tests assert the library's values equal them
LO_STEPS = 10
ENERGY_MARGIN = 1e-9
X = np.longdouble


# ------------------------------------------------------------------------ grid
def gc_grid(src, tgt, G):
    """order [N], cell_start [n_cells + 1], cell_of [N], n_cells, keys [N] (uint64)."""
    P = np.concatenate([np.asarray(src, np.float32), np.asarray(tgt, np.float32)], 1)
    N = len(P)
    key = np.zeros(N, np.uint64)
    for a in range(6):
        x, m, M = P[:, a].astype(np.float64), np.float64(P[:, a].min()), np.float64(P[:, a].max())
        if M == m:
            c = np.zeros(N, np.int64)
        else:
            c = np.minimum(G - 1, np.floor((np.float64(G) * (x - m)) / (M - m)).astype(np.int64))
        key = key * np.uint64(G) + c.astype(np.uint64)
    order = np.lexsort((np.arange(N), key))
    ks = key[order]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    cell_start = np.concatenate([first, [N]]).astype(np.int64)
    cell_of = np.zeros(N, np.int64)
    cell_of[order] = np.cumsum(np.concatenate([[1], (ks[1:] != ks[:-1]).astype(np.int64)])) - 1
    return dict(order=order, cell_start=cell_start, cell_of=cell_of, n_cells=len(first), key=key)


# ------------------------------------------------------------------- minimiser
def cell_energies(K_sorted, lam):
    """E(m), m = 0 .. n, for K in ascending (d2, row) order: the header's formula, operation by operation."""
    K = np.asarray(K_sorted, np.float64)
    n = len(K)
    P = np.zeros(n + 1)
    acc = np.float64(0.0)
    for i in range(n):  # sequential, from 0.0
        acc = acc + K[i]
        P[i + 1] = acc
    S = P[n]
    m, dn = np.arange(n + 1, dtype=np.float64), np.float64(n)
    u = (m - 2.0 * P) + S
    a = m * (dn - m)
    b = (((dn - m) - 1.0) * 0.5) * (S - P)
    c = (m * (m - 1.0)) * 0.5
    d = ((m - 1.0) * 0.5) * P
    return (1.0 - lam) * u + lam * (((a + b) + c) - d)


def cell_minimise(K_sorted, lam):
    """(m_star, E(m_star), second-lowest E - lowest E); ties to the lower m."""
    E = cell_energies(K_sorted, lam)
    m = int(np.argmin(E))  # numpy: the first minimum
    rest = np.delete(E, m)
    return m, float(E[m]), float(rest.min() - E[m])


def labelling_energy(K, L, lam):
    """The energy of labelling L (0/1) of one cell with residual kernels K, term by term (any order of rows)."""
    K, L = np.asarray(K, np.float64), np.asarray(L, np.int64)
    e = ((1.0 - lam) * np.where(L == 1, 1.0 - K, K)).sum()
    for p, q in itertools.combinations(range(len(K)), 2):
        if L[p] != L[q]:
            e += lam
        elif L[p] == 0:
            e += lam * (K[p] + K[q]) / 2
        else:
            e += lam * (1 - (K[p] + K[q]) / 2)
    return float(e)


def brute_force(K, lam):
    """(minimum energy over all 2^n labellings, the minimisers' inlier counts) for n <= 12."""
    n = len(K)
    assert n <= 12
    best, ms = np.inf, []
    for bits in range(1 << n):
        L = [(bits >> i) & 1 for i in range(n)]
        e = labelling_energy(K, L, lam)
        if e < best - 1e-12:
            best, ms = e, [sum(L)]
        elif abs(e - best) <= 1e-12:
            ms.append(sum(L))
    return best, ms


def measure_envelope(cells=300, trials=8, seed=0):
    """max |E'(m) - E(m)| / max(1, max |E|) under random one-ulp perturbations of every K (see the module docstring)."""
    rng = np.random.RandomState(seed)
    worst = 0.0
    for _ in range(cells):
        n = int(rng.choice([2, 3, 8, 64, 65, 300, 1025]))
        K = np.sort(np.exp(-rng.rand(n) * rng.choice([0.5, 5.0, 50.0])))[::-1]
        for lam in (0.0, 0.1, 0.975, 1.0):
            E = cell_energies(K, lam)
            for _ in range(trials):
                Kp = np.where(rng.rand(n) < 0.5, np.nextafter(K, 2.0), np.nextafter(K, -1.0))
                worst = max(worst, float(np.abs(cell_energies(Kp, lam) - E).max() / max(1.0, np.abs(E).max())))
    return worst


# ----------------------------------------------------------------------- label
def distances2(T, src, tgt):
    """d^2 [N] of one [4,4], worked in extended precision from the fp64 pose and rounded to fp64."""
    T = np.asarray(T, np.float64).astype(X)
    q = np.asarray(src, np.float32).astype(X) @ T[:3, :3].T + T[:3, 3]
    return ((q - np.asarray(tgt, np.float32).astype(X)) ** 2).sum(1).astype(np.float64)


def gc_label(T, src, tgt, grid, eps, lam):
    """labels [N], count, d2 [N], per cell m_star / energy / energy_gap, and diag: adjacent = the smallest
    relative gap of adjacent d2 inside a cell (rows with identical coordinates aside: their d2 are the same
    bits everywhere and the order falls to the row), energy = the smallest energy_gap / max(1, |E|) (cells where
    lambda = 1 makes every E exactly 0 aside: singletons)."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    d2 = distances2(T, src, tgt)
    K = np.exp(-(d2 / (2.0 * (np.float64(eps) * np.float64(eps)))))
    N, nc = len(src), grid["n_cells"]
    labels = np.zeros(N, np.float32)
    m_star, energy, gap = np.zeros(nc, np.int64), np.zeros(nc), np.zeros(nc)
    diag = dict(adjacent=np.inf, energy=np.inf)
    rows6 = np.concatenate([src, tgt], 1)
    for k in range(nc):
        rows = grid["order"][grid["cell_start"][k]:grid["cell_start"][k + 1]]
        o = rows[np.lexsort((rows, d2[rows]))]
        m, e, g = cell_minimise(K[o], lam)
        m_star[k], energy[k], gap[k] = m, e, g
        labels[o[:m]] = 1.0
        if len(o) > 1:
            ds = d2[o]
            same = (rows6[o[1:]] == rows6[o[:-1]]).all(1)
            rel = (ds[1:] - ds[:-1]) / np.maximum(ds[1:], 1e-300)
            if (~same).any():
                diag["adjacent"] = min(diag["adjacent"], float(rel[~same].min()))
        if not (lam == 1.0 and len(o) == 1):
            diag["energy"] = min(diag["energy"], g / max(1.0, abs(e)))
    return dict(labels=labels, count=int(labels.sum()), d2=d2, m_star=m_star, energy=energy, energy_gap=gap, diag=diag)


def label_tie_free(diag):
    return bool(diag["adjacent"] >= 1e-7 and diag["energy"] >= ENERGY_MARGIN)


# ---------------------------------------------------------------------- solver
def msac(T, src, tgt, eps):
    """(score, count, the smallest | d - eps | / eps) of one pose; sums in extended precision."""
    d2 = distances2(T, src, tgt).astype(X)
    r2 = X(np.float64(eps) * np.float64(eps))
    inl = d2 < r2
    margin = float((np.abs(np.sqrt(d2) - X(eps)) / X(eps)).min())
    return float(np.where(inl, X(1) - d2 / r2, X(0)).sum()), int(inl.sum()), margin


def _round_scores(R, t, src, tgt, eps, diag):
    """fp64 scores / counts of a batch of poses (ranking and margins only; the top ones are redone by msac)."""
    r2 = np.float64(eps) * np.float64(eps)
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    score, count = np.zeros(len(R)), np.zeros(len(R), np.int64)
    for s in range(0, len(R), 1024):
        q = np.einsum("hij,nj->hni", R[s:s + 1024], s64) + t[s:s + 1024, None, :] - t64[None]
        d2 = (q * q).sum(2)
        inl = d2 < r2
        score[s:s + 1024] = np.where(inl, 1.0 - d2 / r2, 0.0).sum(1)
        count[s:s + 1024] = inl.sum(1)
        diag["distance_margin"] = min(diag["distance_margin"], float((np.abs(np.sqrt(d2) - eps) / eps).min()))
    return score, count


def gc_ransac(src, tgt, eps, lam, G=20, max_iteration=1000, confidence=1.0, seed=0, lo=True, round_size=ROUND,
              rows=True):
    """dict: per-hypothesis samples [H,3], count [H] (-1 repeated, -3 not drawn), hyp_score [H], trans [H,4,4]
    (score / count of every hypothesis in fp64; with rows=True redone in extended precision for all of them --
    the stage test -- else only for the three best of a round); the result best, score, n_inliers, iterations,
    lo_runs, lo_steps, n_cells, labels, transformation, best_minimal_score; diag."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    N, H = len(src), int(max_iteration)
    grid = gc_grid(src, tgt, G) if lo else None
    out = dict(samples=np.zeros((H, 3), np.int64), count=np.full(H, -3, np.int64), hyp_score=np.zeros(H),
               trans=np.zeros((H, 4, 4)))
    diag = dict(distance_margin=np.inf, sigma_ratio=np.inf, score_gap=np.inf, stop=[], lo_delta=np.inf,
                adjacent=np.inf, energy=np.inf)
    best, bT, bscore, bcount, iterations, lo_runs, lo_steps, best_minimal = -1, np.eye(4), -1.0, -1, 0, 0, 0, -1.0
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    for rd in range((H + round_size - 1) // round_size):
        h = np.arange(rd * round_size, min((rd + 1) * round_size, H))
        idx = RR.draw(seed, h, 3, N)
        out["samples"][h] = idx
        rep = (idx[:, 0] == idx[:, 1]) | (idx[:, 0] == idx[:, 2]) | (idx[:, 1] == idx[:, 2])
        out["count"][h[rep]] = -1
        hv = h[~rep]
        iterations = int(h[-1]) + 1
        if len(hv):
            R, t, sig = RR.kabsch_batch(s64[idx[~rep]], t64[idx[~rep]])
            diag["sigma_ratio"] = min(diag["sigma_ratio"], float((sig[:, 1] / np.maximum(sig[:, 0], 1e-300)).min()))
            out["trans"][hv, :3, :3], out["trans"][hv, :3, 3], out["trans"][hv, 3, 3] = R, t, 1.0
            sc, cnt = _round_scores(R, t, src, tgt, eps, diag)
            top = np.lexsort((hv, -sc))
            for o in (top if rows else top[:3]):
                sc[o], cnt[o], _ = msac(out["trans"][hv[o]], src, tgt, eps)
            out["hyp_score"][hv], out["count"][hv] = sc, cnt
            top = np.lexsort((hv, -sc))
            o = top[0]
            if len(top) > 1:
                diag["score_gap"] = min(diag["score_gap"], (sc[o] - sc[top[1]]) / max(sc[o], 1e-300))
            if bscore >= 0:
                diag["score_gap"] = min(diag["score_gap"], abs(sc[o] - bscore) / max(sc[o], bscore, 1e-300))
            if sc[o] > bscore:
                T, s_, c_ = out["trans"][hv[o]].copy(), float(sc[o]), int(cnt[o])
                best_minimal = max(best_minimal, s_)
                if lo:
                    lo_runs += 1
                    prev = None
                    for _ in range(LO_STEPS):
                        lab = gc_label(T, src, tgt, grid, eps, lam)
                        lo_steps += 1
                        diag["adjacent"] = min(diag["adjacent"], lab["diag"]["adjacent"])
                        diag["energy"] = min(diag["energy"], lab["diag"]["energy"])
                        if lab["count"] < 3:
                            break
                        T2 = RR.kabsch(s64[lab["labels"] > 0], t64[lab["labels"] > 0])
                        s2, c2, mg = msac(T2, src, tgt, eps)
                        diag["distance_margin"] = min(diag["distance_margin"], mg)
                        # the same rows as the step before give the same fit and the same score, bit for bit, in
                        # any arithmetic: the LO's fixed point, an exact tie and no near-tie
                        if prev is None or not np.array_equal(prev, lab["labels"]):
                            diag["lo_delta"] = min(diag["lo_delta"], abs(s2 - s_) / max(s2, s_, 1e-300))
                        prev = lab["labels"]
                        if not s2 > s_:
                            break
                        T, s_, c_ = T2, s2, c2
                best, bT, bscore, bcount = int(hv[o]), T, s_, c_
        if confidence < 1.0 and bcount > 0:
            if bcount == N:
                break
            f = bcount / N
            lhs, rhs = float((rd + 1) * round_size), np.log(1.0 - confidence) / np.log(1.0 - f * f * f)
            diag["stop"].append(abs(lhs - rhs) / max(lhs, rhs))
            if lhs >= rhs:
                break
    labels = np.zeros(N, np.float32)
    T = bT
    if best >= 0:
        labels = (distances2(bT, src, tgt) < np.float64(eps) * np.float64(eps)).astype(np.float32)
        assert int(labels.sum()) == bcount
        if bcount >= 3:
            T = RR.kabsch(s64[labels > 0], t64[labels > 0])
    out.update(best=best, score=max(bscore, 0.0), n_inliers=max(bcount, 0), iterations=iterations, lo_runs=lo_runs,
               lo_steps=lo_steps, n_cells=grid["n_cells"] if lo else 0, labels=labels, transformation=T,
               best_minimal_score=best_minimal, diag=diag)
    return out


def tie_free(diag):
    """ransac_reference.tie_free's margins on this solver's decisions, and label_tie_free on every labelling."""
    return bool(diag["distance_margin"] >= 1e-7 and diag["sigma_ratio"] >= 1e-5 and diag["score_gap"] >= 1e-9
                and diag["lo_delta"] >= 1e-9 and all(s >= 0.01 for s in diag["stop"]) and label_tie_free(diag))


# ---------------------------------------------------------------- the GPU file's cases
EPS = 0.1
GRID_SHAPES = [(N, G) for N in (3, 64, 65, 1000) for G in (1, 2, 20, 1024)]


def grid_inputs(name):
    """name: (N, G) of GRID_SHAPES, 'flat_axis' (an axis with M == m) or 'far_outlier' -> (src, tgt, G)."""
    if name == "flat_axis":
        src, tgt = RR.make_case(31, 200, 0.5)[:2]
        src[:, 2] = 0.75
        return src, tgt, 5
    if name == "far_outlier":
        src, tgt = RR.make_case(32, 500, 0.5)[:2]
        src[17], tgt[17] = (1.0e4, -3.0e3, 2.0e3), (-2.0e3, 5.0e3, 1.0e4)  # every other row falls into one cell
        return src, tgt, 20
    N, G = name
    src, tgt = RR.make_case(2000 + N, N, 0.5)[:2]
    return src, tgt, G


# labelling: name -> (N, G, data seed); every size bound of the kernel's split at bound - 1, bound, bound + 1
LABEL_CASES = {f"one_cell_{N}": (N, 1, 3000 + N) for N in (3, 63, 64, 65, 256, 257, 1023, 1024, 1025, 4097)}
LABEL_CASES["one_cell_4097"] = (4097, 1, 7099)  # seeds 7097 and 7098: adjacent d2 closer than 1e-7; replaced
LABEL_CASES["clustered_1000"] = (1000, 4, 3001)
LABEL_CASES["identical_8"] = (8, 20, 3002)
# 0.1 and 1 make a cell of hundreds of rows all-or-nothing (the pairwise term grows with n^2, the unary one with
# n); 0.0005 keeps m* in the interior of the large cells with the pairwise term at work
LABEL_LAMBDAS = (0.0, 0.0005, 0.1, 1.0)


@functools.lru_cache(maxsize=None)
def label_inputs(name):
    """(src, tgt, G, pose): the pose is the planted motion (read by the GPU and by this file as the same bits)."""
    N, G, seed = LABEL_CASES[name]
    if name == "identical_8":
        src, tgt, true, _ = RR.make_case(seed, 1, 1.0, noise=0.05)
        return np.repeat(src, 8, 0), np.repeat(tgt, 8, 0), G, true
    if name == "clustered_1000":  # eight tight clusters: cells of very different sizes
        rng = np.random.RandomState(seed)
        centres = rng.rand(8, 3) * 2.0
        src = (centres[rng.randint(0, 8, N)] + rng.randn(N, 3) * 0.05).astype(np.float32)
        true = RR.rigid(rng.randn(3), 25.0, rng.randn(3) * 0.3)
        tgt = src.astype(np.float64) @ true[:3, :3].T + true[:3, 3] + rng.randn(N, 3) * 0.04
        bad = rng.rand(N) < 0.4
        tgt[bad] += rng.randn(int(bad.sum()), 3) * 0.5
        return src, tgt.astype(np.float32), G, true
    src, tgt, true, _ = RR.make_case(seed, N, 0.5, noise=0.04)
    return src, tgt, G, true


@functools.lru_cache(maxsize=None)
def label_reference(name, lam):
    src, tgt, G, pose = label_inputs(name)
    grid = gc_grid(src, tgt, G)
    return grid, gc_label(pose, src, tgt, grid, EPS, lam)


# solver stages: N = 300, H = 512
# (G = 2: 64 cells, so the LO labels cells of several rows; at the fork's 20 nearly every cell is a singleton)
STAGE = dict(N=300, H=512, ratio=0.3, data_seed=41, seed=7, lam=0.1, G=2)
# whole call: name -> (inlier ratio, rounds, data seed, sampler seed); N = 1000, LO on and off
WHOLE_N, WHOLE_LAMBDA, WHOLE_G = 1000, 0.1, 2
WHOLE_CASES = {"r30_one_round": (0.3, 1, 51, 1), "r30_two_rounds": (0.3, 2, 51, 1),
               "r06_one_round": (0.06, 1, 52, 2), "r06_two_rounds": (0.06, 2, 52, 2)}
EARLY = dict(ratio=0.3, rounds=2, data_seed=51, seed=1, confidence=0.999)


def solver_inputs(N, ratio, data_seed):
    return RR.make_case(data_seed, N, ratio)[:2]


@functools.lru_cache(maxsize=None)
def stage_reference():
    src, tgt = solver_inputs(STAGE["N"], STAGE["ratio"], STAGE["data_seed"])
    return gc_ransac(src, tgt, EPS, STAGE["lam"], G=STAGE["G"], max_iteration=STAGE["H"], seed=STAGE["seed"], lo=True)


@functools.lru_cache(maxsize=None)
def whole_reference(name, lo, confidence=1.0):
    ratio, rounds, data_seed, seed = WHOLE_CASES[name]
    src, tgt = solver_inputs(WHOLE_N, ratio, data_seed)
    return gc_ransac(src, tgt, EPS, WHOLE_LAMBDA, G=WHOLE_G, max_iteration=rounds * ROUND, confidence=confidence, seed=seed,
                     lo=lo, rows=False)
