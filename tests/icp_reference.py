"""numpy fp64 restatement of the ICP semantics of include/pdsc.h (f5): open3d's
RegistrationICP with TransformationEstimationPointToPoint(with_scaling=False) and
its default criteria, by brute-force nearest neighbours and np.linalg.svd -- the
yardstick of tests/test_gpu_icp.py, with the diagnostics that say whether a case
is free of near-ties (so the GPU's different fp64 summation order cannot decide a
correspondence or the convergence test the other way)."""
import numpy as np


def transform(T, p):
    """q = R p + t per point in fp64, in the library's order: (T0 x + T1 y) + T2 z + T3."""
    p = np.asarray(p, np.float64)
    T = np.asarray(T, np.float64)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    return (T[None, :3, 0] * x + T[None, :3, 1] * y) + T[None, :3, 2] * z + T[None, :3, 3]


def evaluate(src, tgt, T, r):
    """(corr [Ns] int32: nearest target index within d^2 <= r^2 -- ties to the lower
    index -- or -1; d2 [Ns] of the chosen one; fitness; inlier_rmse; gap: the
    smallest relative gap between a point's best and second-best d^2; margin: the
    smallest |d^2 - r^2| / r^2 over every pair)."""
    qa = transform(T, src)
    t = np.asarray(tgt, np.float64)
    r2 = float(r) * float(r)
    best, bd = np.empty(len(qa), np.int64), np.empty(len(qa))
    gap = margin = np.inf
    for s in range(0, len(qa), 512):  # source blocks: [512, Nt] at a time
        q = qa[s:s + 512]
        dx, dy, dz = (t[None, :, c] - q[:, None, c] for c in range(3))
        d2 = dx * dx + dy * dy + dz * dz
        b = np.argmin(d2, 1)  # the first (lowest) index of the minimum
        best[s:s + 512], bd[s:s + 512] = b, d2[np.arange(len(q)), b]
        if d2.shape[1] > 1:
            two = np.partition(d2, 1, 1)[:, :2]
            sel = two[:, 0] <= r2 * (1 + 1e-6)  # only where a correspondence is (nearly) taken
            if sel.any():
                gap = min(gap, float(((two[sel, 1] - two[sel, 0]) / np.maximum(two[sel, 1], 1e-300)).min()))
        margin = min(margin, float((np.abs(d2 - r2) / r2).min()))
    ok = bd <= r2
    corr = np.where(ok, best, -1).astype(np.int32)
    n = int(ok.sum())
    fitness = n / len(qa)
    rmse = float(np.sqrt(bd[ok].sum() / n)) if n else 0.0
    return corr, bd, fitness, rmse, gap, margin


def kabsch(A, B):
    """The rigid update [4,4] taking points A onto B (unit weights, fp64,
    R = V diag(1, 1, det(V U^T)) U^T); identity without points."""
    U4 = np.eye(4)
    if len(A) == 0:
        return U4
    ma, mb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((A - ma).T @ (B - mb))
    V = Vt.T
    R = V @ np.diag([1.0, 1.0, np.linalg.det(V @ U.T)]) @ U.T
    U4[:3, :3], U4[:3, 3] = R, mb - R @ ma
    return U4


def registration_icp(src, tgt, r, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """dict: transformation [4,4] fp64, fitness, inlier_rmse, iterations, n_corr,
    correspondence, and the diagnostics min_gap, min_margin (over every
    evaluation), d_fitness / d_rmse (per iteration)."""
    T = np.eye(4) if init is None else np.array(init, np.float64)
    corr, bd, fit, rmse, gap, margin = evaluate(src, tgt, T, r)
    out = dict(iterations=0, min_gap=gap, min_margin=margin, d_fitness=[], d_rmse=[])
    tgt64 = np.asarray(tgt, np.float64)
    for it in range(max_iteration):
        ok = corr >= 0
        update = kabsch(transform(T, src)[ok], tgt64[corr[ok]])
        T = update @ T if ok.any() else T
        corr, bd, nfit, nrmse, gap, margin = evaluate(src, tgt, T, r)
        out["iterations"] = it + 1
        out["min_gap"], out["min_margin"] = min(out["min_gap"], gap), min(out["min_margin"], margin)
        df, dr = abs(fit - nfit), abs(rmse - nrmse)
        out["d_fitness"].append(df)
        out["d_rmse"].append(dr)
        fit, rmse = nfit, nrmse
        if df < relative_fitness and dr < relative_rmse:
            break
    out.update(transformation=T, fitness=fit, inlier_rmse=rmse, n_corr=int((corr >= 0).sum()), correspondence=corr)
    return out


def tie_free(ref, rel=1e-9):
    """The preconditions of a comparison against another fp64 summation order:
    every nearest / second-nearest gap and every radius margin above `rel`, every
    per-iteration |delta fitness| and |delta rmse| below 0.5e-6 or above 2e-6."""
    d = np.array(ref["d_fitness"] + ref["d_rmse"], np.float64)
    return bool(ref["min_gap"] > rel and ref["min_margin"] > rel and np.all((d < 0.5e-6) | (d > 2e-6)))


# ---------------------------------------------------------------- test inputs
def rigid(axis, angle_deg, t):
    """[4,4] fp64: the rotation by angle_deg about axis, then the translation t."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(angle_deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def make_case(seed, ns, nt):
    """The GPU tests' inputs (fixed seed): src uniform in a 2 m cube; tgt = the true
    motion of src (cycled or cut to nt points) + 2 mm Gaussian noise, shuffled, 30 %
    of it replaced by uniform outliers; init = the true motion perturbed by about
    2 degrees and 3 cm.  Returns (src fp32 [ns,3], tgt fp32 [nt,3], init fp64 [4,4],
    true fp64 [4,4])."""
    rng = np.random.RandomState(seed)
    src = (rng.rand(ns, 3) * 2.0).astype(np.float32)
    true = rigid(rng.randn(3), 25.0, rng.randn(3) * 0.5)
    moved = transform(true, src)
    tgt = moved[np.arange(nt) % ns] + rng.randn(nt, 3) * 0.002
    if nt > ns:  # the appended points are outliers, not second copies
        tgt[ns:] = moved.min(0) + rng.rand(nt - ns, 3) * (moved.max(0) - moved.min(0) + 1e-3)
    tgt = tgt[rng.permutation(nt)]
    out = rng.rand(nt) < 0.3
    lo, hi = moved.min(0), moved.max(0)
    tgt[out] = lo + rng.rand(int(out.sum()), 3) * (hi - lo + 1e-3)
    d = rng.randn(3)
    init = rigid(rng.randn(3), 2.0, 0.03 * d / np.linalg.norm(d)) @ true
    return src, tgt.astype(np.float32), init, true


def pose_error(T, true):
    """(rotation error in degrees, translation error)."""
    R = T[:3, :3].T @ true[:3, :3]
    return (float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))),
            float(np.linalg.norm(T[:3, 3] - true[:3, 3])))
