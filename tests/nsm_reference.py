"""fp64 reference of the forward's back half (NSM weights, seed hypotheses,
post-refinement), the seeded inputs of tests/test_gpu_nsm_stages.py and the
fp32 oracle's own distance from that reference on them.

Everything here is numpy fp64 written from the formulas of include/pdsc.h and
oracle/pdsc_oracle.py (models/PointDSC.py:257-282, :338-358, :403-438,
models/common.py:7-45).  The inputs are fp32 arrays; the reference evaluates
the exact values they hold.  tests/test_nsm_reference.py validates the
reference against the oracle on goldens and asserts every case's
preconditions on the CPU, so a bad seed fails there and not on the GPU."""
import functools

import numpy as np

f32 = np.float32
RANK_BAR = 1e-5          # sigma_2 / sigma_1 of H (conftest.seed_H_rank's bar in test_nsm_chain / test_oracle)
EXCLUDED_CAP = 1e-3      # share of (seed, correspondence) entries allowed inside the near-tie band


def _f64(x):
    return np.asarray(x, np.float64)


def near_tie_delta(*coords):
    """16 * 2^-24 * max|coord|: an fp32 residual (three products, four sums and a
    square root on coordinates of that size) differs from the exact one by less."""
    return 16.0 * 2.0 ** -24 * max(float(np.abs(c).max()) for c in coords)


# ------------------------------------------------------------------ a7-a8
def consistency_fp64(normed, src, tgt, knn, sigma, sigma_d):
    """T = F o S with a zero diagonal (models/PointDSC.py:257-278): [S,k,k]."""
    f = _f64(normed)[knn]
    g = f @ f.transpose(0, 2, 1)
    Fm = np.maximum(1.0 - (1.0 - g) / float(f32(sigma)) ** 2, 0.0)
    s, t = _f64(src)[knn], _f64(tgt)[knn]
    ds = np.sqrt(((s[:, :, None] - s[:, None]) ** 2).sum(-1))
    dt = np.sqrt(((t[:, :, None] - t[:, None]) ** 2).sum(-1))
    Sm = np.maximum(1.0 - (ds - dt) ** 2 / float(f32(sigma_d)) ** 2, 0.0)
    T = Fm * Sm
    k = T.shape[1]
    T[:, np.arange(k), np.arange(k)] = 0.0
    return T


def power_fp64(Tm, T):
    """Every iterate of the power iteration (:347-358) and the allclose margins.
    Returns (iterates [T+1,S,k] with iterates[0] = 1, margins [T,S]):
    margins[t, s] = max_a(|v_{t+1} - v_t| - (1e-8 + 1e-5 |v_t|)); seed s passes
    torch.allclose at iterate t + 1 iff margins[t, s] <= 0."""
    v = np.ones(Tm.shape[:2])
    its, mar = [v], []
    for _ in range(T):
        nv = (Tm @ v[:, :, None])[:, :, 0]
        nv = nv / (np.sqrt((nv * nv).sum(1, keepdims=True)) + 1e-6)
        mar.append((np.abs(nv - v) - (1e-8 + 1e-5 * np.abs(v))).max(1))
        its.append(nv)
        v = nv
    return np.stack(its), np.stack(mar) if mar else np.zeros((0, Tm.shape[0]))


def nsm_fp64(normed, src, tgt, knn, sigma, sigma_d, T):
    """One pair's NSM in fp64: (iterates [T+1,S,k], margins [T,S])."""
    return power_fp64(consistency_fp64(normed, src, tgt, knn, sigma, sigma_d), T)


def weights_of(v):
    """w = v / (sum v + 1e-6) (:280-282)."""
    return v / (v.sum(-1, keepdims=True) + 1e-6)


def exit_band(margins, eps):
    """(lo, hi), 1-based: the first iterate whose worst-seed margin is <= +eps and
    the first whose worst-seed margin is <= -eps (T when none)."""
    T = len(margins)
    worst = margins.max(1) if T else np.zeros(0)
    lo = np.nonzero(worst <= eps)[0]
    hi = np.nonzero(worst <= -eps)[0]
    return (int(lo[0]) + 1 if len(lo) else T), (int(hi[0]) + 1 if len(hi) else T)


# --------------------------------------------------------------------- a9
def kabsch_fp64(A, B, w):
    """rigid_transform_3d (models/common.py:7-45) on [...,n,3] points and [...,n]
    weights: (T [...,4,4], singular values of H [...,3])."""
    A, B, w = _f64(A), _f64(B), np.maximum(_f64(w), 0.0)
    den = w.sum(-1)[..., None, None] + 1e-6
    ca = (A * w[..., None]).sum(-2, keepdims=True) / den
    cb = (B * w[..., None]).sum(-2, keepdims=True) / den
    H = np.swapaxes((A - ca) * w[..., None], -1, -2) @ (B - cb)
    U, sv, Vt = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vt, -1, -2), np.swapaxes(U, -1, -2)
    E = np.zeros(H.shape)
    E[..., 0, 0] = E[..., 1, 1] = 1.0
    E[..., 2, 2] = np.linalg.det(V @ Ut)
    R = V @ E @ Ut
    T = np.zeros(H.shape[:-2] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = cb[..., 0, :] - (R @ np.swapaxes(ca, -1, -2))[..., 0]
    T[..., 3, 3] = 1.0
    return T, sv


def rank_ok(sv):
    return sv[..., 1] / np.maximum(sv[..., 0], 1e-300) > RANK_BAR


# -------------------------------------------------------------------- a10
def residual_fp64(trans, src, tgt):
    """|R src + t - tgt| (:325-327): trans [...,4,4], src/tgt [N,3] -> [...,N]."""
    trans, src, tgt = _f64(trans), _f64(src), _f64(tgt)
    pred = src @ np.swapaxes(trans[..., :3, :3], -1, -2) + trans[..., None, :3, 3]
    return np.sqrt(((pred - tgt) ** 2).sum(-1))


# -------------------------------------------------------------------- a11
def post_refine_fp64(trans, src, tgt, thr):
    """post_refinement (:403-438) of one pair.  Returns (pose, iterations run,
    near-tie distances): an iteration counts the inliers and, unless the count
    repeats, refits; the last holds, per iteration, the smallest | |L2 - thr| |
    over the correspondences."""
    trans, src, tgt, thr = _f64(trans), _f64(src), _f64(tgt), float(f32(thr))
    prev, near = 0, []
    for _ in range(20):
        L2 = residual_fp64(trans, src, tgt)
        near.append(float(np.abs(L2 - thr).min()))
        inl = L2 < thr
        n = int(inl.sum())
        if n == prev:
            break
        prev = n
        w = 1.0 / (1.0 + (L2 / thr) ** 2)
        trans = kabsch_fp64(src[inl], tgt[inl], w[inl])[0]
    return trans, len(near), near


def is_proper_rigid(T, atol=1e-5):
    """assert_rigid's properties without the centroids: finite, R orthonormal, det +1."""
    T = _f64(T)
    R = T[:3, :3]
    return bool(np.isfinite(T).all() and np.abs(R @ R.T - np.eye(3)).max() <= atol
                and abs(np.linalg.det(R) - 1.0) < atol and np.array_equal(T[3], [0, 0, 0, 1]))


# ----------------------------------------------------------------- inputs
def make_pair(rng, N, share=0.4, noise=0.01):
    """src uniform in a cube of side 3; tgt = R src + t + `noise` for about `share`
    of the rows, uniform in the moved cube for the rest.  fp32 (src, tgt, inlier
    mask, ground-truth pose)."""
    src = rng.uniform(0.0, 3.0, (N, 3))
    Q, Rr = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(Rr))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    t = rng.uniform(-1.0, 1.0, 3)
    inl = rng.random(N) < share
    tgt = src @ Q.T + t + noise * rng.standard_normal((N, 3))
    tgt[~inl] = rng.uniform(0.0, 3.0, (int((~inl).sum()), 3)) @ Q.T + t
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Q, t
    return src.astype(f32), tgt.astype(f32), inl, T.astype(f32)


def make_features(rng, N):
    """normalize(cluster_centre + 0.3 noise), unit centres and unit-length noise
    directions: 0.92 inside a cluster, about 0.45 between the four clusters that
    share a base direction, about 0 between the others -- Gram entries from 0 to 1."""
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)  # noqa: E731
    base = unit(rng.standard_normal(128))
    centres = unit(unit(rng.standard_normal((8, 128))) + base * (np.arange(8) < 4)[:, None])
    f = centres[rng.integers(0, 8, N)] + 0.3 * unit(rng.standard_normal((N, 128)))
    return unit(f).astype(f32)


def make_knn(rng, N, S, k, dups):
    """Random rows without repeats; `dups`: every other row repeats its first index."""
    knn = np.stack([rng.permutation(N)[:k] for _ in range(S)]).astype(np.int32)
    if dups and k >= 2:
        knn[::2, 1] = knn[::2, 0]
    return knn


def _id(c, keys):
    return "-".join(f"{n}{c[n]}" for n in keys) + ("-dup" if c.get("dups") else "") + \
        ("-outrow" if c.get("outrow") else "")


# NSM cases: every KC variant and its edges, both exit-rule batch sizes
NSM_KS = (1, 2, 15, 16, 17, 32, 33, 48, 49, 63)
NSM_SHAPES = ((1, 128, 3), (3, 128, 13))
SIGMAS, SIGMA_DS = (0.6, 1.2), (0.1, 1.2)


def _nsm_cases():
    out = []
    for B, N, S in NSM_SHAPES:
        for k in NSM_KS:
            out.append(dict(B=B, N=N, S=S, k=k, T=10))
        for k in (17, 49):
            for T in (0, 1, 31):
                out.append(dict(B=B, N=N, S=S, k=k, T=T))
    for i, c in enumerate(out):
        c.update(sigma=SIGMAS[i % 2], sigma_d=SIGMA_DS[(i // 2) % 2], dups=i % 3 == 0 and c["k"] >= 2,
                 seed=1000 + i)
    # one seed row made only of outliers under a tight sigma_d: T = 0, v = 0, w = 0
    out.append(dict(B=1, N=128, S=3, k=17, T=10, sigma=0.6, sigma_d=1e-3, dups=False, seed=1900, outrow=True))
    for c in out:
        c["id"] = _id(c, ("B", "N", "S", "k", "T"))
    return out


NSM_CASES = _nsm_cases()


@functools.lru_cache(maxsize=None)
def _nsm_case(i):
    c = NSM_CASES[i]
    rng = np.random.default_rng(c["seed"])
    B, N, S, k, T = (c[n] for n in "BNSkT")
    d = dict(c, normed=[], src=[], tgt=[], knn=[])
    its, mar = [], []
    for b in range(B):
        src, tgt, inl, _ = make_pair(rng, N)
        normed, knn = make_features(rng, N), make_knn(rng, N, S, k, c["dups"])
        if c.get("outrow") and b == 0:
            knn[0] = rng.permutation(np.nonzero(~inl)[0])[:k]
        a, m = nsm_fp64(normed, src, tgt, knn, c["sigma"], c["sigma_d"], T)
        for n, v in (("normed", normed), ("src", src), ("tgt", tgt), ("knn", knn)):
            d[n].append(v)
        its.append(a)
        mar.append(m)
    for n in ("normed", "src", "tgt", "knn"):
        d[n] = np.stack(d[n])
    d["iterates"], d["margins"] = np.concatenate(its, 1), np.concatenate(mar, 1)  # [T+1,B*S,k], [T,B*S]
    return d


def nsm_case(c):
    """The inputs and the fp64 iterates / margins of one NSM case (cached: both
    precisions and the CPU test share one evaluation; treat as read-only)."""
    return _nsm_case(NSM_CASES.index(c))


def nsm_oracle(d):
    """The fp32 oracle on a case: (largest deviation of any iterate it computes from
    the fp64 iterate, e_ref = |w_oracle - w_fp64| at the oracle's own exit, that
    exit).  One power iteration over all B * S seeds, as forward_training stacks them."""
    from oracle import pdsc_oracle as O
    T32 = np.concatenate([O.local_consistency(d["normed"][b], d["src"][b], d["tgt"][b], d["knn"][b].astype(np.int64),
                                              d["sigma"], d["sigma_d"]) for b in range(d["B"])])
    dev, it = 0.0, 0
    v = np.ones(T32.shape[:2], f32)
    for n in range(1, d["T"] + 1):
        v, it = O.power_iteration(T32, n)
        dev = max(dev, float(np.abs(v - d["iterates"][it]).max()))
        if it < n:
            break
    w32 = (v / (v.sum(-1, keepdims=True) + f32(1e-6))).astype(f32)
    return dev, float(np.abs(w32 - weights_of(d["iterates"][it])).max()), it


# hypotheses cases: the four launch plans, then small / large k
HYP_CASES = [dict(B=1, N=200, S=20, k=40), dict(B=3, N=257, S=600, k=8), dict(B=512, N=16, S=1, k=8),
             dict(B=8, N=300, S=300, k=17)] + [dict(B=2, N=128, S=9, k=k) for k in (1, 2, 3, 63)]
for _i, _c in enumerate(HYP_CASES):
    _c.update(seed=2000 + _i, dups=_c["k"] == 3, id=_id(_c, ("B", "N", "S", "k")))
HYP_TAUS = (0.1, 0.6)
TIE_LAYOUTS = ((44, 300), (10, 266), (45, 300), (44, 200))  # the issue's two, then across lanes and across waves


@functools.lru_cache(maxsize=None)
def _hyp_case(i):
    c = HYP_CASES[i]
    rng = np.random.default_rng(c["seed"])
    B, N, S, k = (c[n] for n in "BNSk")
    d = dict(c, src=[], tgt=[], knn=[], w=[])
    for b in range(B):
        src, tgt, inl, _ = make_pair(rng, N)
        knn = make_knn(rng, N, S, k, c["dups"])
        # weights that favour the inliers (poses near the truth, informative counts), some exactly zero
        w = rng.random((S, k)) * (0.05 + inl[knn])
        if k >= 4:
            w[:, -1] = 0.0
        w = (w / w.sum(-1, keepdims=True)).astype(f32)
        for n, v in (("src", src), ("tgt", tgt), ("knn", knn), ("w", w)):
            d[n].append(v)
    for n in ("src", "tgt", "knn", "w"):
        d[n] = np.stack(d[n])
    d["delta"] = near_tie_delta(d["src"], d["tgt"])
    ix = np.arange(B)[:, None, None]
    d["T64"], d["sv"] = kabsch_fp64(d["src"][ix, d["knn"]], d["tgt"][ix, d["knn"]], d["w"])
    return d


def hyp_case(c):
    """Inputs, fp64 seed poses and singular values of one hypotheses case (cached, read-only)."""
    return _hyp_case(HYP_CASES.index(c))


def excluded_share(trans, src, tgt, tau, delta):
    """Share of (seed, correspondence) entries of a batch whose fp64 residual lies
    within delta of tau, and the residuals [B,S,N]."""
    res = np.stack([residual_fp64(trans[b], src[b], tgt[b]) for b in range(len(src))])
    return float((np.abs(res - float(f32(tau))) <= delta).mean()), res


# post-refinement cases: five pairs per launch
REFINE_NS, REFINE_THRS = (63, 257, 2049), (0.10, 1.2)
# seeds whose fp64 trajectories keep every correspondence > delta from thr on the pinned pairs, and whose
# offset pair runs 3 (thr 0.10) or 5-6 (thr 1.2) iterations: tests/test_nsm_reference.py asserts it
REFINE_SEEDS = {(63, 0.10): 3000, (63, 1.2): 3013, (257, 0.10): 3001, (257, 1.2): 3002, (2049, 0.10): 3001,
                (2049, 1.2): 3002}
REFINE_CASES = [dict(N=N, thr=thr, id=f"N{N}-thr{thr}") for N in REFINE_NS for thr in REFINE_THRS]
PINNED = (0, 3, 4)  # the pairs whose pose is held to post_refine_fp64


@functools.lru_cache(maxsize=None)
def _refine_case(N, thr, seed):
    rng = np.random.default_rng(seed)
    src, tgt, T0 = [], [], []
    for p in range(5):
        s, t, _, gt = make_pair(rng, N)
        start = gt.copy()
        if p == 1:    # 100 units away: no inlier, the loop stops at once
            start[:3, 3] += 100.0 / np.sqrt(3.0)
        elif p == 2:  # every target but one moved far away
            j = N // 2
            t = (t + 50.0).astype(f32)
            t[j] = (s[j].astype(np.float64) @ gt[:3, :3].astype(np.float64).T + gt[:3, 3]).astype(f32)
        elif p == 3:  # offset by 0.8 thr along a random direction
            u = rng.standard_normal(3)
            start[:3, 3] += (0.8 * thr * u / np.linalg.norm(u)).astype(f32)
        elif p == 4:  # every row an inlier: bounded noise
            t = (s.astype(np.float64) @ gt[:3, :3].astype(np.float64).T + gt[:3, 3]
                 + rng.uniform(-0.01, 0.01, (N, 3))).astype(f32)
        src.append(s)
        tgt.append(t)
        T0.append(start)
    d = dict(N=N, thr=thr, src=np.stack(src), tgt=np.stack(tgt), trans0=np.stack(T0).astype(f32))
    d["delta"] = near_tie_delta(d["src"], d["tgt"])
    d["ref"] = [post_refine_fp64(d["trans0"][p], d["src"][p], d["tgt"][p], thr) for p in range(5)]
    return d


def refine_case(c):
    """Five pairs, their start poses and post_refine_fp64's (pose, iterations, near-tie
    distances) for each (cached, read-only)."""
    return _refine_case(c["N"], c["thr"], REFINE_SEEDS[(c["N"], c["thr"])])


def refine_oracle(d, p):
    """e_ref: the fp32 oracle's post_refinement against post_refine_fp64 on pair p."""
    from oracle import pdsc_oracle as O
    T32, _ = O.post_refinement(d["trans0"][p], d["src"][p], d["tgt"][p], d["thr"])
    return float(np.abs(T32 - d["ref"][p][0]).max())


def refine_bound(d, p, e_ref, envelope):
    t = np.linalg.norm(d["ref"][p][0][:3, 3])
    return min(1e-4, envelope * e_ref + 16.0 * 2.0 ** -24 * max(1.0, t))
