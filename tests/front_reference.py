"""Exact references, case tables and input builders for the forward's front half:
a1 compat (compat.hip), a5 seeds (seeds.hip), a6 seed kNN (knn_dist* / knn_select
of knn.hip) and f1 correspondences (corr.hip) -- the index, mask and bit-exact
stages.  tests/test_gpu_front_stages.py runs the cases on the GPU;
tests/test_front_reference.py proves on the CPU that the references and the cases
are what they claim, so a bad seed or a misread path fails there.

numpy only (no torch device code).  The truth is the oracle (oracle/pdsc_oracle.py,
pinned to the reference's goldens) for everything bit-exact, and fp64 evaluated on
the fp32 inputs for the kNN distances.  Which kernel form a shape reaches is read
from the launchers (seeds.hip plan_tail, knn.hip launch_knn_dist /
launch_knn_select, compat.hip) and restated beside each table."""
import functools

import numpy as np

from oracle import pdsc_oracle as O

f32 = np.float32


def _f64(x):
    return np.asarray(x, np.float64)


# ===================================================================== a1 compat
# N % 4 decides dense vector vs scalar stores; ceil(N / 32) odd and even; the last
# 64-block full (64, 128), half (96), one row (65, 129) and one 32-tile + 1 (33, 97).
COMPAT_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191)
COMPAT_SIGMA = 0.1
MPACK_T = 32


def compat_pairs(N, seed=0, dups=0):
    """B = 2 pairs of N correspondences in a 1 m cube: ~60 % follow a rigid motion
    with 3 cm noise (M spread over (0, 1]), the rest are random (M mostly 0).
    dups: the last `dups` points repeat the first ones (exact zero distances)."""
    rng = np.random.RandomState(1000 * N + seed)
    src = rng.rand(2, N, 3).astype(f32)
    tgt = rng.rand(2, N, 3).astype(f32)
    for b in range(2):
        inl = rng.rand(N) < 0.6
        th = rng.rand() * np.pi
        Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
        tgt[b, inl] = (src[b, inl] @ Rz.T + 0.3 + 0.03 * rng.randn(int(inl.sum()), 3)).astype(f32)
        if dups:
            src[b, N - dups:] = src[b, :dups]
            tgt[b, N - dups:] = tgt[b, :dups]
            tgt[b, N - 1] = tgt[b, 1]  # one duplicate in tgt only
    return src, tgt


def packed_floats(N):
    """pdsc_compat_packed_floats: nt (nt + 1) / 2 tiles of 32 x 32, nt = ceil(N / 32)."""
    nt = (N + MPACK_T - 1) // MPACK_T
    return nt * (nt + 1) // 2 * MPACK_T * MPACK_T


def packed_offset(i, j, N):
    """include/pdsc.h: where M[i][j] sits in the packed buffer of one pair.  Tile
    (ti, tj), ti <= tj, is block ti*nt - ti*(ti-1)/2 + (tj - ti), row-major 32 x 32;
    M[i][j] for i > j is element (j % 32, i % 32) of tile (j / 32, i / 32)."""
    nt = (N + MPACK_T - 1) // MPACK_T
    if i > j:
        i, j = j, i
    ti, tj = i // MPACK_T, j // MPACK_T
    block = ti * nt - ti * (ti - 1) // 2 + (tj - ti)
    return block * MPACK_T * MPACK_T + (i % MPACK_T) * MPACK_T + (j % MPACK_T)


def pack_symmetric(M):
    """The packed buffer a symmetric M [N,N] must produce: every upper-triangle tile
    whole (a diagonal tile carries both of its triangles), entries past N +0."""
    N = M.shape[0]
    nt = (N + MPACK_T - 1) // MPACK_T
    P = np.zeros((nt * MPACK_T, nt * MPACK_T), M.dtype)
    P[:N, :N] = M
    out = np.zeros(packed_floats(N), M.dtype)
    blk = 0
    for ti in range(nt):
        for tj in range(ti, nt):
            out[blk * 1024:(blk + 1) * 1024] = P[ti * 32:(ti + 1) * 32, tj * 32:(tj + 1) * 32].reshape(-1)
            blk += 1
    return out


# The packed kernel's zero proof (compat.hip compat_n): M = 0 is taken without a
# square root when (xs - xt)^2 > 2 s2 (xs + xt)(1 + 2^-10) and xs + xt <= 2^20 s2.
ZERO_PROOF_SIGMAS = (0.1, 1.2)
ZERO_PROOF_N = 64
_DELTAS = (0.0, 2.0 ** -12, -2.0 ** -12, 2.0 ** -10, -2.0 ** -10, 2.0 ** -8, -2.0 ** -8, 2.0 ** -6, -2.0 ** -6)


def zero_proof_pair(sigma):
    """One pair on the x axis with |ds - dt| of row 0 = sigma (1 + delta_j): point 0 at
    the origin of both clouds, s_j = (r_j, 0, 0), t_j = (r_j + sigma (1 + delta_j), 0, 0),
    r_j / sigma log-spaced over [1e-3, 4e3] (xs + xt crosses 2^20 sigma^2 near 724)."""
    N = ZERO_PROOF_N
    r = sigma * np.logspace(-3, np.log10(4e3), N - 1)
    d = np.array([_DELTAS[j % len(_DELTAS)] for j in range(N - 1)])
    src = np.zeros((1, N, 3), f32)
    tgt = np.zeros((1, N, 3), f32)
    src[0, 1:, 0] = r
    tgt[0, 1:, 0] = r + sigma * (1.0 + d)
    return src, tgt


# sigma_d^2 subnormal / >= 1e30: the kernels' s2ok == false branch (library sqrtf, '/')
SIGMA_OUTSIDE = (1e-20, 1e16)
SIGMA_OUTSIDE_N = 65


def compat_reference(src, tgt, sigma_d):
    """[B,N,N]: the oracle per pair."""
    return np.stack([O.compat(src[b], tgt[b], sigma_d) for b in range(len(src))])


# ====================================================================== a5 seeds
SEED_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049)
SEED_BS = (1, 3)  # B = 1: local_max_kernel<16>; B = 3: local_max_rows_kernel<16, 2>
SEED_RADIUS = 0.1


def seed_counts(N):
    return sorted({1, max(1, N // 10), N})


def _cloud(rng, N, per_ball=3.0, R=SEED_RADIUS):
    """N points in a cube sized for ~per_ball neighbours inside radius R."""
    side = (N * 4.18879 * R ** 3 / per_ball) ** (1.0 / 3.0)
    return (rng.rand(N, 3) * max(side, 2 * R)).astype(f32)


def _mixed_conf(rng, N):
    """Heavy ties (multiples of 1/4 in [-1, 1]), both zeros, negative maxima."""
    c = (rng.randint(-4, 5, N) / 4.0).astype(f32)
    z = np.nonzero(c == 0)[0]
    c[z[::2]] = f32(-0.0)
    return c


@functools.lru_cache(maxsize=None)
def seed_case(B, N):
    """src [B,N,3], conf [B,N].  Pair 0 (every B): duplicate points, heavy score
    ties, +-0, negative maxima.  B = 3 adds pair 1 with all confidences equal (every
    point a local maximum, the list 0 .. S-1) and pair 2 with -inf confidences on
    isolated points (a -inf that were no local maximum would score -inf * 0 = NaN,
    for which no order is defined: test_front_reference asserts there is none)."""
    rng = np.random.RandomState(7919 * N + B)
    src = np.stack([_cloud(rng, N) for _ in range(B)])
    conf = np.stack([_mixed_conf(rng, N) for _ in range(B)])
    nd = N // 8
    if nd:
        src[0, N - nd:] = src[0, :nd]  # duplicate points, some with equal, some with other confidences
        conf[0, N - nd:N - nd // 2] = conf[0, :nd - nd // 2]
    if B >= 3:
        conf[1] = f32(0.375)
        ninf = max(1, N // 8) if N >= 2 else 0
        far = N - 1 - np.arange(ninf)
        src[2, far] = (100.0 + 2.0 * np.arange(ninf))[:, None].astype(f32)
        if ninf >= 2:
            src[2, far[1]] = src[2, far[0]]  # two -inf points on one spot
        conf[2, far] = -np.inf
    return src, conf


def rank_scores(scores, S):
    """sorted(range(N), key=lambda i: (-score_i, i))[:S] on fp32 scores; -0 and +0
    tie (numpy's sort compares values).  No NaN may be present."""
    scores = np.asarray(scores, f32)
    assert not np.isnan(scores).any()
    return np.lexsort((np.arange(len(scores)), -scores))[:S].astype(np.int64)


def seed_reference(src, conf, radius, S):
    """One pair: (seeds [S], is_local_max [N]).  Flags: the oracle's sqrtf form;
    list: rank_scores of fp32 conf * lm."""
    lm = O.local_max(src, conf, radius)
    with np.errstate(invalid="ignore"):
        scores = (np.asarray(conf, f32) * lm).astype(f32)
    return rank_scores(scores, S), lm


# Forms reached by shape under the default knobs (seeds.hip plan_tail): columns of
# pdsc_launch_plan's out[6], out[7], out[8] = seed_rows, nms_rpt, seed_rank.
#   seed_rows 64 <=> B ceil(N / 64) >= 1024;  nms_rpt 2 <=> B > 1 on 16-row blocks;
#   rank select (2; 3 = split, from S > 256) <=> B N^2 >= 1e8 and sel_lds(N) <= 64 KiB.
SEED_PLAN_CASES = (
    dict(id="B1024-N33-S3", B=1024, N=33, S=3, plan=(64, 1, 0)),
    dict(id="B1600-N250-S25", B=1600, N=250, S=25, plan=(64, 1, 2)),
    dict(id="B400-N513-S51", B=400, N=513, S=51, plan=(64, 1, 2)),
    # more than SEL_CMAX candidates above the threshold: seed_select_kernel's compare
    # fallback (the standalone entry has no scratch, so the split plan runs in one launch)
    dict(id="B1-N10000-S4000", B=1, N=10000, S=4000, plan=(16, 1, 3)),
)
SEL_CMAX = 2048


def sel_lds(N):
    """seeds.hip sel_lds: keys + candidates of seed_select_kernel in LDS bytes."""
    return ((N + 1) & ~1) * 4 + SEL_CMAX * 12


def plan_ratio(N, S):
    """A cfg.ratio with int(N * ratio) == S."""
    r = (S + 0.5) / N
    assert int(N * r) == S
    return r


@functools.lru_cache(maxsize=None)
def seed_plan_case(B, N, S):
    """Big-batch inputs: sparse clouds (most points local maxima), scores with ties.
    The N = 10000 pair has distinct positive confidences, so S - 1 > SEL_CMAX
    candidates lie above the S-th score."""
    rng = np.random.RandomState(31 * B + N)
    src = np.stack([_cloud(rng, N, per_ball=1.0) for _ in range(B)])
    if N == 10000:
        conf = (rng.permutation(N)[None] + 1).astype(f32) / f32(N)
    else:
        conf = (rng.randint(-8, 25, (B, N)) / 8.0).astype(f32)
    return src, conf


def candidates_above(scores, S):
    """A of seed_select_kernel: scores strictly above the S-th largest."""
    s = np.sort(np.asarray(scores, f32))[::-1]
    return int((scores > s[S - 1]).sum())


RADIUS_N, RADIUS_B = 129, 2
RADIUS_CASES = ("zero", "lattice", "tiny", "huge")
LATTICE_R = 0.125


@functools.lru_cache(maxsize=None)
def radius_case(name):
    """(src [2,129,3], conf [2,129], R).
    zero     R = 0: every distance >= R.
    lattice  R = 0.125 on a 2^-6 lattice (248 x 2 x 2 cells): squared distances are
             exact multiples of 2^-12, many pairs exactly 8 cells apart along x
             (distance == R) and others at 7, 9 and sqrt(65) cells.
    tiny     R = 1e-30 (R^2 underflows; sqrt_ge_threshold gives the smallest
             subnormal): points 1e-25 apart (squared distance underflows to 0:
             inside) and 1e-20 apart (subnormal squared distance: outside).
    huge     R = 1e30 (R^2 overflows; threshold +inf): every pair is inside."""
    rng = np.random.RandomState(RADIUS_CASES.index(name) + 77)
    B, N = RADIUS_B, RADIUS_N
    conf = rng.permutation(B * N).reshape(B, N).astype(f32) / f32(B * N) - f32(0.25)
    if name == "lattice":
        src = np.zeros((B, N, 3), f32)
        for b in range(B):
            cells = rng.permutation(240 * 2 * 2)[:N]
            xyz = np.stack([cells // 4, (cells // 2) % 2, cells % 2], 1)
            xyz[50:100] = xyz[:50] + [8, 0, 0]  # 50 partners exactly R away
            src[b] = xyz.astype(f32) * f32(2.0 ** -6)
        return src, conf, LATTICE_R
    src = np.stack([_cloud(rng, N) for _ in range(B)])
    if name == "tiny":
        e25, e20 = f32(1e-25), f32(1e-20)
        cl = np.array([[0, 0, 0], [e25, 0, 0], [0, e25, 0], [0, 0, e25], [e20, 0, 0], [0, e20, 0], [0, 0, e20],
                       [e20, e25, 0]], f32)
        for b in range(B):
            at = rng.permutation(N)[:len(cl)]
            src[b] += f32(1.0)  # the cluster alone sits at the origin
            src[b, at] = cl
        return src, conf, 1e-30
    return src, conf, {"zero": 0.0, "huge": 1e30}[name]


def local_max_strict(src, conf, radius):
    """The NMS with the equality removed from `dist >= R` (what a `>` kernel computes)."""
    D = O.src_dist(src)
    c = np.asarray(conf, f32)
    return ((c[:, None] >= c[None, :]) | (D > f32(radius))).all(1).astype(f32)


ISOLATION = dict(B=3, N=257, S=25)


@functools.lru_cache(maxsize=None)
def isolation_case():
    """B = 3, N = 257; pair 1's confidences are all NaN."""
    src, conf = (x.copy() for x in seed_case(3, 257))
    conf[1] = np.nan
    return src, conf


# =================================================================== a6 seed kNN
KNN_EPS = 2e-6  # conftest.assert_knn_equivalent's bar: the H3 distance error is <= 2^-21 (knn.hip)
C = 128


def _k(**kw):
    kw.setdefault("dups", 0)
    kw.setdefault("dups2", 0)
    kw.setdefault("tag", "")
    kw["id"] = "B{B}-N{N}-S{S}-k{k}".format(**kw) + (f"-dup{kw['dups']}" if kw["dups"] else "") + kw["tag"]
    return kw


# Paths (knn.hip): knn_select_kernel<R>, R = 16 ceil(N / 1024) up to N = 8192, then
# the memory form <0>.  In <R > 0> lane l owns keys 256 i + 4 l + e, so N <= 4 (k + 1)
# leaves fewer than k + 1 lanes with a key: tau0 is all-ones and every key qualifies
# (c = N): bitonic ranking to N = 64, readlane ranking to 128, register radix select
# for 129 .. 160 at k = 40; N = 161 is the first with 41 owning lanes.  Rows are
# loaded by 16-B buffer loads when N % 4 == 0, else dword loads.  knn_dist: 32 seeds
# per wave, 128 per workgroup, rows past S clipped by the buffer resource; 5 key tiles
# per workgroup once ceil(ceil(N/32) / 5) ceil(S / 128) B >= 256, else 1.
KNN_CASES = (
    [_k(B=1, N=2, S=1, k=1), _k(B=2, N=41, S=4, k=40), _k(B=1, N=64, S=7, k=63)]
    + [_k(B=1, N=n, S=5, k=40) for n in (65, 128, 129, 160, 161, 165, 257)]
    + [_k(B=1, N=n, S=9, k=63) for n in (1000, 1001, 1023, 1024, 1025)]
    + [_k(B=1, N=n, S=5, k=40) for n in (2048, 2049)]
    + [_k(B=2, N=300, S=s, k=8) for s in (1, 31, 32, 33, 127, 128, 129, 130)]
    + [_k(B=16, N=300, S=129, k=40),   # B ceil(S / 4) >= 512: 4 seeds per workgroup, the last one partial
       _k(B=19, N=1001, S=129, k=40),  # wg5 = 7 * 2 * 19 = 266 >= 256: 5 key tiles per workgroup, the last short
       _k(B=1, N=8200, S=4, k=63),
       # 300 duplicates of seed 0's row: every lane's minimum is the tie key, 301 keys
       # qualify (> KNN_FASTCAP): memory radix select down to the last digit, the
       # first k + 1 of the tie group in index order
       _k(B=1, N=8200, S=4, k=63, dups=300),
       # 50 duplicates confined to 8 lanes (index % 64 < 8) so tau0 is not the tie key,
       # plus 200 copies of a row at distance ~0.02 in every lane: tau0 is that key, 251
       # keys qualify, and the radix select's first digit isolates the 51-key tie
       # group: need 41 of a 51-key bin (<= KNN_BINCAP): the small-bin branch.  (50
       # duplicates alone stay on the fast path: at most ~115 keys qualify.)
       _k(B=1, N=8200, S=4, k=40, dups=50, dups2=200),
       _k(B=1, N=161, S=3, k=40, dups=140)])


def knn_wg5(B, N, S):
    """launch_knn_dist's rule (knn.hip): workgroups at 5 key tiles each."""
    nkt = (N + 31) // 32
    return ((nkt + 4) // 5) * ((S + 127) // 128) * B


@functools.lru_cache(maxsize=None)
def _knn_case(cid):
    c = next(x for x in KNN_CASES if x["id"] == cid)
    B, N, S, k = (c[n] for n in "BNSk")
    rng = np.random.RandomState(N * 131 + S * 7 + k + c["dups"])
    f = rng.randn(B, N, C).astype(f32)
    f /= np.linalg.norm(f, axis=-1, keepdims=True)
    f = f.astype(f32)
    seeds = np.zeros((B, S), np.int64)
    groups = []
    for b in range(B):
        group = np.zeros(0, np.int64)
        if c["dups"]:
            pool = np.arange(1, N)
            if c["dups2"]:
                pool = pool[pool % 64 < 8]
            group = np.sort(np.concatenate([[0], rng.choice(pool, c["dups"], replace=False)]))
            f[b, group] = f[b, 0]
            if c["dups2"]:
                rest = np.setdiff1d(np.arange(N), group)
                g2 = rng.choice(rest, c["dups2"], replace=False)
                near = f[b, 0].astype(np.float64) + 0.1 * rng.randn(C) / np.sqrt(C)
                f[b, g2] = (near / np.linalg.norm(near)).astype(f32)
        r = int(group[len(group) // 2]) if len(group) else int(rng.randint(N))
        base = [0, N - 1, r, r] + list(rng.randint(0, N, max(S - 4, 0)))
        seeds[b] = base[:S]
        groups.append(group)
    return dict(normed=f, seeds=seeds, groups=groups)


def knn_case(c):
    """normed [B,N,128] unit rows, seeds [B,S] (index 0, index N-1, one index twice,
    then random), groups: per pair the sorted indices that share seed 0's row (the
    repeated seed is one of them, so a lower-indexed duplicate is dropped for it)."""
    return _knn_case(c["id"])


def knn_d64(normed_b, seed):
    """d_j = 2 - 2 f_s . f_j in fp64 from the fp32 features."""
    f = _f64(normed_b)
    return 2.0 - 2.0 * (f @ f[seed])


def check_knn_row(row, d64, k, eps=KNN_EPS):
    """One returned row against the fp64 distances of its seed.  Both precisions are
    within eps / 2 of d64, so: k distinct entries of [0, N) in ascending order up to
    eps; none beyond the (k+1)-th smallest distance D[k] by more than eps; and every
    index surely inside (d64 < D[k] - eps) is present except the one dropped
    positionally, which is a nearest one (d64 <= D[0] + eps).  Where the nearest is
    itself within 2 eps of D[k] (a tie group spanning all k + 1 places -- planted
    duplicates only) it need not be in the sure set: then at most one is absent."""
    row = np.asarray(row, np.int64)
    N = len(d64)
    assert row.shape == (k,), row.shape
    assert ((row >= 0) & (row < N)).all(), f"entries outside [0, {N}): {row[(row < 0) | (row >= N)]}"
    assert len(np.unique(row)) == k, "repeated index"
    dr = d64[row]
    assert (np.diff(dr) >= -eps).all(), f"order not ascending: step {np.diff(dr).min():.3g}"
    D = np.sort(d64)
    assert (dr <= D[k] + eps).all(), f"entry {(dr - D[k]).max():.3g} beyond the (k+1)-th distance"
    sure = np.nonzero(d64 < D[k] - eps)[0]
    absent = np.setdiff1d(sure, row)
    if D[0] + eps < D[k] - eps:
        assert len(absent) == 1, f"{len(absent)} of the surely-inside indices absent (expected the dropped one)"
    else:
        assert len(absent) <= 1, f"{len(absent)} of the surely-inside indices absent"
    if len(absent):
        assert d64[absent[0]] <= D[0] + eps, "the absent index is not a nearest one"


def tie_group_row(group, k):
    """The row's leading entries when `group` (sorted, >= 2 indices, the seed among
    them) shares the seed's feature row: equal fp32 distances below every other, so
    index order decides and the lowest index is the one dropped."""
    return np.asarray(group[1:k + 1], np.int64)


# ============================================================ f1 correspondences
NN_MARGIN = 1e-5  # fp32 summation reordering at D = 32 moves a dot by ~2e-6


def corr_pair(Ns, Nt, D, seed, overlap=0.6, noise=0.05):
    """Keypoints and unit descriptors with a planted overlap (the generator of
    tests/test_correspondence.py): (src, tgt, sd, td, gt)."""
    rng = np.random.RandomState(seed)
    src = (rng.rand(Ns, 3) * 3).astype(f32)
    th = rng.rand() * np.pi
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = R, rng.rand(3)
    sd = rng.randn(Ns, D).astype(f32)
    sd /= np.linalg.norm(sd, axis=1, keepdims=True)
    tgt = (rng.rand(Nt, 3) * 3).astype(f32)
    td = rng.randn(Nt, D).astype(f32)
    m = min(int(overlap * min(Ns, Nt)), Nt)
    perm = rng.permutation(Nt)[:m]
    tgt[perm] = (src[:m] @ R.T + gt[:3, 3] + 0.01 * rng.randn(m, 3)).astype(f32)
    td[perm] = sd[:m] + noise * rng.randn(m, D).astype(f32)
    td /= np.linalg.norm(td, axis=1, keepdims=True)
    return src, tgt, sd, td.astype(f32), gt


def nn_margin(sd, td):
    """(row gaps [Ns], column gaps [Nt]): for every row and column of the fp32 matrix
    2 - 2 sd td^T (the argument of the distance's sqrt, which amplifies error near
    0), the gap between its smallest and second-smallest entry; inf where there is
    one entry only."""
    d = (f32(2) - f32(2) * (np.asarray(sd, f32) @ np.asarray(td, f32).T)).astype(f32)

    def gaps(m):
        if m.shape[1] < 2:
            return np.full(m.shape[0], np.inf)
        p = np.partition(m, 1, axis=1)
        return (p[:, 1].astype(np.float64) - p[:, 0].astype(np.float64))

    return gaps(d), gaps(d.T)


def min_margin(sd, td):
    r, c = nn_margin(sd, td)
    return float(min(r.min(), c.min()))


# (Ns, Nt) -> corr_pair seed with min_margin >= NN_MARGIN (found by search; asserted
# in test_front_reference).  D = 32.
CORR_ORACLE_SEEDS = {(1000, 900): 0, (5000, 5000): 2}
# (Ns, Nt, D) -> seed, the edge shapes: D = 1 and 64, a 64-tile boundary either way,
# corr_select_kernel's 1024-row scan chunk.
CORR_EDGE_SEEDS = {(1, 1, 1): 0, (1, 65, 64): 0, (63, 64, 33): 0, (65, 63, 32): 0, (1023, 70, 32): 1,
                   (1024, 70, 32): 0, (1025, 70, 32): 0}


@functools.lru_cache(maxsize=None)
def single_mutual_pair():
    """(200, 180, 32) with the fewest mutual pairs possible.  A set with none cannot
    be built: the first smallest entry (i0, j0) of the distance matrix in row-major
    order is the first minimum of its row and of its column, so it is always mutual.
    Every source descriptor sits within ~0.3 of u = target 0 and every other target
    near -u: each row picks column 0, and only column 0's own pick is mutual."""
    rng = np.random.RandomState(0)
    Ns, Nt, D = 200, 180, 32
    u = rng.randn(D)
    u /= np.linalg.norm(u)
    sd = u + 0.3 * rng.randn(Ns, D) / np.sqrt(D)
    td = -u + 0.3 * rng.randn(Nt, D) / np.sqrt(D)
    td[0] = u
    sd = (sd / np.linalg.norm(sd, axis=1, keepdims=True)).astype(f32)
    td = (td / np.linalg.norm(td, axis=1, keepdims=True)).astype(f32)
    src, tgt = (rng.rand(Ns, 3) * 3).astype(f32), (rng.rand(Nt, 3) * 3).astype(f32)
    return src, tgt, sd, td


@functools.lru_cache(maxsize=None)
def straddle_ties():
    """Ns = 40, Nt = 65, D = 32: target 64 repeats target 63 (either side of the
    64-column tile edge) and target 5 (a far column of the first tile); sources 0..9
    sit next to target 63's descriptor, 10..19 next to target 5's.  Returns a list of
    (sd, td, rows, expect): nn_src[rows] must be `expect`, the lower index."""
    rng = np.random.RandomState(12)
    sd = rng.randn(40, 32)
    td = rng.randn(65, 32)
    td /= np.linalg.norm(td, axis=1, keepdims=True)
    sd[:10] = td[63] + 0.02 * rng.randn(10, 32)
    sd[10:20] = td[5] + 0.02 * rng.randn(10, 32)
    sd /= np.linalg.norm(sd, axis=1, keepdims=True)
    sd, td = sd.astype(f32), td.astype(f32)
    a, b = td.copy(), td.copy()
    a[64], b[64] = td[63], td[5]
    return [(sd, a, np.arange(10), 63), (sd, b, np.arange(10, 20), 5)]
