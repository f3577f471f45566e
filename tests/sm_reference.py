"""The spectral-matching baseline (baseline_scripts/baseline_3DMatch.py:19-53,
pointdsc_amd/csrc/sm.hip) restated in numpy, the inputs of
tests/test_gpu_sm_stages.py and numpy models of sm_select_kernel's tie rule.

    matrix   M in fp32, in the contract's operation order (include/pdsc.h f3)
    iterate  v <- M v / (|M v| + 1e-6) from v = 1: fp64, or fp32 with the columns
             summed in a permuted order (one more fp32 realisation)
    select   the S largest entries of v, ties to the lower index, -0 == +0
    noise    the fp32 noise of the iterate on a given M

tests/test_sm_reference.py pins these against oracle/pdsc_oracle.py and asserts every
case's preconditions on the CPU, so a bad seed fails there and not on the GPU."""
import functools

import numpy as np

f32 = np.float32
NOISE_SEEDS = 4

# every size stands for one boundary of sm.hip (64 x 64 tiles, 16-B stores and loads
# when N % 4 == 0, 256 elements per wave step of the vector matvec, 1024-thread
# normalize / select)
SIZES = (1, 2, 3, 4,              # below one wave
         9, 10,                   # S = int(N * 0.1) = 0 and 1
         63, 64, 65, 67,          # tile edge, scalar path
         128, 130,                # second tile
         252, 256, 260, 257,      # the vector matvec's 256-element step; the same size on the scalar path
         1023, 1024, 1025, 1028,  # the 1024 stride of normalize and select, both paths
         2050)                    # more than two chunks
PRESET_THR = {"3dmatch": 0.10, "kitti": 0.60}
CASES = [(N, "3dmatch") for N in SIZES] + [(67, "kitti"), (1028, "kitti")]
ITERS = (1, 10)
TOP_RATIO = 0.1


def case_id(c):
    return f"N{c[0]}-{c[1]}"


# ------------------------------------------------------------ the restatement
def _norms(a):
    """|a_j - a_i| [N,N] in fp32: ((dx dx + dy dy) + dz dz), then sqrt."""
    dx = a[None, :, 0] - a[:, None, 0]
    dy = a[None, :, 1] - a[:, None, 1]
    dz = a[None, :, 2] - a[:, None, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def matrix(corr, thr):
    """M [N,N] fp32 (:20-36): sigma = thr / 3 and sigma^2 in double, the tensor divided
    by the fp32 value of sigma^2; m m / 2 / sigma^2 left to right; the diagonal +0."""
    c = np.ascontiguousarray(corr, f32)
    m = _norms(c[:, 0:3]) - _norms(c[:, 3:6])
    sigma = float(thr) / 3.0
    sig2 = f32(sigma * sigma)
    M = np.maximum(f32(0), f32(4.5) - ((m * m) / f32(2)) / sig2)
    assert M.dtype == f32
    np.fill_diagonal(M, f32(0))
    return M


def iterate(M, iters, dtype=np.float64, perm=None):
    """`iters` power iterates from v = 1 (:39-43) in `dtype`; perm: the column order of
    every row's sum (fp32: another summation order, as another fp32 kernel might have)."""
    M = np.asarray(M, dtype)
    if perm is not None:
        M = np.ascontiguousarray(M[:, perm])
    v = np.ones(M.shape[0], dtype)
    for _ in range(iters):
        y = M @ (v if perm is None else v[perm])
        v = y / (np.sqrt(np.sum(y * y, dtype=dtype)) + dtype(1e-6))
        assert v.dtype == dtype
    return v


def noise(M, iters):
    """max |fp32 re-ordered - fp64| of the iterate over NOISE_SEEDS column orders."""
    v64 = iterate(M, iters)
    return max(float(np.abs(iterate(M, iters, f32, np.random.RandomState(s).permutation(M.shape[0])) - v64).max())
               for s in range(NOISE_SEEDS))


def select(v, S):
    """labels [N] fp32: the S largest entries of v, equal entries in index order (a
    stable sort on (-v, index)); -0 and +0 are one value."""
    v = np.asarray(v)
    key = -v.astype(np.float64) + 0.0  # -(+0) + 0 = +0 = -(-0) + 0
    order = np.lexsort((np.arange(len(v)), key))
    labels = np.zeros(len(v), f32)
    labels[order[:S]] = 1
    return labels


def top_count(N, top_ratio):
    """int(N * top_ratio) (:46), the double product truncated."""
    return int(N * float(top_ratio))


def row_abs_sums(M, v):
    """(M v, sum_j |M_ij v_j|) in fp64: the matvec bound's two sides."""
    M, v = np.asarray(M, np.float64), np.asarray(v, np.float64)
    return M @ v, np.abs(M) @ np.abs(v)


def matvec_bound(N, abs_sum):
    """(N + 2) 2^-24 sum_j |M_ij v_j|: N fused multiply-adds in any order (each rounds
    once, relative 2^-24, on a partial sum bounded by the sum of magnitudes) stay
    inside; a dropped or doubled term of typical size does not."""
    return (N + 2) * 2.0 ** -24 * abs_sum


# ---------------------------------------- numpy models of the kernels' rules
def select_model(v, S, ties="index", carry=True, chunk=1024):
    """sm_select_kernel's rule, chunk by chunk: t = the S-th largest key; every key > t
    is chosen, and of the keys == t the first S - #(key > t) in index order, the rank
    of a tie being the count of ties in earlier chunks (`running`) plus those before it
    in its own chunk.  ties='all' / 'none' and carry=False are the rule with one part
    taken out (what the tests must reject)."""
    v = np.asarray(v, np.float64) + 0.0
    N = len(v)
    labels = np.zeros(N, f32)
    if S <= 0:
        return labels
    t = np.sort(v)[::-1][S - 1]
    need_eq = S - int((v > t).sum())
    running = 0
    for base in range(0, N, chunk):
        c = v[base:base + chunk]
        eq = c == t
        r = (running if carry else 0) + np.cumsum(eq) - eq
        if ties == "index":
            take = eq & (r < need_eq)
        else:
            take = eq if ties == "all" else np.zeros_like(eq)
        labels[base:base + chunk] = (c > t) | take
        running += int(eq.sum())
    return labels


MATVEC_PAD = 64  # elements of NaN the GPU test keeps behind M and behind v


def matvec_model(M, v, tail=True):
    """The scalar matvec's row sum in fp64; tail=False: the loop without its j < N
    bound on the last step -- lane l reads j = l + 64 t up to the next multiple of 64,
    i.e. the start of the next row of M and what follows v: MATVEC_PAD NaNs, as the
    GPU test lays its buffers out."""
    M, v = np.asarray(M, np.float64), np.asarray(v, np.float64)
    N = len(v)
    if tail:
        return M @ v
    P = (N + 63) // 64 * 64
    flat = np.concatenate([M.ravel(), np.full(MATVEC_PAD, np.nan)])
    vp = np.concatenate([v, np.full(MATVEC_PAD, np.nan)])[:P]
    return np.stack([flat[i * N:i * N + P] @ vp for i in range(N)])


def matvec_model_dropped_tail(M, v):
    """The scalar matvec stopping at the last whole step of 64: j < N - N % 64."""
    M, v = np.asarray(M, np.float64), np.asarray(v, np.float64)
    n = len(v) - len(v) % 64
    return M[:, :n] @ v[:n]


def compat_store_model(M, sentinel, scalar=True):
    """What sm_compat_kernel leaves in a sentinel-filled buffer: whole groups of four
    by the 16-B store when N % 4 == 0, everything else by the scalar branch."""
    N = M.shape[0]
    out = np.full_like(M, sentinel)
    if N % 4 == 0 or scalar:
        out[:] = M
    return out


# ------------------------------------------------------------------- cases
def _grid(rng, n):
    return rng.randint(-8, 9, size=(n, 3)).astype(f32)


def _pack(src, tgt, thr, **kw):
    src, tgt = np.ascontiguousarray(src, f32), np.ascontiguousarray(tgt, f32)
    return dict(corr=np.concatenate([src, tgt], -1), src=src, tgt=tgt, thr=thr, N=len(src), **kw)


@functools.lru_cache(maxsize=None)
def random_case(N, preset):
    """synthetic_pair(N, seed 31 + N), as tests/test_sm.py draws it; with M, the fp64
    iterates and the fp32 noise for ITERS (cached: treat as read-only)."""
    from pointdsc_amd.synthetic import synthetic_pair
    p = synthetic_pair(N, seed=31 + N, preset=preset)
    d = dict(corr=p["corr_pos"], src=p["src_keypts"], tgt=p["tgt_keypts"], thr=PRESET_THR[preset], N=N,
             gt_trans=p["gt_trans"])
    d["M"] = matrix(d["corr"], d["thr"])
    d["v64"] = {it: iterate(d["M"], it) for it in ITERS}
    d["noise"] = {it: noise(d["M"], it) for it in ITERS}
    return d


@functools.lru_cache(maxsize=None)
def oracle_run(N, preset, iters):
    """oracle.pdsc_oracle.sm on random_case(N, preset): (trans, labels, v)."""
    from oracle import pdsc_oracle as O
    d = random_case(N, preset)
    return O.sm(d["corr"], d["src"], d["tgt"], d["thr"], TOP_RATIO, iters)


@functools.lru_cache(maxsize=None)
def tie_case(N, a, b, seed=0):
    """Integer-grid points with exact ties in v.  Two groups of a > b members at
    scattered indices, each moved by its own integer translation (so every distance
    inside a group is the same fp32 number in both clouds: M = 4.5), the second also
    shifted by 64 in x in both clouds (its distances to the first differ between the
    clouds by more than 7: M = 0); every other point is an outlier with target
    3 p + 1000 (1 + rank) (M = 0 against everything).  Cached, read-only."""
    rng = np.random.RandomState(seed)
    src = _grid(rng, N)
    order = rng.permutation(N)
    ga, gb, out = np.sort(order[:a]), np.sort(order[a:a + b]), np.sort(order[a + b:])
    ta = rng.randint(-5, 6, size=3)
    tb = ta + np.array([-(20 + rng.randint(0, 8)), rng.randint(-5, 6), rng.randint(-5, 6)])
    tgt = np.zeros_like(src)
    tgt[ga] = src[ga] + ta.astype(f32)
    src[gb, 0] += f32(64)
    tgt[gb] = src[gb] + tb.astype(f32)
    tgt[out] = f32(3) * src[out] + (f32(1000) * (1 + np.arange(len(out), dtype=f32)))[:, None]
    group = np.zeros(N, np.int8)  # 0 outlier, 1 the large group, 2 the small one
    group[ga], group[gb] = 1, 2
    d = _pack(src, tgt, 0.10, a=a, b=b, group=group)
    d["M"] = matrix(d["corr"], d["thr"])
    d["v64"], d["noise"] = {1: iterate(d["M"], 1)}, {1: noise(d["M"], 1)}
    return d


@functools.lru_cache(maxsize=None)
def dead_case(N, seed=0):
    """No compatible pair: every point an outlier of tie_case's kind, M == 0, v == 0."""
    rng = np.random.RandomState(1000 + seed + N)
    src = _grid(rng, N)
    tgt = f32(3) * src + (f32(1000) * (1 + np.arange(N, dtype=f32)))[:, None]
    d = _pack(src, tgt, 0.10)
    d["M"] = matrix(d["corr"], d["thr"])
    return d


# top_ratio per regime of the tie cases (S < a; a < S < a + b; S > a + b)
TIE_CASES = {(2500, 900, 500): (0.32, 0.54, 0.96), (70, 30, 20): (0.3, 0.6, 0.9)}
# num_iterations = 0 on the N = 2500 case: v == 1, S on both sides of 1024 and of 2048
ZERO_ITER_RATIOS = (0.4, 0.4096, 0.41, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def signed_matvec_case(N):
    """A random signed M [N,N] and a signed v [N] (fp32): terms that cancel."""
    rng = np.random.RandomState(7000 + N)
    return rng.randn(N, N).astype(f32), rng.randn(N).astype(f32)
