"""tests/sm_reference.py against the oracle (oracle.pdsc_oracle.sm_matrix / sm, which
cite baseline_scripts/baseline_3DMatch.py:19-53), the preconditions of every case of
tests/test_gpu_sm_stages.py, and -- on numpy models of the kernels' rules -- that those
tests reject sm.hip with one part taken out: the scalar store branch of
sm_compat_kernel, the j < N tail of the scalar matvec, the need_eq tie rule and the
`running` carry of sm_select_kernel.  No GPU: no broken kernel is ever run.

Measured here (printed, -s): the fp32 noise of the iterate (4 column orders) is 0 where
M == 0 (N <= 4), else 1.0e-8 .. 8.5e-8 at one iterate and 0.8e-8 .. 4.0e-8 at ten over
the size table; the oracle's vector (fp64 sums, fp32 storage) is 4.5e-9 and 3.1e-9 from
the fp64 iterate at N = 1000 and 2000."""
import numpy as np
import pytest

import sm_reference as R
from conftest import ENVELOPE, FEAT_FLOOR
from oracle import pdsc_oracle as O

f32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


# ------------------------------------------------ the restatement vs the oracle
@pytest.mark.parametrize("N,preset", [(300, "3dmatch"), (1000, "3dmatch"), (2000, "kitti")])
def test_restatement_vs_oracle_sm(N, preset):
    """The sizes of tests/test_sm.py (5000 is left to the size table below: the bitwise
    M check runs on every size there)."""
    d = R.random_case(N, preset)
    assert np.array_equal(_bits(d["M"]), _bits(O.sm_matrix(d["corr"], d["thr"])))
    T, lab, v = O.sm(d["corr"], d["src"], d["tgt"], d["thr"])
    v64, nz = d["v64"][10], d["noise"][10]
    e = float(np.abs(v - v64).max())
    print(f"N{N}-{preset}: |v_oracle - v64| {e:.3g}, fp32 noise {nz:.3g}")
    assert e <= ENVELOPE * nz + FEAT_FLOOR * np.abs(v64).max()
    S = R.top_count(N, R.TOP_RATIO)
    assert S == int(lab.sum())
    assert np.array_equal(R.select(v, S), lab)
    assert np.array_equal(R.select_model(v, S), lab)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_random_case_preconditions(c):
    N, preset = c
    d = R.random_case(N, preset)
    M = d["M"]
    assert M.dtype == f32 and M.shape == (N, N)
    assert np.array_equal(_bits(M), _bits(O.sm_matrix(d["corr"], d["thr"])))
    assert not _bits(np.diag(M)).any()  # +0, not -0
    assert M.min() >= 0 and M.max() <= 4.5
    for it in R.ITERS:
        v64 = d["v64"][it]
        print(f"{R.case_id(c)} iters {it}: fp32 noise {d['noise'][it]:.3g}, max v64 {np.abs(v64).max():.3g}")
        assert np.isfinite(v64).all() and (v64 >= 0).all()
        assert d["noise"][it] <= 1e-6  # four fp32 orderings agree with fp64 to fp32 resolution
        if M.any():
            assert abs(np.linalg.norm(v64) - 1) < 1e-5
    if N > 4:
        assert M.any()  # the size's paths see non-zero entries
    assert (R.top_count(9, R.TOP_RATIO), R.top_count(10, R.TOP_RATIO)) == (0, 1)


@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_oracle_on_size_table(c, iters):
    """The oracle at every size and iterate count of the GPU test: its vector inside the
    envelope of the fp64 iterate, its labels `select` of its own vector."""
    N, preset = c
    d = R.random_case(N, preset)
    T, lab, v = R.oracle_run(N, preset, iters)
    v64 = d["v64"][iters]
    assert np.abs(v - v64).max() <= ENVELOPE * d["noise"][iters] + FEAT_FLOOR * np.abs(v64).max()
    S = R.top_count(N, R.TOP_RATIO)
    assert np.array_equal(R.select(v, S), lab) and int(lab.sum()) == S
    assert np.isfinite(T).all()
    if not np.array_equal(R.select(v64, S), lab):
        print(f"{R.case_id(c)} iters {iters}: a near-tie at the boundary separates fp64 from the oracle")


def test_size_table():
    """Each size sits on the side of its boundary that its comment claims."""
    S = set(R.SIZES)
    assert {1, 2, 3, 4, 9, 10, 63, 64, 65, 67, 128, 130, 252, 256, 260, 257, 1023, 1024, 1025, 1028, 2050} == S
    assert max(S) <= 2500
    scalar = {n for n in S if n % 4}
    assert {1, 2, 3, 9, 10, 63, 65, 67, 130, 257, 1023, 1025, 2050} == scalar
    assert (67, "kitti") in R.CASES and (1028, "kitti") in R.CASES


def test_select_rule():
    v = f32([0.5, -0.0, 0.5, 0.0, 1.0, 0.5, -1.0])
    assert R.select(v, 0).tolist() == [0] * 7
    assert R.select(v, 1).tolist() == [0, 0, 0, 0, 1, 0, 0]
    assert R.select(v, 3).tolist() == [1, 0, 1, 0, 1, 0, 0]   # ties to the lower index
    assert R.select(v, 5).tolist() == [1, 1, 1, 0, 1, 1, 0]   # -0 ties with +0 and comes first by index
    assert R.select(v, 7).tolist() == [1] * 7
    for S in range(8):
        assert np.array_equal(R.select_model(v, S, chunk=3), R.select(v, S))


# --------------------------------------------------------- the tie cases
@pytest.mark.parametrize("key", list(R.TIE_CASES), ids=lambda k: "N%d-a%d-b%d" % k)
def test_tie_case_preconditions(key):
    N, a, b = key
    d = R.tie_case(N, a, b)
    M, g = d["M"], d["group"]
    assert (g == 1).sum() == a and (g == 2).sum() == b and a > b
    assert set(np.unique(M).tolist()) == {0.0, 4.5}
    rows = M.astype(np.float64).sum(1)
    assert np.array_equal(rows, np.where(g == 1, 4.5 * (a - 1), np.where(g == 2, 4.5 * (b - 1), 0.0)))
    # a row sum is exact in fp32 in any order: every partial sum is 4.5 k, k < 2^20
    assert f32(4.5 * (a - 1)) == 4.5 * (a - 1)
    for dt, perm in ((np.float64, None), (f32, np.random.RandomState(0).permutation(N))):
        v = R.iterate(M, 1, dt, perm)
        assert len(np.unique(v)) == 3
        va, vb = v[g == 1][0], v[g == 2][0]
        assert np.all(v[g == 1] == va) and np.all(v[g == 2] == vb) and not v[g == 0].any() and va > vb > 0
    v = R.iterate(M, 1, f32, np.arange(N))
    regimes = []
    for ratio in R.TIE_CASES[key]:
        S = R.top_count(N, ratio)
        regimes.append((S < a, a < S < a + b, S > a + b))
        lab = R.select(v, S)
        tied_group = 1 if S < a else 2 if S < a + b else 0
        idx = np.nonzero(g == tied_group)[0]
        n_tied = S - (0 if S < a else a if S < a + b else a + b)
        # the greater groups whole, then the first n_tied of the tied group by index
        want = np.zeros(N, f32)
        want[g == 1] = S >= a
        want[g == 2] = S >= a + b
        want[idx[:n_tied]] = 1
        assert 0 < n_tied < len(idx)
        assert np.array_equal(lab, want)
        if N > 2048:  # chosen and refused ties on both sides of both chunk edges
            chosen, refused = idx[:n_tied], idx[n_tied:]
            assert chosen.min() < 1024 < chosen.max() and chosen.max() > 2048
            assert (np.diff((chosen // 1024)) >= 0).all() and len(set((chosen // 1024).tolist())) == 3
            assert refused.min() > 2048  # the cut falls in the third chunk: `running` decides it
    assert regimes == [(True, False, False), (False, True, False), (False, False, True)]


def test_zero_iteration_ratios():
    Ss = [R.top_count(2500, r) for r in R.ZERO_ITER_RATIOS]
    assert min(Ss) < 1024 < max(Ss) and any(1024 <= s <= 1025 for s in Ss) and max(Ss) > 2048
    v = np.ones(2500, f32)
    for s in Ss:
        assert np.array_equal(R.select(v, s), (np.arange(2500) < s).astype(f32))


@pytest.mark.parametrize("N", [1, 65])
def test_dead_case_preconditions(N):
    d = R.dead_case(N)
    assert d["M"].shape == (N, N) and not d["M"].any()
    for it in (0, 1, 10):
        v = R.iterate(d["M"], it, f32, np.arange(N))
        assert np.array_equal(v, np.full(N, 1.0 if it == 0 else 0.0, f32))
    if N > 1:  # by a margin no rounding crosses: every |ds - dt| is above 900 against thr 0.1
        c = d["corr"].astype(np.float64)
        ds = np.linalg.norm(c[:, None, :3] - c[None, :, :3], axis=-1)
        dt = np.linalg.norm(c[:, None, 3:] - c[None, :, 3:], axis=-1)
        assert np.abs(ds - dt)[~np.eye(N, dtype=bool)].min() > 900


# ------------------------------- what the GPU tests reject, argued on the CPU
SCALAR_SIZES = [n for n in R.SIZES if n % 4]


@pytest.mark.parametrize("N", SCALAR_SIZES)
def test_rejects_missing_scalar_store(N):
    """sm_compat_kernel without its scalar branch writes nothing when N % 4 != 0: the
    bitwise M test sees the buffer's fill (NaN there) in every element."""
    M = R.random_case(N, "3dmatch")["M"]
    assert np.array_equal(_bits(R.compat_store_model(M, f32(np.nan))), _bits(M))
    assert not np.array_equal(_bits(R.compat_store_model(M, f32(np.nan), scalar=False)), _bits(M))


@pytest.mark.parametrize("N", SCALAR_SIZES)
def test_rejects_scalar_matvec_without_tail(N):
    """The scalar matvec without `j < N` on its last step (reading on into the next
    row), or stopping at the last whole step, breaks the per-row bound of the signed
    case at every scalar-path size."""
    M, v = R.signed_matvec_case(N)
    y64, s = R.row_abs_sums(M, v)
    bound = R.matvec_bound(N, s)
    assert np.all(np.abs(R.matvec_model(M, v) - y64) <= bound)
    fp32 = (M @ v).astype(np.float64)  # numpy's own fp32 order sits inside the bound
    assert np.all(np.abs(fp32 - y64) <= bound)
    assert N % 64 and (N + 63) // 64 * 64 - N <= R.MATVEC_PAD
    # the GPU test asserts all(|y - y64| <= bound): a NaN read from behind v fails it
    assert not np.all(np.abs(R.matvec_model(M, v, tail=False) - y64) <= bound)
    assert not np.all(np.abs(R.matvec_model_dropped_tail(M, v) - y64) <= bound)


@pytest.mark.parametrize("key", list(R.TIE_CASES), ids=lambda k: "N%d-a%d-b%d" % k)
def test_rejects_broken_tie_rule(key):
    """need_eq: choosing every tie, or none, differs from `select` in all three regimes."""
    N, a, b = key
    v = R.iterate(R.tie_case(N, a, b)["M"], 1, f32, np.arange(N))
    for ratio in R.TIE_CASES[key]:
        S = R.top_count(N, ratio)
        want = R.select(v, S)
        assert np.array_equal(R.select_model(v, S), want)
        assert not np.array_equal(R.select_model(v, S, ties="all"), want)
        assert not np.array_equal(R.select_model(v, S, ties="none"), want)


def test_rejects_missing_running_carry():
    """`running`: ranking ties inside each 1024-chunk only chooses too many in the later
    chunks, in every regime of the N = 2500 case and at zero iterations."""
    N, a, b = 2500, 900, 500
    v = R.iterate(R.tie_case(N, a, b)["M"], 1, f32, np.arange(N))
    for ratio in R.TIE_CASES[(N, a, b)]:
        S = R.top_count(N, ratio)
        bad = R.select_model(v, S, carry=False)
        assert not np.array_equal(bad, R.select(v, S)) and bad.sum() > S
    ones = np.ones(N, f32)
    for ratio in R.ZERO_ITER_RATIOS:
        S = R.top_count(N, ratio)
        assert np.array_equal(R.select_model(ones, S), R.select(ones, S))
        assert not np.array_equal(R.select_model(ones, S, carry=False), R.select(ones, S))
