"""tests/front_reference.py on the CPU: the references agree with the oracle, the row
checker of the seed kNN can fail, and every case of tests/test_gpu_front_stages.py
meets the condition it exists for -- so a bad seed or a misread launch rule fails
here and not on the GPU."""
import numpy as np
import pytest

import front_reference as R
from oracle import pdsc_oracle as O

f32 = np.float32


# --------------------------------------------------------------------- a1
@pytest.mark.parametrize("N", R.COMPAT_SIZES)
def test_packed_layout_round_trip(N):
    """pack_symmetric and packed_offset (two restatements of include/pdsc.h's formula)
    invert each other on a random symmetric matrix; everything past N is +0."""
    rng = np.random.RandomState(N)
    M = rng.rand(N, N).astype(f32) + f32(1)
    M = np.maximum(M, M.T)
    P = R.pack_symmetric(M)
    assert P.shape == (R.packed_floats(N),)
    got = np.array([[P[R.packed_offset(i, j, N)] for j in range(N)] for i in range(N)])
    assert np.array_equal(got, M)
    # M >= 1 everywhere, so the zeros are exactly the entries past N of every tile
    nt = (N + 31) // 32
    pad = sum(1024 - min(32, N - ti * 32) * min(32, N - tj * 32) for ti in range(nt) for tj in range(ti, nt))
    assert (P == 0).sum() == pad and not np.signbit(P).any()


@pytest.mark.parametrize("sigma", R.ZERO_PROOF_SIGMAS)
def test_zero_proof_case_sits_on_the_boundary(sigma):
    src, tgt = R.zero_proof_pair(sigma)
    row = O.compat(src[0], tgt[0], sigma)[0]
    zeros, small = int((row == 0).sum()), int(((row > 0) & (row < 2.0 ** -5)).sum())
    xs = (src[0, :, 0].astype(np.float64)) ** 2 + (tgt[0, :, 0].astype(np.float64)) ** 2
    print(f"sigma {sigma}: row 0 has {zeros} exact zeros, {small} values in (0, 2^-5); "
          f"xs + xt > 2^20 s2 for {int((xs > 2.0 ** 20 * sigma ** 2).sum())} of {len(xs)} points")
    assert zeros >= 5 and small >= 5
    assert (xs > 2.0 ** 20 * sigma ** 2).any() and (xs[1:] <= 2.0 ** 20 * sigma ** 2).any()


@pytest.mark.parametrize("sigma", R.SIGMA_OUTSIDE)
def test_sigma_outside_values(sigma):
    """sigma^2 is subnormal / >= 1e30 in fp32, and the oracle still tells duplicate
    points (M = 1) from the rest."""
    s2 = f32(sigma) * f32(sigma)
    assert (0 < s2 < f32(1.17549435e-38)) or s2 >= f32(1e30)
    src, tgt = R.compat_pairs(R.SIGMA_OUTSIDE_N, dups=5)
    M = R.compat_reference(src, tgt, sigma)
    assert (M == 1).sum() > 2 * R.SIGMA_OUTSIDE_N and not np.isnan(M).any()
    if sigma < 1:
        assert (M == 0).any()


# --------------------------------------------------------------------- a5
@pytest.mark.parametrize("B", R.SEED_BS)
@pytest.mark.parametrize("N", R.SEED_SIZES)
def test_seed_reference_vs_oracle(N, B):
    src, conf = R.seed_case(B, N)
    for b in range(B):
        for S in R.seed_counts(N):
            seeds, lm = R.seed_reference(src[b], conf[b], R.SEED_RADIUS, S)
            o_seeds, o_lm = O.pick_seeds(src[b], conf[b], R.SEED_RADIUS, S)
            assert np.array_equal(lm, o_lm) and np.array_equal(seeds, o_seeds)
            sc = [float(x) for x in (conf[b] * lm).astype(f32)]
            assert not np.isnan(sc).any()
            assert list(seeds) == sorted(range(N), key=lambda i: (-sc[i], i))[:S]
    if B == 3:
        assert R.seed_reference(src[1], conf[1], R.SEED_RADIUS, N)[1].all()
        assert np.array_equal(R.seed_reference(src[1], conf[1], R.SEED_RADIUS, N)[0], np.arange(N))
        assert np.isneginf(conf[2]).any() or N < 2


def test_seed_inputs_have_the_edges():
    src, conf = R.seed_case(1, 1025)
    lm = O.local_max(src[0], conf[0], R.SEED_RADIUS)
    sc = (conf[0] * lm).astype(f32)
    assert np.signbit(sc[sc == 0]).any() and (~np.signbit(sc[sc == 0])).any()    # both zeros
    assert ((lm == 1) & (conf[0] < 0)).any()                                      # negative maxima
    assert len(np.unique(sc)) <= 12                                               # heavy ties
    assert len(np.unique(src[0], axis=0)) < 1025                                  # duplicate points
    assert 0.2 < lm.mean() < 0.9


@pytest.mark.parametrize("c", R.SEED_PLAN_CASES, ids=[c["id"] for c in R.SEED_PLAN_CASES])
def test_seed_plan_cases(c):
    """The shape rules of plan_tail restated; the LDS cap and the candidate count of
    the select form's compare fallback."""
    B, N, S = c["B"], c["N"], c["S"]
    rows = 16 if B * ((N + 63) // 64) < 1024 else 64
    select = R.sel_lds(N) <= 64 * 1024 and float(B) * N * N >= 1e8
    rank = (3 if S > 256 else 2) if select else 0
    assert c["plan"] == (rows, 2 if B > 1 and rows == 16 else 1, rank)
    assert int(N * R.plan_ratio(N, S)) == S
    if N == 10000:
        assert ((N + 1) & ~1) * 4 + 2048 * 12 <= 65536
        src, conf = R.seed_plan_case(B, N, S)
        lm = O.local_max(src[0], conf[0], R.SEED_RADIUS)
        A = R.candidates_above((conf[0] * lm).astype(f32), S)
        print(f"N = 10000: {int(lm.sum())} local maxima, {A} candidates above the S-th score")
        assert A > R.SEL_CMAX


@pytest.mark.parametrize("name", R.RADIUS_CASES)
def test_radius_cases(name):
    src, conf, Rad = R.radius_case(name)
    for b in range(R.RADIUS_B):
        lm = O.local_max(src[b], conf[b], Rad)
        D = O.src_dist(src[b])
        iu = np.triu_indices(R.RADIUS_N, 1)
        if name == "zero":
            assert lm.all()
        elif name == "huge":
            with np.errstate(over="ignore"):
                assert lm.sum() == 1 and f32(Rad) * f32(Rad) == np.inf
        elif name == "lattice":
            exact = int((D[iu] == f32(Rad)).sum())
            step = f32(2.0 ** -6)
            print(f"pair {b}: {exact} point pairs at exactly R, {int((D[iu] == 7 * step).sum())} one cell inside, "
                  f"{int((D[iu] == 9 * step).sum())} one cell outside")
            assert exact >= 20 and (D[iu] == 7 * step).any() and (D[iu] == 9 * step).any()
            assert not np.array_equal(lm, R.local_max_strict(src[b], conf[b], Rad))
        else:  # tiny
            with np.errstate(under="ignore"):
                assert f32(Rad) * f32(Rad) == 0
            sq = (D[iu].astype(np.float64)) ** 2
            assert ((D[iu] == 0).sum() >= 3) and ((sq > 0) & (sq < 1.17549435e-38)).sum() >= 3
            # the two separations fall on either side of the radius, and it matters
            assert not np.array_equal(lm, O.local_max(src[b], conf[b], 1e-19))
            assert not np.array_equal(lm, O.local_max(src[b], conf[b], 0.0))


def test_isolation_case():
    src, conf = R.isolation_case()
    assert np.isnan(conf[1]).all() and not np.isnan(conf[[0, 2]]).any()
    assert conf.shape == (R.ISOLATION["B"], R.ISOLATION["N"])


# --------------------------------------------------------------------- a6
def _oracle_rows(c):
    d = R.knn_case(c)
    for b in range(c["B"]):
        yield b, d, O.knn_seed_rows(d["normed"][b], d["seeds"][b], c["k"])


@pytest.mark.parametrize("c", R.KNN_CASES, ids=[c["id"] for c in R.KNN_CASES])
def test_knn_checker_accepts_the_oracle(c):
    for b, d, rows in _oracle_rows(c):
        N, S, k = c["N"], c["S"], c["k"]
        seeds = d["seeds"][b]
        assert seeds[0] == 0 and (S < 2 or seeds[1] == N - 1) and (S < 4 or seeds[2] == seeds[3])
        assert np.abs(np.linalg.norm(d["normed"][b].astype(np.float64), axis=1) - 1).max() < 1e-6
        for r, s in enumerate(seeds):
            R.check_knn_row(rows[r], R.knn_d64(d["normed"][b], s), k)
        g = d["groups"][b]
        if len(g):
            assert len(g) == c["dups"] + 1 and g[0] == 0 and seeds[2] in g and seeds[2] != 0
            for r, s in enumerate(seeds):
                if s in g:  # index order decides inside the tie group; the lowest index is dropped
                    lead = R.tie_group_row(g, k)
                    assert np.array_equal(rows[r][:len(lead)], lead), (r, s)
                    assert (s in rows[r]) == (s != 0 and np.searchsorted(g, s) <= k)
        if c["dups2"]:
            assert (g % 64 < 8).all()


def test_knn_cases_reach_their_forms():
    ids = {c["id"]: c for c in R.KNN_CASES}
    assert len(ids) == len(R.KNN_CASES)
    c = ids["B19-N1001-S129-k40"]
    assert R.knn_wg5(c["B"], c["N"], c["S"]) >= 256
    assert all(R.knn_wg5(x["B"], x["N"], x["S"]) < 256 for x in R.KNN_CASES if x is not c and x["B"] < 16)
    c = ids["B16-N300-S129-k40"]
    assert c["B"] * ((c["S"] + 3) // 4) >= 512 and c["S"] % 4
    assert all(x["B"] * ((x["S"] + 3) // 4) < 512 for x in R.KNN_CASES if x["B"] < 16)
    for x in R.KNN_CASES:
        assert 1 <= x["k"] <= 63 and x["k"] + 1 <= x["N"]


def _row_case():
    c = next(x for x in R.KNN_CASES if x["id"] == "B1-N257-S5-k40")
    d = R.knn_case(c)
    s = int(d["seeds"][0][1])
    d64 = R.knn_d64(d["normed"][0], s)
    row = O.knn_seed_rows(d["normed"][0], d["seeds"][0], c["k"])[1].copy()
    R.check_knn_row(row, d64, c["k"])
    return row, d64, c["k"]


def test_knn_checker_rejects_a_swap():
    row, d64, k = _row_case()
    a = next(i for i in range(k - 1) if d64[row[i + 1]] - d64[row[i]] > 10 * R.KNN_EPS)
    row[[a, a + 1]] = row[[a + 1, a]]
    with pytest.raises(AssertionError, match="ascending"):
        R.check_knn_row(row, d64, k)


def test_knn_checker_rejects_the_wrong_drop():
    row, d64, k = _row_case()
    order = np.argsort(d64, kind="stable")
    assert d64[order[1]] - d64[order[0]] > 10 * R.KNN_EPS
    bad = np.concatenate([[order[0]], order[2:k + 1]])  # the second-nearest dropped, the nearest kept
    with pytest.raises(AssertionError, match="absent"):
        R.check_knn_row(bad, d64, k)


def test_knn_checker_rejects_an_unwritten_slot():
    row, d64, k = _row_case()
    row[k // 2] = -1
    with pytest.raises(AssertionError, match="outside"):
        R.check_knn_row(row, d64, k)


def test_knn_checker_rejects_a_repeat():
    row, d64, k = _row_case()
    row[5] = row[4]
    with pytest.raises(AssertionError, match="repeated"):
        R.check_knn_row(row, d64, k)


def test_knn_checker_rejects_a_far_entry():
    row, d64, k = _row_case()
    row[k - 1] = np.argmax(d64)
    with pytest.raises(AssertionError, match="beyond"):
        R.check_knn_row(row, d64, k)


# --------------------------------------------------------------------- f1
@pytest.mark.parametrize("shape", sorted(R.CORR_ORACLE_SEEDS) + sorted(R.CORR_EDGE_SEEDS), ids=str)
def test_nn_margins(shape):
    if len(shape) == 2:
        Ns, Nt, D, seed = shape + (32, R.CORR_ORACLE_SEEDS[shape])
    else:
        Ns, Nt, D, seed = shape + (R.CORR_EDGE_SEEDS[shape],)
    _, _, sd, td, _ = R.corr_pair(Ns, Nt, D, seed)
    rg, cg = R.nn_margin(sd, td)
    assert rg.shape == (Ns,) and cg.shape == (Nt,)
    m = float(min(rg.min(), cg.min()))
    print(f"{shape}: seed {seed}, minimum gap {m:.3g}")
    assert m >= R.NN_MARGIN
    if Ns > 1 and Nt > 1:
        r = O.build_correspondences(np.zeros((Ns, 3), f32), np.zeros((Nt, 3), f32), sd, td)
        assert 0 < len(r["corr"]) < Ns or min(Ns, Nt) < 64


def test_nn_margin_is_the_runner_up_gap():
    sd = np.eye(3, 4, dtype=f32)
    td = np.array([[1, 0, 0, 0], [0.6, 0.8, 0, 0]], f32)
    rg, cg = R.nn_margin(sd, td)
    np.testing.assert_allclose(rg, [0.8, 1.6, 0.0], atol=1e-6)
    np.testing.assert_allclose(cg, [2.0, 0.4], atol=1e-6)


def test_single_mutual_pair_case():
    src, tgt, sd, td = R.single_mutual_pair()
    r = O.build_correspondences(src, tgt, sd, td)
    assert (r["source_idx"] == 0).all() and len(r["corr"]) == 1
    assert R.min_margin(sd, td) >= R.NN_MARGIN
    # no descriptor set has an empty mutual set: the first global minimum is mutual
    rng = np.random.RandomState(0)
    for _ in range(20):
        a, b = rng.randint(0, 3, (6, 5)).astype(f32), rng.randint(0, 3, (7, 5)).astype(f32)
        d = -(a @ b.T)
        i0, j0 = np.unravel_index(np.argmin(d), d.shape)
        assert np.argmin(d[i0]) == j0 and np.argmin(d[:, j0]) == i0


def test_straddle_ties_case():
    for sd, td, rows, expect in R.straddle_ties():
        assert td.shape == (65, 32) and np.array_equal(td[64], td[expect])
        r = O.build_correspondences(np.zeros((40, 3), f32), np.zeros((65, 3), f32), sd, td)
        assert (r["source_idx"][rows] == expect).all()
        keep = np.arange(65) != 64  # apart from the planted tie every row and column has the margin
        assert R.min_margin(sd, td[keep]) >= R.NN_MARGIN
        assert R.nn_margin(sd, td)[1].min() >= R.NN_MARGIN
