"""The fp64 reference of tests/nsm_reference.py against the oracle (which is pinned
to the reference's goldens), the fp32 oracle's own distance from fp64, and the
preconditions of every case of tests/test_gpu_nsm_stages.py -- on the CPU, so a
seed that lands on a near-tie fails here and not on the GPU.

Measured here (printed by each test, -s): on tiny_k / small_3dm the oracle's T is
within 2.5e-6 of fp64, its leading eigenvector within 3.9e-6, its seed poses within
9e-7, its residuals within 6e-7, its refined pose within 3.6e-7.  On the NSM cases the
oracle's largest iterate deviation from fp64 is 0 .. 1.03e-5 per case (eps = 4x the
case's own value: 0 .. 4.13e-5, the largest on 31 unconverged iterates) and e_ref
(weights) 0 .. 4.68e-6; on the hypotheses cases the oracle's full-rank seed poses are
within 1.78e-5 of fp64 and at most 1.53e-5 of the entries lie in the delta band; on
the refinement cases e_ref is 2.1e-7 .. 2.43e-6."""
import numpy as np
import pytest

import nsm_reference as R
from conftest import ENVELOPE, load_golden, golden_state_dict
from oracle import pdsc_oracle as O

GOLDENS = ["tiny_k", "small_3dm"]


def _ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------ the reference vs the oracle
@pytest.mark.parametrize("name", GOLDENS)
def test_nsm_fp64_vs_oracle(name):
    g = load_golden(name)
    sd = golden_state_dict(g)
    sigma, sigma_d = float(sd["sigma"][0]), float(sd["sigma_spat"][0])
    normed = O.normalize(g["corr_features"])
    src, tgt, knn = g["src_keypts"], g["tgt_keypts"], g["knn_idx"]
    T32 = O.local_consistency(normed, src, tgt, knn, sigma, sigma_d)
    v32, it = O.power_iteration(T32)
    T64 = R.consistency_fp64(normed, src, tgt, knn, sigma, sigma_d)
    its, mar = R.nsm_fp64(normed, src, tgt, knn, sigma, sigma_d, 10)
    assert its.shape == (11,) + knn.shape and mar.shape == (10, len(knn))
    eT, ev = np.abs(T32 - T64).max(), np.abs(v32 - its[it]).max()
    print(f"{name}: |T32-T64| {eT:.3g}, |v32-v64| {ev:.3g} at iterate {it}")
    assert eT <= 5e-5 and ev <= 1e-5  # the oracle's own tolerances against the goldens
    assert np.array_equal(np.diagonal(T64, axis1=1, axis2=2), np.zeros(knn.shape))
    np.testing.assert_array_equal(T64, T64.transpose(0, 2, 1))
    # the margins restate allclose: the oracle's exit lies in the band its own error allows
    lo, hi = R.exit_band(mar, 4 * max(float(np.abs(O.power_iteration(T32, n)[0] - its[min(n, it)]).max())
                                      for n in range(1, it + 1)))
    assert lo <= it <= hi
    # iterate t + 1 really is T v_t / (|T v_t| + 1e-6)
    nv = (T64 @ its[3][:, :, None])[:, :, 0]
    np.testing.assert_allclose(its[4], nv / (np.linalg.norm(nv, axis=1, keepdims=True) + 1e-6), rtol=1e-14)


@pytest.mark.parametrize("name", GOLDENS)
def test_kabsch_fp64_vs_oracle(name):
    from conftest import kabsch64, seed_H_rank
    g = load_golden(name)
    src, tgt, knn, v = g["src_keypts"], g["tgt_keypts"], g["knn_idx"], g["leading_eig"]
    w = (v / (v.sum(-1, keepdims=True) + np.float32(1e-6))).astype(np.float32)
    T64, sv = R.kabsch_fp64(src[knn], tgt[knn], w)
    T32 = O.rigid_transform_3d(src[knn], tgt[knn], w)
    ok = R.rank_ok(sv)
    assert np.array_equal(ok, seed_H_rank(g) > R.RANK_BAR)
    e = np.abs(T32 - T64)[ok].max()
    print(f"{name}: |kabsch32 - kabsch64| {e:.3g} over {int(ok.sum())} of {len(ok)} seeds")
    assert e <= 1e-4
    assert np.all(np.diff(sv, axis=-1) <= 0)
    for s in np.nonzero(ok)[0][:5]:
        np.testing.assert_allclose(T64[s], kabsch64(src[knn[s]], tgt[knn[s]], w[s]), atol=1e-12)
    # unbatched input, the form post_refine_fp64 uses
    np.testing.assert_allclose(R.kabsch_fp64(src[knn[0]], tgt[knn[0]], w[0])[0], T64[0], atol=1e-12)


@pytest.mark.parametrize("name", GOLDENS)
def test_residual_fp64_vs_oracle(name):
    g = load_golden(name)
    src, tgt, tau = g["src_keypts"], g["tgt_keypts"], float(g["inlier_threshold"])
    L32 = O.residuals(g["seed_trans"], src, tgt)
    L64 = R.residual_fp64(g["seed_trans"], src, tgt)
    e = np.abs(L32 - L64).max()
    delta = R.near_tie_delta(src, tgt)
    print(f"{name}: |residual32 - residual64| {e:.3g}, delta {delta:.3g}")
    assert e <= delta
    fitness, best, labels = O.verify(g["seed_trans"], src, tgt, tau)
    far = np.abs(L64 - float(np.float32(tau))) > delta
    assert np.array_equal((L32 < np.float32(tau))[far], (L64 < float(np.float32(tau)))[far])
    assert np.array_equal(labels[far[best]] > 0, (L64[best] < float(np.float32(tau)))[far[best]])


@pytest.mark.parametrize("name", GOLDENS)
def test_post_refine_fp64_vs_oracle(name):
    g = load_golden(name)
    src, tgt, tau = g["src_keypts"], g["tgt_keypts"], float(g["inlier_threshold"])
    thr = 0.10 if tau == 0.10 else 1.2
    T32, hist = O.post_refinement(g["trans_pre_refine"], src, tgt, tau)
    T64, iters, near = R.post_refine_fp64(g["trans_pre_refine"], src, tgt, thr)
    e = np.abs(T32 - T64).max()
    print(f"{name}: |refine32 - refine64| {e:.3g}, {iters} iterations, near-tie {min(near):.3g}")
    assert iters == len(near) == len(hist) + 1  # the last iteration saw the count repeat
    assert e <= 1e-4
    assert R.is_proper_rigid(T64, 1e-12)


# --------------------------------------------- preconditions of the GPU cases
@pytest.mark.parametrize("c", R.NSM_CASES, ids=_ids(R.NSM_CASES))
def test_nsm_case_preconditions(c):
    """The oracle's iterate deviation (eps = 4x) and e_ref of the case, and that the
    oracle's own exit lies inside the band eps gives it."""
    d = R.nsm_case(c)
    B, S, k, T = (c[n] for n in "BSkT")
    assert d["knn"].shape == (B, S, k) and d["iterates"].shape == (T + 1, B * S, k)
    assert (len(set(d["knn"][0, 0].tolist())) < k) == bool(c["dups"])
    dev, e_ref, it = R.nsm_oracle(d)
    lo, hi = R.exit_band(d["margins"], 4 * dev)
    print(f"{c['id']}: oracle iterate deviation {dev:.3g} (eps {4 * dev:.3g}), e_ref {e_ref:.3g}, "
          f"exit {it} in [{lo}, {hi}]")
    assert lo <= it <= hi
    assert dev <= 5e-5 and e_ref <= 2e-5  # fp32 noise (largest on 31 unconverged iterates), not another algorithm
    if k == 1:
        assert not d["iterates"][1:].any()
    if c.get("outrow"):  # the all-outlier row's T is zero by a margin no fp32 rounding crosses
        s, t = d["src"][0][d["knn"][0, 0]].astype(np.float64), d["tgt"][0][d["knn"][0, 0]].astype(np.float64)
        dd = np.abs(np.linalg.norm(s[:, None] - s[None], axis=-1) - np.linalg.norm(t[:, None] - t[None], axis=-1))
        assert dd[~np.eye(k, dtype=bool)].min() > 2 * c["sigma_d"]
        assert not d["iterates"][1:, 0].any()


@pytest.mark.parametrize("c", R.HYP_CASES, ids=_ids(R.HYP_CASES))
def test_hypotheses_case_preconditions(c):
    d = R.hyp_case(c)
    B, N, S, k = (c[n] for n in "BNSk")
    # the launch plan the shape selects (hypotheses.hip: seed_wpb, kabsch_small, HS = 8)
    plan = (1 if B * ((S + 3) // 4) < 512 else 4, B * S <= 1024)
    want = {"B1-N200-S20-k40": (1, True), "B3-N257-S600-k8": (1, False), "B512-N16-S1-k8": (4, True),
            "B8-N300-S300-k17": (4, False)}
    if c["id"] in want:
        assert plan == want[c["id"]]
    if c["id"] == "B8-N300-S300-k17":
        assert S % 8 == 4
    T32 = np.stack([O.rigid_transform_3d(d["src"][b][d["knn"][b]], d["tgt"][b][d["knn"][b]], d["w"][b])
                    for b in range(B)])
    ok = R.rank_ok(d["sv"])
    if k <= 2:
        assert not ok.any()  # one point, or two: rank(H) <= 1
    elif c["dups"]:
        assert not ok[:, ::2].any()  # three points, two of them the same
    else:
        assert ok.all()
    if ok.any():
        e = np.abs(T32 - d["T64"])[ok].max()
        print(f"{c['id']}: |kabsch32 - kabsch64| {e:.3g} on {int(ok.sum())} of {ok.size} seeds")
        assert e <= 1e-4 / ENVELOPE  # so assert_poses_close's 1e-4 is fp32 noise away from fp64 with room
    for tau in R.HYP_TAUS:
        share, res = R.excluded_share(d["T64"], d["src"], d["tgt"], tau, d["delta"])
        print(f"{c['id']} tau {tau}: excluded share {share:.3g} (delta {d['delta']:.3g})")
        assert share <= R.EXCLUDED_CAP
        cnt = (res < float(np.float32(tau))).sum(-1)
        if S == 600:
            assert (cnt.max(1) > cnt.min(1)).all()  # a best and a worse seed to build ties from
    assert max(max(lay) for lay in R.TIE_LAYOUTS) < 600


@pytest.mark.parametrize("c", R.REFINE_CASES, ids=_ids(R.REFINE_CASES))
def test_refine_case_preconditions(c):
    d = R.refine_case(c)
    N, thr = c["N"], float(np.float32(c["thr"]))
    start = [R.residual_fp64(d["trans0"][p], d["src"][p], d["tgt"][p]) for p in range(5)]
    assert (start[1] < thr).sum() == 0 and d["ref"][1][1] == 1
    assert (start[2] < thr).sum() == 1 and start[2].min() < 1e-5 and np.sort(start[2])[1] > 10
    assert (start[4] < thr).sum() == N
    assert d["ref"][3][1] >= (3 if thr < 1 else 5)
    assert len({d["ref"][p][1] for p in range(5)}) >= 3  # the pairs of one launch stop at different iterations
    assert d["ref"][0][1] < 20
    for p in R.PINNED:
        T64, iters, near = d["ref"][p]
        e_ref = R.refine_oracle(d, p)
        print(f"{c['id']} pair {p}: {iters} iterations, near-tie {min(near):.3g} (delta {d['delta']:.3g}), "
              f"e_ref {e_ref:.3g}, bound {R.refine_bound(d, p, e_ref, ENVELOPE):.3g}")
        assert min(near) > d["delta"]
        assert R.is_proper_rigid(T64, 1e-12)
        assert e_ref <= 1e-4 / ENVELOPE
