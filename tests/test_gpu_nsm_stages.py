"""pdsc_nsm_weights, pdsc_seed_hypotheses, pdsc_post_refine and
pdsc_rigid_transform_3d against the fp64 reference of tests/nsm_reference.py at the
shapes where nsm.hip or hypotheses.hip takes another path: every KC variant of nsm_seed_kernel and
the edges of its Gram tiles, T = 0 / 1 / 31, the four (seed_wpb, kabsch_small)
launch plans, a partial count_inliers group, S > 256 in the argmax, exact ties at
the inlier threshold and between seeds, and several pairs per post_refine launch
(run with -m gpu).  Inputs and their preconditions: tests/test_nsm_reference.py.
Every call goes through pointdsc_amd.kernels; paths are selected by shape only."""
import numpy as np
import pytest
import torch

import nsm_reference as R
from conftest import ENVELOPE, assert_poses_close, assert_rigid

pytestmark = pytest.mark.gpu
f32 = np.float32


def _t(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)


def _ids(cases):
    return [c["id"] for c in cases]


# -------------------------------------------------------------- a. NSM
@pytest.mark.parametrize("precision", ["h3", "f32"])
@pytest.mark.parametrize("c", R.NSM_CASES, ids=_ids(R.NSM_CASES))
def test_nsm_weights_vs_fp64(c, precision, gpu_device):
    """iters_used inside the band the fp64 margins allow, weights equal to the fp64
    iterate at the kernel's own iters_used.

    eps = 4 x the fp32 oracle's largest iterate deviation from fp64 on the case's own
    inputs (measured: 0 .. 1.0e-5 per case, so eps 0 .. 4.1e-5; the largest on the 31
    unconverged iterates of B3-N128-S13-k17-T31).  Weight bound: ENVELOPE x e_ref +
    2^-22 max(1, 1/sigma^2), e_ref = the oracle's weight error on the case (measured
    0 .. 4.7e-6); the second term is H3's 22-bit operand resolution on weights <= 1.
    Measured on an MI355X: |w - w64| at most 0.75 x the bound in either precision
    (5.5e-6 against 1.24e-5 at T = 31), so the derived 2^-22 floor stands."""
    from pointdsc_amd import kernels
    d = R.nsm_case(c)
    B, S, k, T = (c[n] for n in "BSkT")
    dev, e_ref, _ = R.nsm_oracle(d)
    w, it = kernels.nsm_weights(_t(d["normed"], gpu_device), _t(d["src"], gpu_device), _t(d["tgt"], gpu_device),
                                _t(d["knn"], gpu_device, torch.int32), T, _t(f32([c["sigma"]]), gpu_device),
                                _t(f32([c["sigma_d"]]), gpu_device), precision=precision)
    w, it = w.cpu().numpy().reshape(B * S, k), it.cpu().numpy()
    lo, hi = R.exit_band(d["margins"], 4 * dev)
    assert (it == it[0]).all()  # the standalone entry point exits batch-globally
    tk = int(it[0])
    w64 = R.weights_of(d["iterates"][min(max(tk, 0), T)])
    err = float(np.abs(w - w64).max())
    bound = ENVELOPE * e_ref + 2.0 ** -22 * max(1.0, 1.0 / c["sigma"] ** 2)
    print(f"{c['id']} {precision}: iters_used {tk} in [{lo}, {hi}] (eps {4 * dev:.3g}), "
          f"|w - w64| {err:.3g} <= {bound:.3g} (e_ref {e_ref:.3g})")
    assert lo <= tk <= hi
    assert err <= bound
    if k == 1:
        assert not w.any()
    if T == 0:
        assert tk == 0 and np.array_equal(w, np.full_like(w, f32(1) / (f32(k) + f32(1e-6))))
    if c.get("outrow"):
        assert not w[0].any()


# ------------------------------------------------------- b. hypotheses
def _hypotheses(d, knn, w, tau, dev):
    from pointdsc_amd import kernels
    out = kernels.seed_hypotheses(_t(d["src"], dev), _t(d["tgt"], dev), _t(knn, dev, torch.int32), _t(w, dev), tau)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("tau", R.HYP_TAUS)
@pytest.mark.parametrize("c", R.HYP_CASES, ids=_ids(R.HYP_CASES))
def test_seed_hypotheses_vs_fp64(c, tau, gpu_device):
    """Seed poses against kabsch_fp64, the inlier counts against fp64 residuals of the
    kernel's own poses (exact outside the delta band, which holds <= 1 entry in 1000),
    count == labels of the best seed with no exclusion, first argmax, labels."""
    d = R.hyp_case(c)
    B, N, S, k = (c[n] for n in "BNSk")
    st, fit, best, trans, labels = _hypotheses(d, d["knn"], d["w"], tau, gpu_device)
    tauf, delta = float(f32(tau)), d["delta"]
    ok = R.rank_ok(d["sv"])
    for b in range(B):
        A, Bp = d["src"][b][d["knn"][b]], d["tgt"][b][d["knn"][b]]
        o = ok[b]
        assert_poses_close(st[b][o], d["T64"][b][o], A[o], Bp[o], d["w"][b][o], 1e-4)
        for s in np.nonzero(~o)[0]:
            assert_rigid(st[b, s], A[s].astype(np.float64), Bp[s].astype(np.float64), d["w"][b, s])
    share, res = R.excluded_share(st, d["src"], d["tgt"], tau, delta)
    lo, hi = (res < tauf - delta).sum(-1), (res < tauf + delta).sum(-1)
    cnt = np.rint(fit.astype(np.float64) * N).astype(np.int64)
    print(f"{c['id']} tau {tau}: excluded share {share:.3g}, seeds with a band entry {int((lo != hi).sum())} of {B * S}")
    assert share <= R.EXCLUDED_CAP
    assert np.array_equal(fit, cnt.astype(f32) / f32(N))  # fitness = count / N, one fp32 division
    assert (lo <= cnt).all() and (cnt <= hi).all()
    bi = np.arange(B)
    assert np.array_equal(best, fit.argmax(1))  # numpy's argmax: the first maximum
    assert np.array_equal(trans.view(np.uint32), st[bi, best].view(np.uint32))
    # the squared-threshold count and the distance-threshold labels of the same pose: one integer
    assert np.array_equal(cnt[bi, best], labels.sum(1).astype(np.int64))
    assert np.isin(labels, (0.0, 1.0)).all()
    rb = np.stack([R.residual_fp64(trans[b], d["src"][b], d["tgt"][b]) for b in range(B)])
    far = np.abs(rb - tauf) > delta
    assert np.array_equal(labels[far] > 0, (rb < tauf)[far])


@pytest.mark.parametrize("layout", R.TIE_LAYOUTS, ids=lambda lay: "-".join(map(str, lay)))
def test_first_argmax_on_constructed_ties(layout, gpu_device):
    """S = 600 (every thread of the 256-strided loop sees two or three seeds): the
    best seed's kNN row and weights copied to other seeds give bit-identical poses
    and counts, and `best` is the lowest of them -- copies in one thread (44 / 300,
    10 / 266), in neighbouring lanes of one wave (45 / 300) and in two waves (44 / 200)."""
    c = next(c for c in R.HYP_CASES if c["S"] == 600)
    d = R.hyp_case(c)
    B, tau = c["B"], 0.1
    st, fit, best, _, _ = _hypotheses(d, d["knn"], d["w"], tau, gpu_device)
    knn, w = d["knn"].copy(), d["w"].copy()
    for b in range(B):
        top, worst = np.nonzero(fit[b] == fit[b].max())[0], int(fit[b].argmin())
        assert fit[b, worst] < fit[b].max()
        src_row = int(best[b])
        kb, wb = d["knn"][b, src_row].copy(), d["w"][b, src_row].copy()
        for s in top:  # every natural holder of the maximum steps down ...
            knn[b, s], w[b, s] = d["knn"][b, worst], d["w"][b, worst]
        for s in layout:  # ... and the copies hold it alone
            knn[b, s], w[b, s] = kb, wb
    st2, fit2, best2, trans2, _ = _hypotheses(d, knn, w, tau, gpu_device)
    for b in range(B):
        holders = np.nonzero(fit2[b] == fit2[b].max())[0]
        assert np.array_equal(holders, sorted(layout)), (b, holders)
        for s in layout:
            assert np.array_equal(st2[b, s].view(np.uint32), st[b, best[b]].view(np.uint32))
        assert best2[b] == min(layout)
        assert np.array_equal(trans2[b].view(np.uint32), st2[b, min(layout)].view(np.uint32))


def _sq_threshold(tau):
    """sqrt_ge_threshold (pdsc_common.hpp): the smallest fp32 t with sqrtf(t) >= tau."""
    tau = f32(tau)
    t = f32(tau * tau)
    while np.sqrt(np.nextafter(t, f32(0))) >= tau:
        t = np.nextafter(t, f32(0))
    while np.sqrt(t) < tau:
        t = np.nextafter(t, f32(np.inf))
    return t


def _probe(target):
    """(dx, dy) in fp32 with fma(dy, dy, dx * dx) == target exactly: dx^2 a few ulps
    short, dy = m 2^q with m < 2^12 making up the rest (dy^2 then has <= 24 bits and
    the fp64 sum below is exact, so it rounds once, as the fma does)."""
    dx = f32(np.sqrt(np.float64(target)))
    for _ in range(4):
        dx = np.nextafter(dx, f32(0))
    base = np.float64(f32(np.float64(dx) * np.float64(dx)))
    need = np.float64(target) - base
    q = int(np.floor(np.log2(np.sqrt(need)))) - 10
    m0 = int(np.sqrt(need) / 2.0 ** q)
    for m in range(max(m0 - 64, 1), m0 + 64):
        dy = np.float64(m) * 2.0 ** q
        if f32(dy * dy + base) == target:
            return dx, f32(dy)
    raise AssertionError(f"no probe for {target!r}")


@pytest.mark.parametrize("B,S", [(1, 4), (3, 400)])  # the count inside kabsch_sums / count_inliers_kernel
@pytest.mark.parametrize("tau", R.HYP_TAUS)
def test_inlier_count_at_exact_threshold(tau, B, S, gpu_device):
    """tgt == src on a grid of small integers with equal power-of-two weights: every
    seed's H is bitwise symmetric and its pose the identity with t = 0 (asserted).
    Three rows at the origin whose squared residual is the fp32 below, at and above
    sqrt_ge_threshold(tau): `<` counts only the first, in the squared count and in
    the labels alike."""
    N, k = 67, 8
    rng = np.random.default_rng(2500 + S)
    src = rng.integers(0, 4, (B, N, 3)).astype(f32)
    tgt = src.copy()
    t2 = _sq_threshold(tau)
    targets = (np.nextafter(t2, f32(0)), t2, np.nextafter(t2, f32(np.inf)))
    assert np.sqrt(targets[0]) < f32(tau) <= np.sqrt(targets[1])
    for j, tg in enumerate(targets):
        src[:, N - 3 + j] = 0.0
        tgt[:, N - 3 + j] = (*_probe(tg), 0.0)
    knn = np.stack([np.stack([rng.permutation(N - 3)[:k] for _ in range(S)]) for _ in range(B)]).astype(np.int32)
    w = np.full((B, S, k), 0.125, f32)
    d = dict(src=src, tgt=tgt)
    st, fit, best, trans, labels = _hypotheses(d, knn, w, tau, gpu_device)
    sv = R.kabsch_fp64(src[np.arange(B)[:, None, None], knn], tgt[np.arange(B)[:, None, None], knn], w)[1]
    full = R.rank_ok(sv) & (sv[..., 2] / sv[..., 0] > 1e-3)  # a full-rank H: the rotation is unique
    assert full.mean() > 0.9
    eye = np.eye(4, dtype=f32)
    exact = np.abs(st - eye).max((-1, -2)) < 1e-12
    assert exact[full].all()
    assert (st[..., :3, 3][full] == 0).all() and (st[..., [0, 1, 2], [0, 1, 2]][full] == 1).all()
    assert np.array_equal(fit[full], np.full(int(full.sum()), f32(N - 2) / f32(N)))
    for b in range(B):
        assert full[b, best[b]]
        assert np.array_equal(labels[b, N - 3:], [1.0, 0.0, 0.0]) and labels[b].sum() == N - 2


# ------------------------------------------------------ c. post_refine
def _refine(d, rows, dev):
    from pointdsc_amd import kernels
    out = kernels.post_refine(_t(d["trans0"][rows], dev), _t(d["src"][rows], dev), _t(d["tgt"][rows], dev), d["thr"])
    return out.cpu().numpy()


@pytest.mark.parametrize("c", R.REFINE_CASES, ids=_ids(R.REFINE_CASES))
def test_post_refine_vs_fp64(c, gpu_device):
    """Five pairs that stop at different iterations in one launch: ground truth, no
    inlier (pose untouched), one inlier (properties), an offset start (>= 3 iterations),
    every row an inlier.  Pairs 0, 3, 4 within min(1e-4, ENVELOPE x e_ref + 16 x 2^-24
    max(1, |t|)) of post_refine_fp64, e_ref = the oracle's distance from fp64 on the
    pair (measured 2.1e-7 .. 2.43e-6; the kernel's own distance: 3.2e-8 .. 3.5e-7, bounds
    1.5e-6 .. 7.0e-6); the same pairs one per launch: the same bits."""
    d = R.refine_case(c)
    out = _refine(d, slice(0, 5), gpu_device)
    assert np.array_equal(out[1].view(np.uint32), d["trans0"][1].view(np.uint32))
    assert R.is_proper_rigid(out[2])
    for p in R.PINNED:
        T64, iters, near = d["ref"][p]
        assert min(near) > d["delta"]
        e_ref = R.refine_oracle(d, p)
        bound, err = R.refine_bound(d, p, e_ref, ENVELOPE), float(np.abs(out[p] - T64).max())
        print(f"{c['id']} pair {p}: {iters} iterations, |T - T64| {err:.3g} <= {bound:.3g} (e_ref {e_ref:.3g})")
        assert err <= bound
    for p in range(5):
        one = _refine(d, slice(p, p + 1), gpu_device)
        assert np.array_equal(one[0].view(np.uint32), out[p].view(np.uint32)), p


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("thr", R.REFINE_THRS)
def test_post_refine_tiny_pairs(N, thr, gpu_device):
    """(B, N) = (1, 1) and (1, 2), every row an inlier at the start: a finite proper pose."""
    from pointdsc_amd import kernels
    rng = np.random.default_rng(3100 + N)
    src, _, _, gt = R.make_pair(rng, N)
    tgt = (src.astype(np.float64) @ gt[:3, :3].astype(np.float64).T + gt[:3, 3] + 0.2 * thr).astype(f32)
    out = kernels.post_refine(_t(gt[None], gpu_device), _t(src[None], gpu_device), _t(tgt[None], gpu_device), thr)
    assert R.is_proper_rigid(out[0].cpu().numpy())


# ------------------------------------------------ d. rigid_transform_3d
@pytest.mark.parametrize("n", [1, 2])
def test_rigid_transform_tiny_sets(n, gpu_device):
    from pointdsc_amd import kernels
    rng = np.random.default_rng(3200 + n)
    A, Bp = rng.uniform(0, 3, (4, n, 3)).astype(f32), rng.uniform(0, 3, (4, n, 3)).astype(f32)
    w = rng.uniform(0.1, 1.0, (4, n)).astype(f32)
    T = kernels.rigid_transform_3d(_t(A, gpu_device), _t(Bp, gpu_device), _t(w, gpu_device)).cpu().numpy()
    for b in range(4):
        assert np.isfinite(T[b]).all() and np.array_equal(T[b, 3], [0, 0, 0, 1])
        assert_rigid(T[b], A[b].astype(np.float64), Bp[b].astype(np.float64), w[b])


def test_rigid_transform_nan_weight_stays_in_its_pair(gpu_device):
    """One NaN weight in pair 0 of 2: pair 1's pose is the oracle's within 2e-5."""
    from oracle import pdsc_oracle as O
    from pointdsc_amd import kernels
    rng = np.random.default_rng(3300)
    src, tgt, inl, _ = R.make_pair(rng, 200)
    A, Bp = np.stack([src, src[::-1]]), np.stack([tgt, tgt[::-1]])
    w = (rng.random((2, 200)) * (0.05 + np.stack([inl, inl[::-1]]))).astype(f32)
    w[0, 77] = np.nan
    T = kernels.rigid_transform_3d(_t(A, gpu_device), _t(Bp, gpu_device), _t(w, gpu_device)).cpu().numpy()
    ref = O.rigid_transform_3d(A[1:], Bp[1:], w[1:])[0]
    assert np.abs(T[1] - ref).max() <= 2e-5
