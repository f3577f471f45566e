"""tests/odometry_edge_cases.py on the CPU: every case's precondition from
tests/fragments_reference.py alone, a second restatement of f13 step 1 (a per-pixel
loop in scalar fp32 with explicit clamped indices, written from the contract
sentence) that pins preprocess() bit for bit, and the evidence that the assertions of
tests/test_gpu_odometry_edges.py reject single-rule defects: each defect is put into a
numpy model of the rule, the model without the defect is pinned to the restatement,
and the model with it falls outside the bar of at least one table case."""
import numpy as np
import pytest

import fragments_reference as R
import odometry_edge_cases as C

f32 = np.float32


# ------------------------------------------------------------------ preconditions
@pytest.mark.parametrize("mn,mx", C.DEPTH_BOUNDS)
@pytest.mark.parametrize("H,W", C.SHAPES)
def test_pyramid_case_preconditions(H, W, mn, mx):
    I, D = C.pyramid_case(H, W, mn, mx)
    ref = C.pyramid_reference(H, W, mn, mx)
    assert (D[0] == 0).sum() >= 6 and D[0][0, 0] == 0 and D[0][H - 1, W - 1] == 0 and D[0][0, W // 2] == 0
    for val in C.bound_values(mn, mx):
        assert (D[0] == val).sum() >= 1
    for l in range(3):
        assert ref[0][l]["D"].shape == (H >> l, W >> l)
        assert not np.isfinite(ref[1][l]["D"]).any() and not np.isfinite(ref[2][l]["D"]).any()
        assert np.isfinite(ref[1][l]["I"]).all()
        d3 = ref[3][l]["D"]
        assert np.isnan(d3).any() and np.isfinite(d3).any()           # NaN neighbours at every level, 2 x 2 included
        assert np.isnan(ref[3][l]["Ddx"]).any()
        assert np.isfinite(ref[3][l]["Ddx"]).any() or min(d3.shape) == 2  # at 2 x 2 every Sobel reads the NaN pixel
    assert ((D[2] > 0) & np.isfinite(D[2])).sum() == 1
    # the bounds themselves stay; one ulp outside is NaN; d <= 0 is NaN whatever min_depth is
    want = {(0.0, 4.0): [False, False, True, True, True, False], (0.5, 2.5): [True, False, True, True, True, False]}
    for k, (val, kept) in enumerate(zip(C.bound_values(mn, mx), want[(mn, mx)])):
        assert C.bound_kept(val, mn, mx) == kept, C.BOUND_FRAMES[k]
        d0 = ref[4 + k][0]["D"]
        if kept:
            assert np.isfinite(d0).all(), C.BOUND_FRAMES[k]
        else:
            nan = np.argwhere(np.isnan(d0))
            assert len(nan) == 9 and np.all(np.abs(nan - [H // 2, W // 2]) <= 1), C.BOUND_FRAMES[k]


@pytest.mark.parametrize("H,W", C.SHAPES)
def test_lin_case_preconditions(H, W):
    """Every level, the 2 x 2 one included, has a correspondence and a target pixel without one."""
    nan_grad = 0
    for level in range(3):
        JtJ, Jtr, n, aJJ, aJr, corr, (a_s, a_t) = C.lin_reference(H, W, level)
        assert n >= 1 and (corr < 0).sum() >= 1, (level, n)
        assert np.isfinite(JtJ).all() and np.isfinite(Jtr).all() and abs(a_t - 1.0) > 1e-3
        I, D, K, T = C.lin_case(H, W)
        Lt = R.preprocess(I[1], D[1])[level]
        j = np.nonzero(corr >= 0)[0]
        nan_grad += int(np.isnan(Lt["Ddx"].reshape(-1)[j]).sum() + np.isnan(Lt["Ddy"].reshape(-1)[j]).sum())
    if (H, W) != (8, 8):
        assert nan_grad > 0  # "NaN gradients count as 0" decides a sum


def test_rounding_case_preconditions():
    """Some target pixel receives source pixels whose fp64 p.z differ and whose fp32
    roundings are equal, the lowest index having the largest fp64 p.z; the contract
    keeps that index, a key on fp64 p.z another."""
    I, D, K, T = C.rounding_case()
    corr, P = C.map_reference("rounding")
    H, W = D.shape[1:]
    ok, uf, vf, pz = C.projections(P[0][0], K, T)
    assert ok.all() and np.all((uf > 0) & (uf < W) & (vf > 0) & (vf < H))
    tgt = vf.astype(np.int64) * W + uf.astype(np.int64)
    assert len(np.unique(pz.astype(f32))) == 1 and len(np.unique(pz)) > 1
    n_decided = 0
    for j in np.nonzero(corr >= 0)[0]:
        src = np.nonzero(tgt == j)[0]
        assert corr[j] == src.min()                                   # ties on the fp32 key: the lowest index
        if len(src) >= 2 and pz[src.min()] > pz[src].min():
            assert pz[src.min()] == pz[src].max()
            n_decided += 1
    assert n_decided >= 16
    assert not np.array_equal(_model_corr(P[0][0], P[1][0], K, T, "key_fp64"), corr)


def test_truncation_case_preconditions():
    I, D, K, T = C.truncation_case()
    corr, P = C.map_reference("truncation")
    H, W = D.shape[1:]
    ok, uf, vf, pz = C.projections(P[0][0], K, T)
    inside = ok & (uf > -1.0) & (uf < W) & (vf > -1.0) & (vf < H)
    accepted = np.zeros(H * W, bool)
    accepted[corr[corr >= 0]] = True
    assert (accepted & (uf > -1.0) & (uf < 0.0)).sum() > 0 and (accepted & (vf > -1.0) & (vf < 0.0)).sum() > 0
    assert (ok & (uf >= W)).sum() > 0 and (ok & (vf >= H)).sum() > 0 and not accepted[ok & ~inside].any()
    col0, row0 = corr.reshape(H, W)[:, 0], corr.reshape(H, W)[0, :]
    assert np.any(uf[col0[col0 >= 0]] < 0.0) and np.any(vf[row0[row0 >= 0]] < 0.0)  # such pixels win column 0 and row 0


def test_failing_pair_fails_at_its_first_iteration():
    P = C.scene_pyramids()
    for init in (None, C.INITS[0]):
        T, info, ok, n, runs = R.odometry_pair(P[0], P[4], C.SCENE_K, init, C.MDD, C.BATCH_ITERATIONS)
        assert not ok and runs == 0 and n == 0 and not info.any()
        assert np.array_equal(T, np.eye(4) if init is None else init)
    assert not np.isfinite(P[4][2]["D"]).any()
    for s, t in C.GOOD_PAIRS + C.REVERSE_BATCH + C.UNNAMED_PAIRS:
        T, info, ok, n, runs = R.odometry_pair(P[s], P[t], C.SCENE_K, None, C.MDD, C.BATCH_ITERATIONS)
        assert ok and runs == sum(C.BATCH_ITERATIONS) and n > 100, (s, t)


def test_step_case_preconditions():
    """Every one-iteration case succeeds in the restatement on a well-conditioned system;
    no iteration at all returns init, success and the level-0 information."""
    P = C.scene_pyramids()
    for name, (s, t), its, init in C.STEP_CASES:
        T, info, ok, n, runs = C.step_reference(name)
        assert ok and runs == 1 and n > 100 and sum(its) == 1
        T0 = np.eye(4) if init is None else init
        assert 1e-5 < np.abs(T - T0).max() < 0.1                      # the step moves the pose by more than any bar
    for name, (s, t), init in C.ZERO_CASES:
        T, info, ok, n, runs = C.step_reference(name)
        assert ok and runs == 0 and n == 0                            # f13: success = no iteration failed
        assert np.array_equal(T, np.eye(4) if init is None else init)
        assert info.any() == (t != 4)


def test_conversion_case_preconditions():
    c, d = C.convert_case()
    for trunc in C.CONVERT_TRUNCS:
        inten, dep = R.rgbd_from_color_and_depth(c, d, C.CONVERT_SCALE, trunc)
        assert dep[d == 3000][0] == f32(3.0) and dep[d == 0][0] == 0
        assert (dep[d == 3001][0] == 0) == (trunc == 3.0) and (dep[d == 32768][0] == 0) == (trunc == 3.0)
        assert inten.min() == 0.0 and inten.max() <= 1.0 and inten[0, 0, 7] == inten.max()
    assert dep[d == 65535][0] == f32(65535) / f32(1000) and dep[d == 32768][0] == f32(32.768)
    assert (d.view(np.int16) < 0).sum() == 8


# ------------------------------------------------------------------ step 1, a second time
def _clampi(x, hi):
    return 0 if x < 0 else (hi if x > hi else x)


def _tap(a, b, c):
    return f32(f32(f32(0.25) * a + f32(0.5) * b) + f32(0.25) * c)


class LoopPyramid:
    """f13 step 1 pixel by pixel: scalar fp32, explicit clamped indices.  `defect` breaks one rule."""

    def __init__(self, defect=None):
        self.defect = defect

    def read(self, img, v, u):
        H, W = img.shape
        if self.defect == "zero_pad" and not (0 <= v < H and 0 <= u < W):
            return f32(0)
        return img[_clampi(v, H - 1), _clampi(u, W - 1)]

    def clip(self, d, mn, mx):
        if self.defect == "bounds_le":
            return f32(np.nan) if (d <= mn or d >= mx or d <= 0) else d
        return f32(np.nan) if (d < mn or d > mx or d <= 0) else d

    def gauss(self, img):
        H, W = img.shape
        out = np.empty((H, W), f32)
        for v in range(H):
            for u in range(W):
                h = [_tap(self.read(img, r, u - 1), self.read(img, r, u), self.read(img, r, u + 1))
                     for r in (v - 1, v, v + 1)]
                out[v, u] = _tap(h[0], h[1], h[2])
        return out

    def down(self, img):
        H, W = img.shape[0] // 2, img.shape[1] // 2
        out = np.empty((H, W), f32)
        for v in range(H):
            for u in range(W):
                p00, p10, p01, p11 = img[2 * v, 2 * u], img[2 * v, 2 * u + 1], img[2 * v + 1, 2 * u], img[2 * v + 1, 2 * u + 1]
                if self.defect == "sum_order":
                    out[v, u] = f32(f32(f32(f32(p00 + p01) + p10) + p11) * f32(0.25))
                else:
                    out[v, u] = f32(f32(f32(f32(p00 + p10) + p01) + p11) * f32(0.25))
        return out

    def sobel(self, img):
        H, W = img.shape
        dx, dy = np.empty((H, W), f32), np.empty((H, W), f32)
        for v in range(H):
            for u in range(W):
                h = [f32(self.read(img, r, u + 1) - self.read(img, r, u - 1)) for r in (v - 1, v, v + 1)]
                k = [f32(self.read(img, v + 1, c) - self.read(img, v - 1, c)) for c in (u - 1, u, u + 1)]
                dx[v, u] = f32(f32(h[0] + f32(f32(2) * h[1])) + h[2])
                dy[v, u] = f32(f32(k[0] + f32(f32(2) * k[1])) + k[2])
        return dx, dy

    def __call__(self, intensity, depth, mn, mx):
        with np.errstate(invalid="ignore", over="ignore"):
            H, W = depth.shape
            d = np.array([[self.clip(depth[v, u], f32(mn), f32(mx)) for u in range(W)] for v in range(H)], f32)
            I, D = self.gauss(intensity), self.gauss(d)
            out = []
            for l in range(3):
                if l:
                    I = self.down(self.gauss(I))
                    D = self.down(self.gauss(D) if self.defect == "depth_refiltered" else D)
                Idx, Idy = self.sobel(I)
                Ddx, Ddy = self.sobel(D)
                out.append(dict(I=I, D=D, Idx=Idx, Idy=Idy, Ddx=Ddx, Ddy=Ddy))
            return out


LOOP_SHAPES = C.SHAPES[:2]


def _pyramid_differs(defect):
    """Does tests/test_gpu_odometry_edges.py's pyramid assertion reject a step 1 with `defect`?  On the two smallest shapes."""
    hits = 0
    for H, W in LOOP_SHAPES:
        for mn, mx in C.DEPTH_BOUNDS:
            I, D = C.pyramid_case(H, W, mn, mx)
            ref = C.pyramid_reference(H, W, mn, mx)
            for f in range(len(I)):
                got = LoopPyramid(defect)(I[f], D[f], mn, mx)
                for l in range(3):
                    for name in C.IMAGES:
                        try:
                            C.assert_images_bitwise(got[l][name], ref[f][l][name], f"{H}x{W} frame {f} L{l} {name}")
                        except AssertionError:
                            hits += 1
    return hits


def test_preprocess_is_the_per_pixel_loop_bit_for_bit():
    assert _pyramid_differs(None) == 0


@pytest.mark.parametrize("defect", ["zero_pad", "depth_refiltered", "sum_order", "bounds_le"])
def test_pyramid_defect_is_rejected(defect):
    assert _pyramid_differs(defect) > 0


# ------------------------------------------------------------------ models of steps 3 .. 5 with one rule broken
def _model_corr(Ls, Lt, K, T, defect=None):
    """f13 step 3, target pixel by target pixel from the definition (no atomic-min key)."""
    H, W = Ls["D"].shape
    ok, uf, vf, pz = C.projections(Ls, K, T)
    dt = Lt["D"].reshape(-1).astype(np.float64)
    cand = [[] for _ in range(H * W)]
    for i in np.nonzero(ok)[0]:
        if not (-1.0 < uf[i] < W and -1.0 < vf[i] < H):
            continue
        ut, vt = (int(np.floor(uf[i])), int(np.floor(vf[i]))) if defect == "floor" else (int(uf[i]), int(vf[i]))
        if ut < 0 or vt < 0:
            continue  # the floor defect's column -1: outside the image
        j = vt * W + ut
        if np.isfinite(dt[j]) and abs(pz[i] - dt[j]) <= C.MDD:
            cand[j].append(i)
    corr = np.full(H * W, -1, np.int64)
    for j, c in enumerate(cand):
        if c:
            z = pz[c] if defect == "key_fp64" else pz[c].astype(f32)
            tied = [i for i, zi in zip(c, z) if zi == z.min()]
            corr[j] = max(tied) if defect == "tie_highest" else min(tied)
    return corr


def _model_sums(Ls, Lt, K, T, a_s, a_t, defect=None):
    """f13 steps 4 and 5's sums, correspondence by correspondence in scalar fp64."""
    fx, fy, cx, cy = K
    W = Ls["D"].shape[1]
    corr = _model_corr(Ls, Lt, K, T)
    si, sd = np.sqrt(1.0 - R.LAMBDA_DEP), np.sqrt(R.LAMBDA_DEP)
    JtJ, Jtr = np.zeros((6, 6)), np.zeros(6)
    g = (lambda x: float(x)) if defect == "nan_gradients" else (lambda x: 0.0 if np.isnan(x) else float(x))
    for j in np.nonzero(corr >= 0)[0]:
        i = corr[j]
        d = float(Ls["D"].reshape(-1)[i])
        px, py, pz = R.apply_T(T, ((i % W - cx) * d) / fx, ((i // W - cy) * d) / fy, d)
        sI = R.SOBEL_SCALE * (1.0 if defect == "no_a_t" else a_t)
        c0, c1 = sI * g(Lt["Idx"].reshape(-1)[j]) * fx / pz, sI * g(Lt["Idy"].reshape(-1)[j]) * fy / pz
        c2 = -(c0 * px + c1 * py) / pz
        d0 = R.SOBEL_SCALE * g(Lt["Ddx"].reshape(-1)[j]) * fx / pz
        d1 = R.SOBEL_SCALE * g(Lt["Ddy"].reshape(-1)[j]) * fy / pz
        d2 = -(d0 * px + d1 * py) / pz
        JI = si * np.array([-pz * c1 + py * c2, pz * c0 - px * c2, -py * c0 + px * c1, c0, c1, c2])
        JD = sd * np.array([-pz * d1 + py * d2 - py, pz * d0 - px * d2 + px, -py * d0 + px * d1, d0, d1, d2 - 1.0])
        rI = si * (a_t * float(Lt["I"].reshape(-1)[j]) - a_s * float(Ls["I"].reshape(-1)[i]))
        rD = sd * (float(Lt["D"].reshape(-1)[j]) - pz)
        JtJ += np.outer(JI, JI) + np.outer(JD, JD)
        Jtr += JI * rI + JD * rD
    return JtJ, Jtr


def _sums_within_bar(JtJ, Jtr, ref):
    """tests/test_gpu_odometry_edges.py's sums assertion."""
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.abs(JtJ - ref[0]) <= 1e-9 * ref[3]) and np.all(np.abs(Jtr - ref[1]) <= 1e-9 * ref[4]))


LIN_MODEL_CASES = [(H, W, l) for H, W in C.SHAPES[:5] for l in range(3)]


def _lin_levels(H, W, level):
    I, D, K, T = C.lin_case(H, W)
    P = [R.preprocess(I[f], D[f]) for f in range(2)]
    return P[0][level], P[1][level], R.level_K(K, level), T


def test_models_are_the_restatement():
    for H, W, l in LIN_MODEL_CASES:
        Ls, Lt, K, T = _lin_levels(H, W, l)
        ref = C.lin_reference(H, W, l)
        assert np.array_equal(_model_corr(Ls, Lt, K, T), ref[5])
        assert _sums_within_bar(*_model_sums(Ls, Lt, K, T, *ref[6]), ref)
    for which, case in (("rounding", C.rounding_case), ("truncation", C.truncation_case)):
        corr, P = C.map_reference(which)
        assert np.array_equal(_model_corr(P[0][0], P[1][0], case()[2], case()[3]), corr)


@pytest.mark.parametrize("defect,which", [("floor", "truncation"), ("key_fp64", "rounding"), ("tie_highest", "rounding")])
def test_map_defect_is_rejected(defect, which):
    """`corr` exact rejects it on the case built for it."""
    case = {"rounding": C.rounding_case, "truncation": C.truncation_case}[which]()
    corr, P = C.map_reference(which)
    assert not np.array_equal(_model_corr(P[0][0], P[1][0], case[2], case[3], defect), corr)


@pytest.mark.parametrize("defect", ["nan_gradients", "no_a_t"])
def test_sums_defect_is_rejected(defect):
    rejected = 0
    for H, W, l in LIN_MODEL_CASES:
        Ls, Lt, K, T = _lin_levels(H, W, l)
        ref = C.lin_reference(H, W, l)
        rejected += not _sums_within_bar(*_model_sums(Ls, Lt, K, T, *ref[6], defect), ref)
    assert rejected >= 3


def test_init_of_pair_0_for_every_pair_is_rejected():
    """The batch assertion is bitwise equality with the single call under init[p]: a pair run
    under init[0] instead ends more than the step bar away, at every BATCH_ITERATIONS."""
    P = C.scene_pyramids()
    pairs, inits = C.INIT_BATCH
    for p in (1, 2):
        s, t = pairs[p]
        own = R.odometry_pair(P[s], P[t], C.SCENE_K, inits[p], C.MDD, C.BATCH_ITERATIONS)
        wrong = R.odometry_pair(P[s], P[t], C.SCENE_K, inits[0], C.MDD, C.BATCH_ITERATIONS)
        assert own[2] and wrong[2] and np.abs(own[0] - wrong[0]).max() > 1e-6
    assert pairs[0] == pairs[2] and not np.array_equal(inits[0], inits[2])
