"""TEASER++ on the GPU (include/pdsc.h f9; pointdsc_amd/csrc/teaser.hip,
pointdsc_amd/kernels.py, matching.py, teaser.py) against the fp64 restatement
tests/teaser_reference.py.

Tolerances.  The kernels sum in a tree where the restatement sums one term
after the other, so the yardstick is the restatement's own spread under
reordering: each listed input was run with its TIM order permuted 20 times and
the largest |dR| / |dt| against the unpermuted run recorded (DESIGN.md §7
"TEASER++" has the table); the tolerance is 10 x that maximum per stage.
  rotation stage   max |dR| 2.11e-15 (K = 8192)            -> ROT_R_TOL
  whole solve      max |dR| 4.44e-16, max |dt| 6.66e-16     -> SOLVE_*_TOL
                   (the chain's TIMs permuted inside the rotation stage)
No case's iteration count differed between permutations.
The translation stage has NO spread: the restatement walks the sorted events,
so the order of its running sums does not depend on the order of the input and
all 20 permutations gave the same bits.  10 x 0 would ask for bit equality
between two different formulas (running sums / n against median + prefix
difference / n), so that stage is held to the restatement's own rounding error
instead: each of its at most 2K running-sum updates rounds a partial sum of at
most n max|x|, and the sum is divided by n: |error of xhat| <= 2 K u max|x|,
u = 2^-53 (tls_tol below; 1.8e-12 at K = 8192, 2e-16 at K = 1)."""
import types

import numpy as np
import pytest
import torch

import fr_reference as F
import teaser_reference as T
from pointdsc_amd.synthetic import PRESETS, synthetic_pair

pytestmark = pytest.mark.gpu

NB = 0.3
ROT_R_SPREAD, ROT_R_TOL = 2.11e-15, 2.11e-14
SOLVE_R_SPREAD, SOLVE_R_TOL = 4.44e-16, 4.44e-15
SOLVE_T_SPREAD, SOLVE_T_TOL = 6.66e-16, 6.66e-15
TLS_T_SPREAD = 0.0
U = 2.0 ** -53

KS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 8192)
# (K, tim_case keywords, seed): every seed checked on the CPU (test_teaser_reference.py; K = 8192 below)
ROT_CASES = [(K, {}, 0) for K in KS] + [(300, dict(noise=0.0, outliers=0.0), 0), (300, dict(outliers=1.0), 0)]
# (K, duplicated values, seed)
TLS_CASES = [(K, False, 0) for K in KS] + [(300, True, 0)]
SOLVE_NS = (2, 64, 65, 300, 1100)


def tls_tol(K, x):
    return 2 * K * U * float(np.abs(x).max())


def residuals_off_threshold(g):
    """No final r_j within a relative 1e-6 of noise_bound^2 (so w_j >= 0.5 is decided away from rounding)."""
    nb2 = NB * NB
    return not (np.abs(g["residuals"] - nb2) <= 1e-6 * nb2).any()


def tls_separated(src, dst):
    """Per axis: the best cost is a relative 1e-9 below the best of any other window."""
    for c in range(3):
        _, best, other = T.tls_scalar((dst - src)[:, c], NB, detail=True)
        if not (other == np.inf or other - best > 1e-9 * abs(best)):
            return False
    return True


def _np(t):
    return t.cpu().numpy()


def _t(a, dev, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(*ts):
    return [_np(t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t).tobytes() for t in ts]


# ------------------------------------------------------------------- rotation
@pytest.mark.parametrize("K,kw,seed", ROT_CASES, ids=[f"K{K}" + "".join(f"-{k}{v}" for k, v in kw.items())
                                                     for K, kw, _ in ROT_CASES])
def test_rotation_stage(K, kw, seed, gpu_device):
    from pointdsc_amd import kernels as Kn
    a, b, _, _ = T.tim_case(K, seed, NB, **kw)
    ref = T.gnc_tls_rotation(a, b, NB)
    assert residuals_off_threshold(ref)
    out = Kn.gnc_tls_rotation(_t(a, gpu_device), _t(b, gpu_device), NB)
    R, w, inl, info = out
    gi = Kn.GncInfo(info)
    Rn = _np(R)
    err = np.abs(Rn - ref["R"]).max()
    print(f"K={K} iterations gpu {gi.iterations} ref {ref['iterations']} |dR| {err:.3g} tol {ROT_R_TOL:.3g}")
    assert abs(gi.iterations - ref["iterations"]) <= 1 and gi.iterations < 10000
    assert gi.stop_reason == ref["stop_reason"]
    assert err <= ROT_R_TOL
    assert np.array_equal(_np(inl) != 0, ref["inliers"])
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rn) - 1.0) <= 1e-12
    again = Kn.gnc_tls_rotation(_t(a, gpu_device), _t(b, gpu_device), NB)
    assert _bits(R, w, info, inl) == _bits(again[0], again[1], again[3], again[2])


def test_rotation_max_iterations(gpu_device):
    from pointdsc_amd import kernels as Kn
    a, b, _, _ = T.tim_case(257, 0, NB)
    for n in (1, 3):
        ref = T.gnc_tls_rotation(a, b, NB, max_iterations=n)
        R, w, inl, info = Kn.gnc_tls_rotation(_t(a, gpu_device), _t(b, gpu_device), NB, max_iterations=n)
        gi = Kn.GncInfo(info)
        assert gi.iterations == n == ref["iterations"] and gi.stop_reason == 0
        assert np.abs(_np(R) - ref["R"]).max() <= ROT_R_TOL
        assert np.abs(_np(w) - ref["weights"]).max() <= 1e-9


# ---------------------------------------------------------------- translation
@pytest.mark.parametrize("K,dup,seed", TLS_CASES, ids=[f"K{K}" + ("-dup" if d else "") for K, d, _ in TLS_CASES])
def test_translation_stage(K, dup, seed, gpu_device):
    from pointdsc_amd import kernels as Kn
    src, dst, _ = T.offset_case(K, seed, NB, dup)
    assert tls_separated(src, dst)
    t_ref, inl_ref = T.tls_translation(src, dst, NB)
    t, inl = Kn.tls_translation(_t(src, gpu_device), _t(dst, gpu_device), NB)
    err, tol = np.abs(_np(t) - t_ref).max(), tls_tol(K, dst - src)
    print(f"K={K} dup={dup} |dt| {err:.3g} tol {tol:.3g}")
    assert err <= tol
    assert np.array_equal(_np(inl) != 0, inl_ref)
    again = Kn.tls_translation(_t(src, gpu_device), _t(dst, gpu_device), NB)
    assert _bits(t, inl) == _bits(*again)


# ----------------------------------------------------------------- whole solve
@pytest.mark.parametrize("N", SOLVE_NS)
def test_whole_solve(N, gpu_device):
    from pointdsc_amd import kernels as Kn
    tau = PRESETS["3dmatch"]["inlier_threshold"]
    p = synthetic_pair(N, seed=N)
    src, tgt = p["src_keypts"], p["tgt_keypts"]
    s, t = _t(src, gpu_device, np.float32), _t(tgt, gpu_device, np.float32)
    trans, t32, labels, result = Kn.teaser_solve(s, t, tau)
    info = Kn.TeaserInfo(result)
    adj, _ = Kn.consistency_graph(torch.cat([s, t], 1), 2 * tau, "length")
    members, clabels, cres = Kn.max_clique(adj)
    ci = Kn.CliqueInfo(cres)
    assert info.clique_size == ci.size and info.clique_exact == ci.exact
    m = _np(members)[:ci.size]
    ref = T.solve_on_members(src, tgt, m, tau)
    Tn = _np(trans)
    assert info.valid == ref["valid"]
    dR, dt = np.abs(Tn[:3, :3] - ref["trans"][:3, :3]).max(), np.abs(Tn[:3, 3] - ref["trans"][:3, 3]).max()
    print(f"N={N} clique {ci.size} |dR| {dR:.3g} (tol {SOLVE_R_TOL:.3g}) |dt| {dt:.3g} (tol {SOLVE_T_TOL:.3g})")
    assert dR <= SOLVE_R_TOL and dt <= SOLVE_T_TOL
    assert np.array_equal(Tn[3], [0, 0, 0, 1]) and np.array_equal(_np(t32), Tn.astype(np.float32))
    assert np.array_equal(_np(labels), ref["labels"])
    if ref["valid"]:
        assert info.gnc_iterations == ref["gnc"]["iterations"]
        assert info.n_translation_inliers == int(ref["t_inliers"].sum())
        assert info.n_rotation_inliers == int(ref["gnc"]["inliers"].sum())
        # the planted noise is 0.1 tau per axis: an estimate over the clique's points stays inside 3 sigma of one point
        assert np.abs(Tn - p["gt_trans"]).max() < 3 * 0.1 * tau
    again = Kn.teaser_solve(s, t, tau)
    assert _bits(trans, t32, labels, result) == _bits(*again)


def test_whole_solve_without_edges(gpu_device):
    from pointdsc_amd import kernels as Kn
    rng = np.random.RandomState(8)
    src = (np.arange(8)[:, None] * 10.0 + rng.rand(8, 3)).astype(np.float32)
    tgt = (np.arange(8)[:, None] ** 2 * 7.0 + rng.rand(8, 3)).astype(np.float32)
    assert not T.length_graph(src, tgt, 2 * NB).any()
    trans, t32, labels, result = Kn.teaser_solve(_t(src, gpu_device, np.float32), _t(tgt, gpu_device, np.float32), NB)
    info = Kn.TeaserInfo(result)
    assert info.valid == 0 and info.clique_size == 1 and info.gnc_iterations == 0
    assert np.array_equal(_np(trans), np.eye(4)) and np.array_equal(_np(t32), np.eye(4, dtype=np.float32))
    assert not _np(labels).any()


# ----------------------------------------------------------------------- GPF
@pytest.mark.parametrize("N0", [50, 700])
def test_gpf_bb_first(N0, gpu_device):
    from pointdsc_amd import matching as M
    N1 = N0 - N0 // 10
    f0, f1, xyz0 = F.desc_case(F.tie_free_seed(N0, N1, 32, 10, 1.0), N0, N1, 32)
    d = [_t(x, gpu_device, np.float32) for x in (f0, f1, xyz0)]
    idx0, idx1, idx2, _ = M.find_2nn(d[0], d[1])
    n_mutual = len(T.gpf_bb_first(f0, f1, xyz0, 10, 10 ** 9)["idx0"])
    for total in (n_mutual + 5, n_mutual, max(1, n_mutual // 2)):
        ref = T.gpf_bb_first(f0, f1, xyz0, 10, total)
        args = types.SimpleNamespace(GPF_grid_wid=10, GPF_max_matches=total)
        out = M.Grid_Prioritized_Filter(d[0], d[1], idx0, idx1, idx2, d[2], args, BB_first=True)
        assert len(out) == 7 and (out[6] is None) == ref["early"]
        assert np.array_equal(_np(out[0]), ref["idx0"]) and np.array_equal(_np(out[1]), ref["idx1"])
        assert np.array_equal(_np(out[2]), _np(idx2)[ref["idx0"]])
        assert out[3] is idx0 and out[4] is idx1 and out[5] is idx2


# --------------------------------------------------------------------- TEASER
def test_teaser_end_to_end(gpu_device):
    from pointdsc_amd import TEASER
    xyz0, xyz1, f0, f1, T_gt = F.planted_registration(F.planted_seed())
    dev_in = [_t(x, gpu_device, np.float32) for x in (xyz0, xyz1, f0, f1)]
    for mode in (None, "FAIL_TOLERANT"):
        args = types.SimpleNamespace(GPF_grid_wid=10, GPF_max_matches=5000, mode=mode)
        Tm, elapsed = TEASER(*dev_in, args)
        err = np.abs(_np(Tm) - T_gt).max()
        print("mode", mode, "max |T - planted|:", err)
        assert Tm.dtype == torch.float64 and elapsed > 0 and err <= 1e-3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TEASER(*(torch.from_numpy(x) for x in (xyz0, xyz1, f0, f1)), args)


def test_teaser_rejects_too_many_pairs(monkeypatch, gpu_device):
    from pointdsc_amd import matching, teaser
    xyz0, xyz1, f0, f1, _ = F.planted_registration(0, N=64)
    dev_in = [_t(x, gpu_device, np.float32) for x in (xyz0, xyz1, f0, f1)]
    stub = torch.zeros(8193, dtype=torch.int64, device=gpu_device)
    monkeypatch.setattr(matching, "Grid_Prioritized_Filter", lambda *a, **k: (stub, stub, stub, None, None, None, None))
    with pytest.raises(ValueError, match="GPF_max_matches"):
        teaser.TEASER(*dev_in, types.SimpleNamespace(GPF_grid_wid=10, GPF_max_matches=10 ** 6, mode=None))
