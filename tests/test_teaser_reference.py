"""tests/teaser_reference.py held to brute force and planted truths on the CPU,
and the seeds of tests/test_gpu_teaser.py held to the conditions that make its
exact comparisons meaningful (no final residual on a threshold; the best TLS
cost separated from every other window's)."""
import numpy as np
import pytest

import fr_reference as F
import teaser_reference as T
from pointdsc_amd.synthetic import PRESETS, synthetic_pair

NB = 0.3


# ---------------------------------------------------------------- scalar TLS
@pytest.mark.parametrize("K", [1, 2, 3, 17, 200])
def test_tls_scalar_equals_brute_force(K):
    for seed in range(3):
        rng = np.random.RandomState(31 * K + seed)
        x = np.concatenate([1.5 + 0.2 * rng.randn(K - K // 3), rng.uniform(-6, 6, K // 3)])[rng.permutation(K)]
        a, b = T.tls_scalar(x, NB), T.tls_scalar_brute(x, NB)
        assert abs(a - b) <= 1e-12, (K, seed, a, b)


def test_tls_tie_rule_and_duplicates():
    # a leave sorts before an enter of the same value (negative tag): 0 and 0.6 never share a set
    assert T.tls_scalar(np.array([0.0, 0.6]), NB) == 0.0  # two sets of one, equal cost: the first event wins
    x = np.array([1.0, 1.0, 1.0, 5.0])
    assert T.tls_scalar(x, NB) == 1.0 and T.tls_scalar_brute(x, NB) == 1.0


# ------------------------------------------------------------------------ GNC
def test_svd_rot_equals_lapack_where_determined():
    rng = np.random.RandomState(0)
    for _ in range(50):
        H = rng.randn(3, 3)
        assert np.abs(T.svd_rot(H) - T.svd_rot_lapack(H)).max() < 1e-10
    a, b = rng.randn(2, 3), rng.randn(2, 3)  # rank 2
    H = np.outer(a[0], b[0]) + np.outer(a[1], b[1])
    assert np.abs(T.svd_rot(H) - T.svd_rot_lapack(H)).max() < 1e-9
    R1 = T.svd_rot(np.outer(a[0], b[0]))  # rank 1: a rotation taking a to b's direction
    assert np.abs(R1 @ R1.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R1) - 1) < 1e-12
    assert np.abs(R1 @ a[0] / np.linalg.norm(a[0]) - b[0] / np.linalg.norm(b[0])).max() < 1e-12
    assert np.array_equal(T.svd_rot(np.zeros((3, 3))), np.eye(3))


def test_gnc_recovers_planted_rotation_through_all_branches():
    a, b, R, out = T.tim_case(200, 0, NB)
    trace = []
    g = T.gnc_tls_rotation(a, b, NB, trace=trace)
    assert any(z > 0 and o > 0 and m > 0 for z, o, m in trace), trace  # one pass uses all three branches
    assert 1 < g["iterations"] < 10000 and g["stop_reason"] == 2
    assert np.array_equal(g["inliers"], ~out)
    # 140 inlier TIMs of ~5 m with 0.09 m of noise: the rotation is good to about 0.09 / 5 / sqrt(140)
    assert np.abs(g["R"] - R).max() < 5e-3


def test_gnc_degenerate_cases():
    a, b, R, _ = T.tim_case(300, 0, NB, noise=0.0, outliers=0.0)
    g = T.gnc_tls_rotation(a, b, NB)
    assert g["iterations"] == 1 and g["stop_reason"] == 1 and (g["weights"] == 1).all()
    assert np.abs(g["R"] - R).max() < 1e-12
    g = T.gnc_tls_rotation(a, b, NB, max_iterations=1)
    assert g["iterations"] == 1
    src = np.random.RandomState(1).rand(5, 3).astype(np.float32)
    for members in ([], [3]):
        s = T.solve_on_members(src, src, members, NB)
        assert s["valid"] == 0 and np.array_equal(s["trans"], np.eye(4)) and not s["labels"].any()
    s = T.solve_on_members(src, src + np.float32(1.0), [1, 4], NB)  # Kc = 2: two opposite TIMs
    assert s["valid"] == 1 and np.abs(s["trans"][:3, 3] - 1.0).max() < 1e-6 and s["labels"].sum() == 2


# ----------------------------------------------------------------- whole solve
def test_whole_solve_within_the_planted_noise():
    tau = PRESETS["3dmatch"]["inlier_threshold"]
    p = synthetic_pair(300, seed=300)
    m = T.greedy_clique(T.length_graph(p["src_keypts"], p["tgt_keypts"], 2 * tau))
    assert p["gt_labels"][m].all() and len(m) >= 60
    s = T.solve_on_members(p["src_keypts"], p["tgt_keypts"], m, tau)
    # per-axis noise 0.1 tau over >= 60 inliers in a 3 m box: a few millimetres at the far corner
    assert s["valid"] == 1 and np.abs(s["trans"] - p["gt_trans"]).max() < 0.1 * tau
    assert np.array_equal(np.flatnonzero(s["labels"]), m)


# --------------------------------------------------------- the GPU test's seeds
def test_gpu_rotation_seeds_have_no_residual_on_a_threshold():
    import test_gpu_teaser as G
    for K, kw, seed in G.ROT_CASES:
        if K > 1100:
            continue  # K = 8192 is asserted by the GPU test itself (seconds here)
        a, b, _, _ = T.tim_case(K, seed, NB, **kw)
        g = T.gnc_tls_rotation(a, b, NB)
        assert G.residuals_off_threshold(g), (K, kw, seed)
        assert g["iterations"] < 10000


def test_gpu_translation_seeds_are_separated():
    import test_gpu_teaser as G
    for K, dup, seed in G.TLS_CASES:
        if K > 1100:
            continue
        src, dst, _ = T.offset_case(K, seed, NB, dup)
        assert G.tls_separated(src, dst), (K, dup, seed)


def test_gpf_bb_first_restatement():
    f0, f1, xyz0 = F.desc_case(3, 300, 280, 32)
    full = T.gpf_bb_first(f0, f1, xyz0, 10, 10 ** 6)
    assert full["early"] and len(full["idx0"]) > 20
    half = T.gpf_bb_first(f0, f1, xyz0, 10, len(full["idx0"]) // 2)
    assert not half["early"] and set(half["idx0"]) <= set(full["idx0"])
    assert abs(len(half["idx0"]) - len(full["idx0"]) // 2) <= 0.2 * len(full["idx0"])
