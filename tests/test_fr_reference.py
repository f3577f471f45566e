"""tests/fr_reference.py (the fp64 restatement of include/pdsc.h f7) against the
goldens recorded from the reference's algorithms/matching.py
(tools/gen_fr_goldens.py -> tests/golden/fr), its near-tie conditions, and the
water-filling loop on hand-made count tables.  CPU only."""
import os

import numpy as np
import pytest

import fr_reference as F
from conftest import GOLDEN


def _golden(name):
    with np.load(os.path.join(GOLDEN, "fr", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(F.GOLDEN_CASES))
def test_goldens(name):
    g = _golden(name)
    N0, N1, D, G, factor = F.GOLDEN_CASES[name]
    assert g["f0"].shape == (N0, D) and g["f1"].shape == (N1, D) and int(g["grid"]) == G and float(g["factor"]) == factor
    f0, f1, xyz0 = F.desc_case(int(g["seed"]), N0, N1, D)
    assert np.array_equal(f0, g["f0"]) and np.array_equal(f1, g["f1"]) and np.array_equal(xyz0, g["xyz0"])
    m_nn, m_cell, m_gpf, (nn, mr, gp) = F.case_margins(f0, f1, xyz0, G, factor)
    print("margins (x twice the fp32 bound): nn", m_nn, "cell", m_cell, "gpf", m_gpf)
    assert min(m_nn, m_cell, m_gpf) > 1.0  # the generator's condition, again
    assert np.array_equal(nn["nn1"], g["nn1"]) and np.array_equal(nn["nn2"], g["nn2"])
    assert np.array_equal(np.flatnonzero(mr["is_bb"]), g["mutual_idx0"])
    assert np.array_equal(g["nn1"][g["mutual_idx0"]], g["mutual_idx1"])
    assert np.array_equal(mr["is_bb"], g["is_bb"]) and mr["num_bb"] == int(g["num_bb"])
    # ratios to fp32 resolution: the reference's torch fp32 against fp64
    rel = np.abs(g["feat_dist"] - mr["feat_dist"]) / mr["feat_dist"]
    err = np.abs(g["norm_feat_dist"] - mr["norm"]).max()
    print("feat_dist relative:", rel.max(), "bound", F.ratio_rel(D), " norm:", err, "bound", mr["norm_bound"])
    assert rel.max() <= F.ratio_rel(D) and err <= mr["norm_bound"]
    assert np.array_equal(g["quadrant_i"] * G + g["quadrant_j"], gp["cell"])
    assert np.array_equal(g["max_per_quad"], gp["max_per_quad"]) and np.array_equal(g["per_quad"], gp["per_quad"])
    assert float(g["height"]) == gp["height"]
    assert np.array_equal(g["kept"], gp["kept"]) and np.array_equal(np.flatnonzero(g["keep"]), gp["kept"])
    # the kept set from the reference's own fp32 norm too
    assert np.array_equal(F.gpf_select(xyz0, g["norm_feat_dist"], int(g["num_bb"]), G, factor)["kept"], g["kept"])


def test_tie_rules():
    f0, f1, _ = F.desc_case(3, 40, 30, 8)
    f1[7] = f1[2]   # duplicate target rows: the lower index first, the other second
    f0[0] = f1[2]
    f0[5] = f0[1]   # duplicate source rows: rev takes the lower
    nn = F.nn2(f0, f1)
    assert nn["nn1"][0] == 2 and nn["nn2"][0] == 7
    j = nn["nn1"][1]
    assert nn["nn1"][5] == j and (nn["rev"][j] != 5)
    near = f1.copy()
    near[9] = f1[4] + np.float32(1e-7)  # a near-tie that is no duplicate
    f0[3] = f1[4]
    assert F.nn2(f0, near)["margin"] <= 1.0
    # equal norms inside a truncated cell: the lower row wins
    xyz = np.zeros((6, 3), np.float32)
    xyz[:, 0] = [0, 0, 0, 0, 0, 1]
    r = F.gpf_select(xyz, np.array([0.5, 0.2, 0.2, 0.2, 0.9, 0.1]), 3, 1, 1.0)
    assert r["max_per_quad"].tolist() == [[6]] and r["per_quad"].tolist() == [[2.0]] and r["kept"].tolist() == [1, 5]


def test_max_equals_min():
    f1 = np.eye(4, dtype=np.float32)
    f0 = f1.copy()
    mr = F.match_ratio(f0, f1, np.arange(4), (np.arange(4) + 1) % 4, np.arange(4))
    assert np.array_equal(mr["norm"], -np.ones(4)) and mr["num_bb"] == 4


@pytest.mark.parametrize("counts,total,want,height", [
    # height 4.5 exactly (sum 9 == TOTAL at the first step): half to even gives 4, not 5
    ([10, 10], 9.0, [4, 4], 4.5),
    # 5.5 -> 6 (even)
    ([10, 10], 11.0, [6, 6], 5.5),
    ([3, 0, 5], 0.0, [0, 0, 0], 0.0),           # TOTAL = 0: nothing
    # TOTAL >= N0: 8 -> 12 -> 14 -> 15, |16 - 14| = 2 ends the loop; every cell is a dwarf
    ([3, 5], 16.0, [3, 5], 15.0),
    # 10 -> 15 -> 17.5 -> 18.75 -> 19.375 (|20 - 18.75| <= 2); rint 19
    ([1, 100], 20.0, [1, 19], 19.375),
])
def test_waterfill_by_hand(counts, total, want, height):
    pq, h = F.waterfill(np.array(counts), total)
    assert pq.tolist() == [float(v) for v in want] and h == height


def test_refit_and_composition():
    xyz0, xyz1, f0, f1, T = F.planted_registration(0, N=120)
    out = F.fr(xyz0, xyz1, f0, f1, T, "GPF", 512)
    assert out["num_pairs_init"] == 120 and 4 <= out["num_pairs_filtered"] <= 120
    assert out["inlier_ratio_filtered"] > out["inlier_ratio_init"] > 0.2
    assert np.abs(out["T"] - T).max() < 1e-2
    pose, n, inl = F.refit_inliers(np.eye(4), xyz0, xyz1, 1e-3)
    assert n < 3 and np.array_equal(pose, np.eye(4))
    with pytest.raises(AssertionError):
        F.fr(xyz0, xyz1, f0, f1, T, "DFR", 16)


def test_abi_lists_f7():
    from pointdsc_amd import _lib
    for name in ("pdsc_nn2_workspace_bytes", "pdsc_nn2", "pdsc_nn2_split", "pdsc_match_ratio", "pdsc_gpf_select_workspace_bytes",
                 "pdsc_gpf_select", "pdsc_refit_inliers"):
        assert name in _lib.EXPORTS, name
