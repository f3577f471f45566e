#!/usr/bin/env python3
"""Golden data for the filtered-RANSAC front end (include/pdsc.h f7) from the
reference itself: runs find_nn, nn_to_mutual and Grid_Prioritized_Filter of the
reference's algorithms/matching.py (numpy + torch only, on the CPU) on the cases
of tests/fr_reference.py GOLDEN_CASES and records the inputs and every
intermediate into tests/golden/fr/<case>.npz.  The filter's local variables
(quadrants, max_per_quad, per_quad, the height, feat_dist, is_bb, keep) are read
from its frame when it returns.

A case is recorded only for a seed at which every decision is free of near-ties
by the fp64 margins of tests/fr_reference.py (each margin above twice the fp32
bound, derived there); the tool walks the seeds until one qualifies, and asserts
that the reference's own results equal the fp64 restatement's at that seed.

    python tools/gen_fr_goldens.py --reference /path/to/PointDSC-fork
"""
import argparse
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_gpf(M, f0, f1, i0, i1, i2, xyz0, args):
    """Grid_Prioritized_Filter's result and its locals at return."""
    seen = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "Grid_Prioritized_Filter":
            seen.update(frame.f_locals)

    sys.setprofile(prof)
    try:
        out = M.Grid_Prioritized_Filter(f0, f1, i0, i1, i2, xyz0, args)
    finally:
        sys.setprofile(None)
    return out, seen


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds algorithms/matching.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fr"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import torch
    import fr_reference as F
    from algorithms import matching as M
    warnings.filterwarnings("ignore")
    os.makedirs(a.out, exist_ok=True)
    for name, (N0, N1, D, G, factor) in F.GOLDEN_CASES.items():
        seed = F.tie_free_seed(N0, N1, D, G, factor)
        f0, f1, xyz0 = F.desc_case(seed, N0, N1, D)
        m_nn, m_cell, m_gpf, (nn, mr, g) = F.case_margins(f0, f1, xyz0, G, factor)
        t0, t1, tx = torch.from_numpy(f0), torch.from_numpy(f1), torch.from_numpy(xyz0)
        i0, i1, i2 = M.find_nn(t0, t1, return_2nd=True)
        mu0, mu1 = M.nn_to_mutual(t0, t1, i0, i1)
        args = types.SimpleNamespace(GPF_grid_wid=G, GPF_factor=factor)
        out, loc = run_gpf(M, t0, t1, i0, i1, i2, tx, args)
        is_bb = np.asarray(loc["is_bb"], bool)
        feat_dist = loc["feat_dist"].numpy()
        fd_t = loc["feat_dist"]
        norm = ((fd_t - fd_t.min()) / (fd_t.max() - fd_t.min())).numpy()  # normalize(), matching.py:122-125
        norm[is_bb] -= 1
        kept = out[0].numpy()
        assert np.array_equal(_bits(norm[kept]), _bits(out[6].numpy())), "norm_feat_dist is not the filter's"
        rec = dict(f0=f0, f1=f1, xyz0=xyz0, grid=np.int64(G), factor=np.float64(factor), seed=np.int64(seed),
                   nn1=i1.numpy(), nn2=i2.numpy(), mutual_idx0=mu0.numpy(), mutual_idx1=mu1.numpy(), is_bb=is_bb,
                   num_bb=np.int64(loc["num_bb"]), feat_dist=feat_dist, norm_feat_dist=norm,
                   quadrant_i=np.asarray(loc["quadrant_i"]), quadrant_j=np.asarray(loc["quadrant_j"]),
                   max_per_quad=np.asarray(loc["max_per_quad"]), per_quad=np.asarray(loc["per_quad"]),
                   height=np.float64(loc["curr_height"]), keep=np.asarray(loc["keep"], bool), kept=kept,
                   kept_norm=out[6].numpy(), margins=np.array([m_nn, m_cell, m_gpf]))
        # the reference agrees with the restatement at a tie-free seed
        assert np.array_equal(rec["nn1"], nn["nn1"]) and np.array_equal(rec["nn2"], nn["nn2"]), name
        assert np.array_equal(rec["mutual_idx0"], np.flatnonzero(mr["is_bb"])) and np.array_equal(is_bb, mr["is_bb"])
        assert np.array_equal(rec["quadrant_i"] * G + rec["quadrant_j"], g["cell"]), name
        assert np.array_equal(rec["max_per_quad"], g["max_per_quad"]) and np.array_equal(rec["per_quad"], g["per_quad"])
        assert np.array_equal(kept, g["kept"]), name
        np.savez_compressed(os.path.join(a.out, name + ".npz"), **rec)
        print(f"{name}: seed {seed}, margins nn {m_nn:.3g} cell {m_cell:.3g} gpf {m_gpf:.3g}, "
              f"num_bb {rec['num_bb']}, kept {len(kept)} of {N0}")


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


if __name__ == "__main__":
    main()
