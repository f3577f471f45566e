"""The fork's ``--algo TEASER`` (algorithms/TEASER_plus_plus.py:101-126 of
AmnonDrory/PointDSC) on the GPU: second nearest neighbours, the Grid-Prioritized
Filter in its best-buddies-first form, and TEASER++ on the matched points --
consistency graph, maximum clique, GNC-TLS rotation, TLS translation
(include/pdsc.h f7, f8, f9).  From descriptors to pose nothing leaves the device
but the filter's pair count.

The reference calls the x86 library teaserpp_python; here the algorithm is the
one restated in include/pdsc.h (parity with that library is unpinned).

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from time import time

import torch

from . import matching
from .kernels import _dev, teaser_solve

VOXEL_SIZE = 0.3          # TEASER_plus_plus.py:13, the solver's noise bound
MAX_PAIRS = 8192          # pdsc_teaser_solve's limit (one wavefront holds a graph row)
# ``mode == "FAIL_TOLERANT"``: the reference runs the solver in a subprocess and kills it after 10 s
# (TEASER_plus_plus.py:16-59).  Here the clique search's per-root node budget is the bound: a quarter of the
# library default (0 = pdsc_max_clique_default_budget(), 4096), so a search that does not finish gives up
# four times sooner and still returns the best clique found (clique_exact = 0) and its pose.
FAIL_TOLERANT_BUDGET = 1024


def _check_pairs(n: int):
    if n > MAX_PAIRS:
        raise ValueError(f"{n} pairs after the filter exceed the solver's {MAX_PAIRS}: lower args.GPF_max_matches")


def TEASER(A, B, A_feats, B_feats, args):
    """TEASER_plus_plus.py:101-126.  A [N0,3], B [N1,3], A_feats [N0,D], B_feats
    [N1,D] fp32 device tensors (A stands in for A_pcd and A_tensor, B for B_pcd);
    args carries ``GPF_grid_wid``, ``GPF_max_matches`` and ``mode``.  Returns (T,
    elapsed_time): T a device fp64 [4,4] (the identity when the clique has fewer
    than two members), elapsed_time as the reference adds it up (the additional
    time of the second neighbours plus the solver's)."""
    xyz0, xyz1 = _dev(A, "A"), _dev(B, "B")
    f0, f1 = _dev(A_feats, "A_feats"), _dev(B_feats, "B_feats")
    dev = xyz0.device
    idx0, idx1, idx2, t_2nd, rev = matching._find_2nn(f0, f1)
    idx0, idx1 = matching.Grid_Prioritized_Filter(f0, f1, idx0, idx1, idx2, xyz0, args, BB_first=True, _rev=rev)[:2]
    _check_pairs(idx0.shape[0])
    torch.cuda.synchronize(dev)
    start = time()
    if idx0.shape[0] == 0:
        T = torch.eye(4, dtype=torch.float64, device=dev)
    else:
        budget = FAIL_TOLERANT_BUDGET if getattr(args, "mode", None) == "FAIL_TOLERANT" else 0
        T = teaser_solve(xyz0[idx0], xyz1[idx1], VOXEL_SIZE, node_budget=budget)[0]
    torch.cuda.synchronize(dev)
    return T, t_2nd + (time() - start)
