"""The fork's filtered "fast RANSAC" (algorithms/FR.py:16-119 of
AmnonDrory/PointDSC; test.py:163-170, ``--algo RANSAC --mode no_filter | MFR |
GPF``) on the GPU: second nearest neighbours, the filter, RANSAC on the
filtered pairs and one refit over the inliers among the unfiltered ones
(include/pdsc.h, f7 and f6).  ``--algo GC`` runs GC-RANSAC (f10,
pointdsc_amd/gc_ransac.py) on the filtered pairs in place of RANSAC and the
refit: it has its own final fit (FR.py:102).

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from time import time

import torch

from . import matching
from .gc_ransac import GC_RANSAC
from .kernels import _dev
from .ransac import registration_ransac_based_on_correspondence

VOXEL_SIZE = 0.3  # FR.py:18


def FR(A, B, A_feat, B_feat, args, T_gt, seed=0):
    """FR.py:16-119.  A [N0,3], B [N1,3], A_feat [N0,D], B_feat [N1,D] fp32 device
    tensors; args carries ``mode`` (``MFR``, ``GPF`` with ``GPF_grid_wid`` and
    ``GPF_factor``, ``no_filter``), ``algo`` (``RANSAC``, or ``GC`` with the options
    of ``gc_ransac.GC_RANSAC``: ``spatial_coherence_weight`` -- required; without it
    NotImplementedError, as the reference's default None fails inside pygcransac
    -- ``GC_conf``, ``GC_LO``, ``prosac``, ``use_edge_len``, ``use_sprt``), ``iters``
    (None: 500000) and ``ELC``;
    T_gt [4,4] only feeds the inlier ratios.  Returns the reference's 8-tuple (T,
    elapsed_time, pcd0, pcd1, num_pairs_init, inlier_ratio_init,
    num_pairs_filtered, inlier_ratio_filtered) with T a device fp64 [4,4] and the
    xyz tensors standing in for pcd0 / pcd1.  ``seed`` is the RANSAC sampler's: two
    calls with the same seed give the same T bit for bit.  If the filter leaves
    fewer than 4 pairs (RANSAC's sample size; 3 for GC) T is the identity.  B needs at least
    two rows (a second neighbour), A at most 262144 for ``GPF``."""
    if args.algo == "GC" and getattr(args, "spatial_coherence_weight", None) is None:
        raise NotImplementedError("algo == 'GC' needs args.spatial_coherence_weight (and GC_conf, GC_LO): it is not set")
    if args.algo not in ("RANSAC", "GC"):
        raise AssertionError("unexpected algo")
    if args.mode not in ("MFR", "GPF", "no_filter"):
        raise AssertionError("when running with algo==RANSAC, must define mode to MFR, GPF or no_filter")
    xyz0, xyz1 = _dev(A, "A"), _dev(B, "B")
    f0, f1 = _dev(A_feat, "A_feat"), _dev(B_feat, "B_feat")
    dev = xyz0.device

    # 1. coarse correspondences
    idx0, idx1, idx2, t_2nd, rev = matching._find_2nn(f0, f1)
    num_pairs_init = idx0.shape[0]
    inlier_ratio_init = matching.measure_inlier_ratio(idx0, idx1, xyz0, xyz1, T_gt, VOXEL_SIZE)

    # 2. filter
    torch.cuda.synchronize(dev)
    start = time()
    idx0_orig, idx1_orig = idx0, idx1
    if args.mode == "MFR":
        idx0, idx1, idx2 = matching.nn_to_mutual(f0, f1, idx0, idx1, idx2, force_return_2nd=True, _rev=rev)
    elif args.mode == "GPF":
        idx0, idx1, idx2 = matching.Grid_Prioritized_Filter(f0, f1, idx0, idx1, idx2, xyz0, args, _rev=rev)[:3]
    torch.cuda.synchronize(dev)
    filter_time = time() - start
    num_pairs_filtered = idx0.shape[0]
    inlier_ratio_filtered = matching.measure_inlier_ratio(idx0, idx1, xyz0, xyz1, T_gt, VOXEL_SIZE)

    # 3. GC-RANSAC (FR.py:70-87) or RANSAC (FR.py:122-150), 4. the refit over the unfiltered pairs (FR.py:101-114)
    start = time()
    iters = 500 * 10 ** 3 if args.iters is None else int(args.iters)
    if args.algo == "GC":  # FR.py:70-87; no step 4 (FR.py:102)
        if num_pairs_filtered < 3:
            T = torch.eye(4, dtype=torch.float64, device=dev)
        else:
            T = GC_RANSAC(xyz0[idx0].contiguous(), xyz1[idx1].contiguous(), 2 * VOXEL_SIZE, iters, args, None,
                          seed=seed)[0]
    elif num_pairs_filtered < 4:
        T = torch.eye(4, dtype=torch.float64, device=dev)
    else:
        kw = dict(edge_similarity=0.9, confidence=0.9995) if args.ELC else dict(confidence=0.9999)
        res = registration_ransac_based_on_correspondence(xyz0, xyz1, torch.stack([idx0, idx1], 1), 2 * VOXEL_SIZE,
                                                          ransac_n=4, max_iteration=iters, seed=seed, **kw)
        T = matching.refit_inliers(res.transformation, xyz0[idx0_orig], xyz1[idx1_orig], 2 * VOXEL_SIZE)[0]
    torch.cuda.synchronize(dev)
    algo_time = time() - start
    return (T, filter_time + algo_time + t_2nd, xyz0, xyz1, num_pairs_init, inlier_ratio_init, num_pairs_filtered,
            inlier_ratio_filtered)
