"""The reference's baselines on the GPU: SM, RANSAC, PMC, GCRANSAC.

``SM(corr, src_keypts, tgt_keypts, ...)`` mirrors
baseline_scripts/baseline_3DMatch.py:19-53 -- same inputs (``corr`` is the
loader's ``corr_pos`` [1,N,6]), same outputs ``(pred_trans [1,4,4],
pred_labels [1,N])`` -- with ``args.inlier_threshold`` passed as a keyword.
Runs on pointdsc_amd/csrc/sm.hip through the C ABI (pdsc_spectral_matching):
dense M built once, 10 matrix-vector power iterates (HBM/MALL-bound), top-10 %
selection and the weighted Kabsch of a9.  No CPU fallback.
"""
from __future__ import annotations

import torch

from ._call import call
from .kernels import _dev


def SM(corr, src_keypts, tgt_keypts, inlier_threshold: float = 0.10, top_ratio: float = 0.1,
       num_iterations: int = 10, return_eig: bool = False):
    corr, src, tgt = _dev(corr, "corr"), _dev(src_keypts, "src_keypts"), _dev(tgt_keypts, "tgt_keypts")
    assert corr.shape[0] == 1, "SM: bs = 1 (baseline_3DMatch.py:48)"
    N = corr.shape[1]
    if corr.shape != (1, N, 6) or src.shape != (1, N, 3) or tgt.shape != (1, N, 3):
        raise ValueError(f"shapes {tuple(corr.shape)} {tuple(src.shape)} {tuple(tgt.shape)}")
    dev = corr.device
    trans = torch.empty((1, 4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty((1, N), dtype=torch.float32, device=dev)
    eig = torch.empty((1, N), dtype=torch.float32, device=dev)
    call("pdsc_spectral_matching", corr, src, tgt, N, float(inlier_threshold), float(top_ratio), int(num_iterations),
         trans, labels, eig, device=dev, ws=("pdsc_spectral_matching_workspace_bytes", N))
    return (trans, labels, eig) if return_eig else (trans, labels)


def RANSAC(corr, src_keypts, tgt_keypts, inlier_threshold: float = 0.10, max_iteration: int = 1000, seed: int = 0):
    """baseline_scripts/baseline_3DMatch.py:80-98: RANSAC with ransac_n = 4 over
    every correspondence (``corr`` is accepted for the baselines' common
    signature and not read, as there), ``args.inlier_threshold`` and
    ``args.max_iteration`` passed as keywords.  Same outputs as ``SM``:
    ``(pred_trans [1,4,4], pred_labels [1,N])``.  Runs on
    pointdsc_amd/csrc/ransac.hip (pdsc_ransac_correspondence); ``seed`` fixes the
    draws.  No CPU fallback."""
    from .ransac import registration_ransac_based_on_correspondence
    src, tgt = _dev(src_keypts, "src_keypts"), _dev(tgt_keypts, "tgt_keypts")
    assert src.shape[0] == 1, "RANSAC: bs = 1 (baseline_3DMatch.py:81-82)"
    N = src.shape[1]
    if src.shape != (1, N, 3) or tgt.shape != (1, N, 3):
        raise ValueError(f"shapes {tuple(src.shape)} {tuple(tgt.shape)}")
    res = registration_ransac_based_on_correspondence(src[0], tgt[0], None, inlier_threshold, ransac_n=4,
                                                      max_iteration=max_iteration, seed=seed)
    return res.transformation_f32[None], res.labels[None]


def PMC(corr, src_keypts, tgt_keypts, inlier_threshold: float = 0.10, mode: str = "squared", node_budget: int = 0,
        return_info: bool = False):
    """baseline_scripts/baseline_3DMatch.py:56-77: the graph of length-consistent
    correspondence pairs over ``corr`` (the loader's ``corr_pos`` [1,N,6]), its
    maximum clique as the inlier set and one Kabsch over it.  Same outputs as
    ``SM``: ``(pred_trans [1,4,4], pred_labels [1,N])``; ``return_info=True``
    appends the search's ``CliqueInfo`` (size, exact, heuristic_size,
    roots_incomplete, nodes; reading it synchronises).  mode 'squared' is the
    reference as written (squared lengths against ``inlier_threshold``),
    'length' compares the lengths.  Runs on pointdsc_amd/csrc/clique.hip
    (pdsc_consistency_graph, pdsc_max_clique) where the reference calls a
    prebuilt x86 libpmc.so; ``node_budget`` bounds each root's search (0: the
    library default).  No CPU fallback."""
    from .kernels import CliqueInfo, consistency_graph, max_clique, rigid_transform_3d
    corr, src, tgt = _dev(corr, "corr"), _dev(src_keypts, "src_keypts"), _dev(tgt_keypts, "tgt_keypts")
    assert corr.shape[0] == 1, "PMC: bs = 1 (baseline_3DMatch.py:73)"
    N = corr.shape[1]
    if corr.shape != (1, N, 6) or src.shape != (1, N, 3) or tgt.shape != (1, N, 3):
        raise ValueError(f"shapes {tuple(corr.shape)} {tuple(src.shape)} {tuple(tgt.shape)}")
    adj, _ = consistency_graph(corr[0], inlier_threshold, mode)
    _, labels, result = max_clique(adj, node_budget)
    pred_labels = labels[None]
    pred_trans = rigid_transform_3d(src, tgt, pred_labels)
    return (pred_trans, pred_labels, CliqueInfo(result)) if return_info else (pred_trans, pred_labels)


def GCRANSAC(corr, src_keypts, tgt_keypts, inlier_threshold: float = 0.10, max_iteration: int = 1000, seed: int = 0):
    """baseline_scripts/baseline_3DMatch.py:101-123: GC-RANSAC over every
    correspondence (``corr`` is accepted for the baselines' common signature and
    not read, as there) with spatial_coherence_weight 0.1 and conf 0.99999999,
    ``args.inlier_threshold`` and ``args.max_iteration`` passed as keywords.  Same
    outputs as ``SM``: ``(pred_trans [1,4,4], pred_labels [1,N])``; an empty mask
    gives the identity.  Runs on pointdsc_amd/csrc/gc_ransac.hip (pdsc_gc_ransac,
    include/pdsc.h f10: the algorithm restated, parity with pygcransac itself is
    unpinned; its SPRT pre-emption is left out); ``seed`` fixes the draws.  No CPU
    fallback."""
    from .gc_ransac import gc_ransac
    src, tgt = _dev(src_keypts, "src_keypts"), _dev(tgt_keypts, "tgt_keypts")
    assert src.shape[0] == 1, "GCRANSAC: bs = 1 (baseline_3DMatch.py:104-105)"
    N = src.shape[1]
    if src.shape != (1, N, 3) or tgt.shape != (1, N, 3):
        raise ValueError(f"shapes {tuple(src.shape)} {tuple(tgt.shape)}")
    res = gc_ransac(src[0], tgt[0], inlier_threshold, 0.1, max_iteration, 0.99999999, seed)
    pred_trans = res.transformation_f32[None]
    if res.n_inliers == 0:
        pred_trans = torch.eye(4, dtype=torch.float32, device=src.device)[None]
    return pred_trans, res.labels[None]


def sm_compat(corr, inlier_threshold: float = 0.10, out=None):
    """SM's dense M [N,N] over corr [N,6] (baseline_3DMatch.py:20-36), by the
    launch ``SM`` makes.  ``out``: a contiguous fp32 [N,N] device tensor to write
    into (a view of a larger buffer lets a test put a guard row behind M)."""
    corr = _dev(corr, "corr")
    N = corr.shape[0]
    if corr.shape != (N, 6):
        raise ValueError(f"shape {tuple(corr.shape)}")
    if out is None:
        out = torch.empty((N, N), dtype=torch.float32, device=corr.device)
    elif not (out.device == corr.device and out.dtype == torch.float32 and out.shape == (N, N)
              and out.is_contiguous()):
        raise ValueError("out: a contiguous fp32 [N,N] tensor on corr's device")
    call("pdsc_sm_compat", corr, N, float(inlier_threshold), out, device=corr.device)
    return out


def sm_matvec(M, v):
    """y = M v (one SM power-iteration product; M [N,N], v [N])."""
    M, v = _dev(M, "M"), _dev(v, "v")
    N = v.shape[0]
    y = torch.empty(N, dtype=torch.float32, device=v.device)
    call("pdsc_sm_matvec", M, v, N, y, device=v.device)
    return y
