"""RANSAC on correspondences on the GPU: the ``RANSAC`` baseline
(baseline_scripts/baseline_3DMatch.py:80-98), the ``--solver RANSAC`` option of
the PointDSC drivers (evaluation/test_3DMatch.py:59-77, test.py:137-155) and the
fork's RANSAC competitors (algorithms/FR.py:122-150) of AmnonDrory/PointDSC, on
the gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f6).  open3d is not needed:
its ``registration_ransac_based_on_correspondence`` is restated and the choices
it leaves open are fixed (a counter-based sampler, the order among equal
hypotheses, the confidence stop at round granularity: include/pdsc.h), so two
calls with the same ``seed`` are bitwise equal.

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._call import _p, call, read_struct, struct_buffer, trans_view
from .kernels import _dev


@dataclass
class RansacResult:
    """open3d's RegistrationResult for the winning hypothesis: ``transformation``
    fp64 [4,4] (device; the refit over its inliers with ``refit=True``), its fp32
    copy, ``fitness`` = n_inliers / N, ``inlier_rmse``, ``correspondence_set``
    (the inlier rows of ``corres`` [n_inliers,2], as open3d returns them) and
    ``labels`` [N] 0/1 over the rows of ``corres``; ``iterations`` hypotheses were
    drawn, ``n_validated`` of them passed sampling and the checker, ``best`` is
    the winner's index (-1: none valid).  ``debug``: dict of per-hypothesis
    ``samples`` [H,n], ``count`` [H], ``sumsq`` [H], ``trans`` [H,4,4] on request."""
    transformation: torch.Tensor
    transformation_f32: torch.Tensor
    fitness: float
    inlier_rmse: float
    correspondence_set: torch.Tensor
    labels: torch.Tensor
    n_inliers: int
    iterations: int
    best: int
    n_validated: int
    debug: dict | None = None


def ransac_round() -> int:
    """Hypotheses per round (the granularity of the confidence stop)."""
    return int(_lib.load().pdsc_ransac_round())


def registration_ransac_based_on_correspondence(source: torch.Tensor, target: torch.Tensor, corres=None,
                                                max_correspondence_distance: float = 0.1, ransac_n: int = 3,
                                                edge_similarity: float = 0.0, max_iteration: int = 1000,
                                                confidence: float = 1.0, seed: int = 0, refit: bool = False,
                                                debug: bool = False) -> RansacResult:
    """o3d registration_ransac_based_on_correspondence(source, target, corres,
    max_correspondence_distance, TransformationEstimationPointToPoint(False),
    ransac_n, [CorrespondenceCheckerBasedOnEdgeLength(edge_similarity)],
    RANSACConvergenceCriteria(max_iteration, confidence)) on the current torch
    stream.  source [Ns,3], target [Nt,3] fp32 device tensors; corres [M,2]
    integer device tensor of (source row, target row), None = row i with row i."""
    source, target = _dev(source, "source"), _dev(target, "target")
    if source.dim() != 2 or source.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
        raise ValueError(f"source {tuple(source.shape)} / target {tuple(target.shape)} must be [n,3]")
    dev = source.device
    if corres is None:
        if source.shape[0] != target.shape[0]:
            raise ValueError("corres=None pairs row i with row i: source and target need the same length")
        corres = torch.arange(source.shape[0], device=dev, dtype=torch.int64)[:, None].expand(-1, 2)
        src, tgt = source, target
    else:
        if not isinstance(corres, torch.Tensor) or not corres.is_cuda:
            raise RuntimeError("corres must be a device tensor (there is no CPU fallback)")
        if corres.dim() != 2 or corres.shape[1] != 2 or corres.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"corres must be an [M,2] int32 / int64 tensor, got {corres.dtype} {tuple(corres.shape)}")
        idx = corres.to(torch.int64)
        src, tgt = source[idx[:, 0]].contiguous(), target[idx[:, 1]].contiguous()
    n, H, ns = src.shape[0], int(max_iteration), int(ransac_n)
    res = struct_buffer(_lib.PdscRansacResult, dev)
    t32 = torch.empty((4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty(n, dtype=torch.float32, device=dev)
    dbg = dstruct = None
    if debug and H >= 1 and ns in (3, 4):
        dbg = dict(samples=torch.zeros((H, ns), dtype=torch.int32, device=dev),
                   count=torch.zeros(H, dtype=torch.int32, device=dev),
                   sumsq=torch.zeros(H, dtype=torch.float64, device=dev),
                   trans=torch.zeros((H, 4, 4), dtype=torch.float64, device=dev))
        dstruct = _lib.PdscRansacDebug(*(_p(dbg[k]) for k in ("samples", "count", "sumsq", "trans")))
    call("pdsc_ransac_correspondence", src, tgt, n, float(max_correspondence_distance), ns, float(edge_similarity), H,
         float(confidence), int(seed) & (2 ** 64 - 1), 1 if refit else 0, t32, labels, res, dstruct, device=dev,
         ws=("pdsc_ransac_workspace_bytes", n))
    r = read_struct(res, _lib.PdscRansacResult)
    return RansacResult(trans_view(res), t32, r.fitness, r.inlier_rmse, corres[labels > 0], labels, r.n_inliers,
                        r.iterations, r.best, r.n_validated, dbg)


def ransac_solver(src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, pred_labels: torch.Tensor,
                  inlier_threshold: float, max_iteration: int = 5000, seed: int = 0):
    """evaluation/test_3DMatch.py:59-77 (``--solver RANSAC``, PointDSC as a
    pre-filter): RANSAC with ransac_n = 3 over the correspondences with
    ``pred_labels > 0``.  src_keypts / tgt_keypts [1,N,3], pred_labels [1,N] ->
    (pred_trans [1,4,4] float, pred_labels [1,N] 0/1).  With fewer than 3
    predicted inliers: the identity and zeros."""
    src, tgt = _dev(src_keypts, "src_keypts"), _dev(tgt_keypts, "tgt_keypts")
    assert src.shape[0] == 1 and pred_labels.shape[0] == 1, "ransac_solver: bs = 1 (test_3DMatch.py:61-64)"
    dev = src.device
    out_labels = torch.zeros_like(pred_labels, dtype=torch.float32, device=dev)
    pred_trans = torch.eye(4, dtype=torch.float32, device=dev)[None]
    pred_inliers = torch.nonzero(pred_labels[0].to(dev) > 0)[:, 0]
    if pred_inliers.numel() < 3:
        return pred_trans, out_labels
    corres = torch.stack([pred_inliers, pred_inliers], 1)
    res = registration_ransac_based_on_correspondence(src[0], tgt[0], corres, inlier_threshold, ransac_n=3,
                                                      max_iteration=max_iteration, seed=seed)
    out_labels[0, res.correspondence_set[:, 0]] = 1
    pred_trans[0] = res.transformation_f32
    return pred_trans, out_labels
