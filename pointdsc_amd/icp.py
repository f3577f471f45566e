"""ICP refinement of a predicted pose on the GPU: the "+ICP" stage the drivers
of AmnonDrory/PointDSC run through open3d on the forward's ``final_trans``
(test.py:183-189, evaluation/benchmark_utils.py:40-56), on the gfx950 kernels
of ``libpdsc.so`` (include/pdsc.h, f5).  open3d is not needed; its
point-to-point ``registration_icp`` is restated and the choices it leaves open
are fixed (nearest-neighbour ties, summation order: include/pdsc.h).

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib
from ._call import call, read_struct, struct_buffer, trans_view
from .kernels import _dev


@dataclass
class RegistrationResult:
    """open3d's RegistrationResult: ``transformation`` fp64 [4,4] (device),
    its fp32 copy, ``fitness`` = n_corr / Ns, ``inlier_rmse``, the number of
    updates applied, and (on request) the final evaluation's target index per
    source point, -1 where none is within max_distance."""
    transformation: torch.Tensor
    transformation_f32: torch.Tensor
    fitness: float
    inlier_rmse: float
    iterations: int
    n_corr: int
    correspondence: torch.Tensor | None = None


def registration_icp(source: torch.Tensor, target: torch.Tensor, max_distance: float, init=None,
                     max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
                     want_correspondences: bool = False) -> RegistrationResult:
    """o3d registration_icp(source, target, max_distance, init,
    TransformationEstimationPointToPoint(), ICPConvergenceCriteria(relative_fitness,
    relative_rmse, max_iteration)) on the current torch stream.  source [Ns,3],
    target [Nt,3] fp32 device tensors; init: [4,4] fp32 or fp64 device tensor
    (source -> target), None = identity."""
    source, target = _dev(source, "source"), _dev(target, "target")
    if source.dim() != 2 or source.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
        raise ValueError(f"source {tuple(source.shape)} / target {tuple(target.shape)} must be [n,3]")
    dev = source.device
    if init is not None:
        if not isinstance(init, torch.Tensor) or not init.is_cuda:
            raise RuntimeError("init must be a device tensor (there is no CPU fallback)")
        if init.dtype not in (torch.float32, torch.float64) or tuple(init.shape) != (4, 4):
            raise TypeError(f"init must be a [4,4] float32 / float64 tensor, got {init.dtype} {tuple(init.shape)}")
        init = init.to(torch.float64).contiguous()
    ns, nt = source.shape[0], target.shape[0]
    res = struct_buffer(_lib.PdscIcpResult, dev)
    t32 = torch.empty((4, 4), dtype=torch.float32, device=dev)
    corr = torch.empty(ns, dtype=torch.int32, device=dev) if want_correspondences else None
    call("pdsc_icp_point_to_point", source, ns, target, nt, init, float(max_distance), int(max_iteration),
         float(relative_fitness), float(relative_rmse), t32, res, corr, device=dev,
         ws=("pdsc_icp_workspace_bytes", ns, nt))
    r = read_struct(res, _lib.PdscIcpResult)
    return RegistrationResult(trans_view(res), t32, r.fitness, r.inlier_rmse, r.iterations, r.n_corr, corr)


def icp_refine(src_keypts: torch.Tensor, tgt_keypts: torch.Tensor, pred_trans: torch.Tensor,
               max_distance: float = 0.1) -> torch.Tensor:
    """evaluation/benchmark_utils.py:40-56: src_keypts [B,N,3], tgt_keypts [B,M,3],
    pred_trans [B,4,4] -> the refined [B,4,4] float on pred_trans.device (the
    reference takes B = 1; B > 1 refines pair by pair on the same stream)."""
    out = [registration_icp(src_keypts[b].detach().float(), tgt_keypts[b].detach().float(), max_distance,
                            pred_trans[b].detach()).transformation_f32 for b in range(pred_trans.shape[0])]
    return torch.stack(out).to(pred_trans.device)
