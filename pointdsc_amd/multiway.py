"""Multiway registration on the GPU: what the multiway driver of
AmnonDrory/PointDSC runs through open3d around each forward
(multiway/test_multi_ate.py:54-83, 141-147, 166-174, 217-224, 31-51) -- the
information matrix of a fragment pair, multi-scale ICP, the pose graph and its
global optimisation with loop-closure pruning, and the absolute trajectory
error -- on the gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f11 and f12).
open3d is not needed; its algorithms are restated and the choices they leave
open are fixed in include/pdsc.h.

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import torch

from . import _lib
from ._call import call, read_struct, struct_buffer
from .descriptors import voxel_down_sample
from .icp import registration_icp
from .kernels import _dev, rigid_transform_3d

ICP_DISTANCE = 0.05 * 1.4  # test_multi_ate.py:60, :144, :167


def _trans(t, name, dev):
    """A [4,4] device tensor as contiguous fp64 (None stays None)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (there is no CPU fallback)")
    if t.dtype not in (torch.float32, torch.float64) or tuple(t.shape) != (4, 4):
        raise TypeError(f"{name} must be a [4,4] float32 / float64 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float64).contiguous()


def information_matrix(source: torch.Tensor, target: torch.Tensor, max_distance: float, trans=None,
                       want_correspondences: bool = False):
    """o3d get_information_matrix_from_point_clouds(source, target, max_distance,
    trans): (info fp64 [6,6] on the device, n_corr[, corr int32 [Ns]]).  source
    [Ns,3], target [Nt,3] fp32 device tensors; trans [4,4] device tensor (source ->
    target), None = identity."""
    source, target = _dev(source, "source"), _dev(target, "target")
    if source.dim() != 2 or source.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
        raise ValueError(f"source {tuple(source.shape)} / target {tuple(target.shape)} must be [n,3]")
    dev = source.device
    ns, nt = source.shape[0], target.shape[0]
    res = struct_buffer(_lib.PdscInformationResult, dev)
    corr = torch.empty(ns, dtype=torch.int32, device=dev) if want_correspondences else None
    call("pdsc_information_matrix", source, ns, target, nt, _trans(trans, "trans", dev), float(max_distance), res, corr,
         device=dev, ws=("pdsc_information_matrix_workspace_bytes", ns, nt))
    n_corr = read_struct(res, _lib.PdscInformationResult).n_corr
    info = res[:36 * 8].view(torch.float64).view(6, 6)
    return (info, n_corr, corr) if want_correspondences else (info, n_corr)


def loop_edge_ok(info: torch.Tensor, n_src: int, n_tgt: int, trans: torch.Tensor) -> bool:
    """test_multi_ate.py:147: a pair becomes a loop-closure edge unless its overlap
    info[5,5] / min(n_src, n_tgt) is under 0.30 or trans has the identity's trace."""
    return not (float(info[5, 5]) / min(int(n_src), int(n_tgt)) < 0.30 or float(torch.trace(trans)) == 4.0)


def multi_scale_icp(source: torch.Tensor, target: torch.Tensor, voxel_sizes, max_iters, init,
                    max_distance: float = ICP_DISTANCE):
    """test_multi_ate.py:54-73: per scale voxel_down_sample both clouds and run
    point-to-point ICP from the previous scale's result; the information matrix at
    the last scale, radius voxel_size * 1.4.  Returns (trans fp64 [4,4], info fp64
    [6,6]), both on the device."""
    if len(voxel_sizes) != len(max_iters) or not len(max_iters):
        raise ValueError("voxel_sizes and max_iters must have the same, non-zero length")
    source, target = _dev(source, "source"), _dev(target, "target")
    cur = _trans(init, "init", source.device)
    info = None
    for k, (vs, it) in enumerate(zip(voxel_sizes, max_iters)):
        s_down, t_down = voxel_down_sample(source, vs)[0], voxel_down_sample(target, vs)[0]
        cur = registration_icp(s_down, t_down, max_distance, cur, max_iteration=int(it)).transformation
        if k == len(max_iters) - 1:
            info = information_matrix(s_down, t_down, vs * 1.4, cur)[0]
    return cur, info


def local_refinement(source: torch.Tensor, target: torch.Tensor, init):
    """test_multi_ate.py:76-83: multi_scale_icp with the driver's constants."""
    return multi_scale_icp(source, target, [0.05, 0.05 / 2.0, 0.05 / 4.0], [50, 30, 14], init)


@dataclass
class PoseGraph:
    """o3d.registration.PoseGraph as tensors: ``nodes`` fp64 [n,4,4] (node frame ->
    world); per edge the source and target node, ``trans`` fp64 [E,4,4] (source
    node's frame -> target node's), ``info`` fp64 [E,6,6], ``uncertain``; after
    global_optimization also the line process ``confidence`` [E] of the edges kept."""
    device: torch.device
    nodes: torch.Tensor = None
    edge_src: torch.Tensor = None
    edge_tgt: torch.Tensor = None
    edge_trans: torch.Tensor = None
    edge_info: torch.Tensor = None
    edge_uncertain: torch.Tensor = None
    confidence: torch.Tensor = None
    result: object = field(default=None, repr=False)

    def __post_init__(self):
        d = self.device = torch.device(self.device)
        if d.type != "cuda":
            raise RuntimeError("PoseGraph lives on the device (there is no CPU fallback)")
        if self.nodes is None:
            self.nodes = torch.empty((0, 4, 4), dtype=torch.float64, device=d)
            self.edge_src = torch.empty(0, dtype=torch.int32, device=d)
            self.edge_tgt = torch.empty(0, dtype=torch.int32, device=d)
            self.edge_trans = torch.empty((0, 4, 4), dtype=torch.float64, device=d)
            self.edge_info = torch.empty((0, 6, 6), dtype=torch.float64, device=d)
            self.edge_uncertain = torch.empty(0, dtype=torch.int32, device=d)

    @property
    def n_nodes(self) -> int:
        return self.nodes.shape[0]

    @property
    def n_edges(self) -> int:
        return self.edge_src.shape[0]

    def add_node(self, pose: torch.Tensor) -> int:
        self.nodes = torch.cat([self.nodes, _trans(pose, "pose", self.device)[None]])
        return self.n_nodes - 1

    def add_edge(self, source: int, target: int, trans: torch.Tensor, info: torch.Tensor, uncertain: bool) -> int:
        if not isinstance(info, torch.Tensor) or not info.is_cuda or tuple(info.shape) != (6, 6):
            raise TypeError("info must be a [6,6] device tensor")
        ids = torch.tensor([int(source), int(target), int(bool(uncertain))], dtype=torch.int32, device=self.device)
        self.edge_src = torch.cat([self.edge_src, ids[0:1]])
        self.edge_tgt = torch.cat([self.edge_tgt, ids[1:2]])
        self.edge_uncertain = torch.cat([self.edge_uncertain, ids[2:3]])
        self.edge_trans = torch.cat([self.edge_trans, _trans(trans, "trans", self.device)[None]])
        self.edge_info = torch.cat([self.edge_info, info.to(device=self.device, dtype=torch.float64)[None]])
        return self.n_edges - 1


def pose_graph_optimize(nodes, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain,
                        max_correspondence_distance: float, edge_prune_threshold: float = 0.25,
                        preference_loop_closure: float = 20.0, reference_node: int = 0, criteria=None):
    """pdsc_pose_graph_optimize on tensors: (poses fp64 [n,4,4] (a copy), confidence
    fp64 [E], edge_keep int32 [E], PdscPoseGraphResult)."""
    poses = _dev(nodes, "nodes", torch.float64).clone()
    dev = poses.device
    n, E = poses.shape[0], edge_src.shape[0]
    es, et = _dev(edge_src, "edge_src", torch.int32), _dev(edge_tgt, "edge_tgt", torch.int32)
    tr, inf = _dev(edge_trans, "edge_trans", torch.float64), _dev(edge_info, "edge_info", torch.float64)
    unc = _dev(edge_uncertain, "edge_uncertain", torch.int32)
    if tuple(poses.shape[1:]) != (4, 4) or tuple(tr.shape) != (E, 4, 4) or tuple(inf.shape) != (E, 6, 6) \
            or et.shape[0] != E or unc.shape[0] != E:
        raise ValueError("nodes [n,4,4], edge_src / edge_tgt / edge_uncertain [E], edge_trans [E,4,4], edge_info [E,6,6]")
    opt = _lib.PdscPoseGraphOptions(float(max_correspondence_distance), float(edge_prune_threshold),
                                    float(preference_loop_closure), int(reference_node), 0)
    conf = torch.ones(max(E, 1), dtype=torch.float64, device=dev)
    keep = torch.ones(max(E, 1), dtype=torch.int32, device=dev)
    res = struct_buffer(_lib.PdscPoseGraphResult, dev)
    call("pdsc_pose_graph_optimize", poses, n, es, et, tr, inf, unc, E, ctypes.byref(opt),
         ctypes.byref(criteria) if criteria is not None else None, conf, keep, res, device=dev,
         ws=("pdsc_pose_graph_workspace_bytes", n, E))
    return poses, conf[:E], keep[:E], read_struct(res, _lib.PdscPoseGraphResult)


def pose_graph_linearize(nodes, edge_src, edge_tgt, edge_trans, edge_info, edge_uncertain, line_process=None,
                         mu: float = 0.0, reference_node: int = 0):
    """pdsc_pose_graph_linearize: (e fp64 [E,6], F, H fp64 [6n,6n], b fp64 [6n]) at
    `nodes` under the line process (None: 1)."""
    poses = _dev(nodes, "nodes", torch.float64)
    dev = poses.device
    n, E = poses.shape[0], edge_src.shape[0]
    lp = _dev(line_process, "line_process", torch.float64) if line_process is not None else None
    e = torch.empty((max(E, 1), 6), dtype=torch.float64, device=dev)
    F = torch.empty(1, dtype=torch.float64, device=dev)
    H = torch.empty((6 * n, 6 * n), dtype=torch.float64, device=dev)
    b = torch.empty(6 * n, dtype=torch.float64, device=dev)
    call("pdsc_pose_graph_linearize", poses, n, _dev(edge_src, "edge_src", torch.int32),
         _dev(edge_tgt, "edge_tgt", torch.int32), _dev(edge_trans, "edge_trans", torch.float64),
         _dev(edge_info, "edge_info", torch.float64), _dev(edge_uncertain, "edge_uncertain", torch.int32), E, lp,
         float(mu), int(reference_node), e, F, H, b, device=dev, ws=("pdsc_pose_graph_workspace_bytes", n, E))
    return e[:E], float(F.item()), H, b


def global_optimization(graph: PoseGraph, max_correspondence_distance: float = ICP_DISTANCE,
                        edge_prune_threshold: float = 0.25, preference_loop_closure: float = 20.0,
                        reference_node: int = 0, criteria=None) -> PoseGraph:
    """o3d global_optimization(graph, GlobalOptimizationLevenbergMarquardt(),
    GlobalOptimizationConvergenceCriteria(), GlobalOptimizationOption(...)): the
    optimised graph with the pruned edges removed (a new PoseGraph; open3d edits
    its argument).  Its ``result`` is the call's PdscPoseGraphResult."""
    poses, conf, keep, res = pose_graph_optimize(graph.nodes, graph.edge_src, graph.edge_tgt, graph.edge_trans,
                                                 graph.edge_info, graph.edge_uncertain, max_correspondence_distance,
                                                 edge_prune_threshold, preference_loop_closure, reference_node,
                                                 criteria)
    if res.solver_failed:
        raise RuntimeError("pose-graph optimisation: the Cholesky factorisation met a pivot that is not positive")
    k = keep.bool()
    return PoseGraph(graph.device, poses, graph.edge_src[k], graph.edge_tgt[k], graph.edge_trans[k],
                     graph.edge_info[k], graph.edge_uncertain[k], conf[k], res)


def absolute_trajectory_error(gt_poses: torch.Tensor, est_poses: torch.Tensor):
    """test_multi_ate.py:31-51, 268-287: align the ground-truth positions onto the
    estimated ones (rigid_transform_3d, fp32 as the driver) and return (the RMSE of
    the remaining distances in cm, the per-node distances in cm [n])."""
    if not gt_poses.is_cuda or not est_poses.is_cuda:
        raise RuntimeError("poses must be device tensors (there is no CPU fallback)")
    model = gt_poses[:, :3, 3].float().contiguous()[None]
    data = est_poses[:, :3, 3].float().contiguous()[None]
    T = rigid_transform_3d(model, data)[0]
    err = torch.linalg.norm(model[0] @ T[:3, :3].T + T[:3, 3] - data[0], dim=-1) * 100.0
    return float(torch.sqrt(torch.mean(err ** 2))), err
