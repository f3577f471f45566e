"""Fragment making on the GPU: step 1 of the multiway experiment of
AmnonDrory/PointDSC (multiway/make_fragments.py) -- RGB-D odometry between
adjacent frames, the fragment's pose graph and its optimisation, integration of
every frame into a sparse TSDF volume, and the surface points of that volume --
on the gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f13 and f14).  open3d is
not needed; its algorithms are restated and the choices they leave open are fixed
in include/pdsc.h.

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._call import call, query
from .kernels import _dev
from .multiway import PoseGraph, global_optimization

# multiway/initialize_config.py
DEFAULT_CONFIG = {"n_frames_per_fragment": 100, "max_depth": 3.0, "max_depth_diff": 0.07, "tsdf_cubic_size": 3.0,
                  "preference_loop_closure_odometry": 0.1, "depth_scale": 1000.0, "sdf_trunc": 0.04,
                  "max_blocks": 32768}
ODOMETRY_ITERATIONS = (20, 10, 5)  # open3d's OdometryOption, coarsest level first
BLOCK = 16
BLOCK_VOXELS = BLOCK ** 3


def _intrinsic(intrinsic):
    """(fx, fy, cx, cy) from a 4-sequence or a [3,3] matrix."""
    if isinstance(intrinsic, torch.Tensor):
        intrinsic = intrinsic.detach().cpu().tolist()
    k = list(intrinsic)
    if len(k) == 3:
        k = [k[0][0], k[1][1], k[0][2], k[1][2]]
    if len(k) != 4:
        raise ValueError("intrinsic must be (fx, fy, cx, cy) or a [3,3] matrix")
    return tuple(float(v) for v in k)


def rgbd_from_color_and_depth(color: torch.Tensor, depth: torch.Tensor, depth_scale: float = 1000.0,
                              depth_trunc: float = 3.0):
    """o3d create_from_color_and_depth(convert_rgb_to_intensity=True) for F frames:
    color uint8 [F,H,W,3], depth uint16 (or int16 bits) [F,H,W] -> (intensity fp32
    [F,H,W], depth fp32 [F,H,W] in metres, 0 above depth_trunc)."""
    color = _dev(color, "color", torch.uint8)
    if depth.dtype not in (torch.uint16, torch.int16):
        raise TypeError(f"depth must be uint16 (or its bits as int16), got {depth.dtype}")
    depth = _dev(depth, "depth", depth.dtype)
    if color.dim() != 4 or color.shape[3] != 3 or tuple(depth.shape) != tuple(color.shape[:3]):
        raise ValueError(f"color {tuple(color.shape)} must be [F,H,W,3] and depth {tuple(depth.shape)} [F,H,W]")
    F, H, W = depth.shape
    inten = torch.empty((F, H, W), dtype=torch.float32, device=color.device)
    dep = torch.empty((F, H, W), dtype=torch.float32, device=color.device)
    call("pdsc_rgbd_from_color_and_depth", color, depth, F, H, W, float(depth_scale), float(depth_trunc), inten, dep,
         device=color.device)
    return inten, dep


def _odometry_args(intensity, depth, intrinsic, pairs, max_depth_diff, min_depth, max_depth, iterations):
    intensity, depth = _dev(intensity, "intensity"), _dev(depth, "depth")
    if intensity.dim() != 3 or tuple(intensity.shape) != tuple(depth.shape):
        raise ValueError(f"intensity {tuple(intensity.shape)} and depth {tuple(depth.shape)} must both be [F,H,W]")
    pairs = [(int(s), int(t)) for s, t in (pairs.tolist() if isinstance(pairs, torch.Tensor) else pairs)]
    P = len(pairs)
    src = (ctypes.c_int32 * max(P, 1))(*[p[0] for p in pairs])
    tgt = (ctypes.c_int32 * max(P, 1))(*[p[1] for p in pairs])
    if len(iterations) != 3:
        raise ValueError("iterations: three counts, coarsest level first")
    opt = _lib.PdscRgbdOdometryOptions(float(max_depth_diff), float(min_depth), float(max_depth),
                                       (ctypes.c_int32 * 3)(*[int(i) for i in iterations]), 0)
    return intensity, depth, _intrinsic(intrinsic), src, tgt, P, opt


def _init(init, P, dev):
    if init is None:
        return None
    init = _dev(init, "init", torch.float64)
    if tuple(init.shape) != (P, 4, 4):
        raise ValueError(f"init must be [P,4,4] = [{P},4,4], got {tuple(init.shape)}")
    return init


def rgbd_odometry(intensity, depth, intrinsic, pairs, init=None, max_depth_diff: float = 0.07, min_depth: float = 0.0,
                  max_depth: float = 4.0, iterations=ODOMETRY_ITERATIONS, want_status: bool = False):
    """o3d compute_rgbd_odometry(.., RGBDOdometryJacobianFromHybridTerm(), option)
    for every (source, target) frame pair of `pairs` in one call: (trans fp64
    [P,4,4] source frame -> target frame, info fp64 [P,6,6], success bool [P]) on
    the device[, status int32 [P,4] = (success, n_corr_last, iterations_run, 0)].
    intensity, depth: fp32 [F,H,W] device tensors (depth in metres, 0 invalid)."""
    intensity, depth, k, src, tgt, P, opt = _odometry_args(intensity, depth, intrinsic, pairs, max_depth_diff,
                                                           min_depth, max_depth, iterations)
    dev = intensity.device
    F, H, W = intensity.shape
    trans = torch.empty((max(P, 1), 4, 4), dtype=torch.float64, device=dev)
    info = torch.empty((max(P, 1), 6, 6), dtype=torch.float64, device=dev)
    status = torch.zeros((max(P, 1), 4), dtype=torch.int32, device=dev)
    call("pdsc_rgbd_odometry", intensity, depth, F, H, W, *k, src, tgt, P, _init(init, P, dev), ctypes.byref(opt), trans,
         info, status, device=dev, ws=("pdsc_rgbd_odometry_workspace_bytes", F, H, W, P))
    out = (trans, info, status[:, 0] != 0)
    return out + (status,) if want_status else out


def rgbd_odometry_linearize(intensity, depth, intrinsic, pairs, trans=None, level: int = 0,
                            max_depth_diff: float = 0.07, min_depth: float = 0.0, max_depth: float = 4.0):
    """One linearisation at pyramid `level` under `trans` (pdsc_rgbd_odometry_linearize):
    (corr int32 [P, H_l W_l] target pixel -> source pixel or -1, JtJ fp64 [P,6,6],
    Jtr fp64 [P,6], count [P], scales fp64 [P,2] = (a_s, a_t))."""
    intensity, depth, k, src, tgt, P, opt = _odometry_args(intensity, depth, intrinsic, pairs, max_depth_diff,
                                                           min_depth, max_depth, ODOMETRY_ITERATIONS)
    dev = intensity.device
    F, H, W = intensity.shape
    corr = torch.empty((max(P, 1), (H >> level) * (W >> level)), dtype=torch.int32, device=dev)
    sums = torch.empty((max(P, 1), 28), dtype=torch.float64, device=dev)
    scales = torch.empty((max(P, 1), 2), dtype=torch.float64, device=dev)
    call("pdsc_rgbd_odometry_linearize", intensity, depth, F, H, W, *k, src, tgt, P, _init(trans, P, dev),
         ctypes.byref(opt), int(level), corr, sums, scales, device=dev,
         ws=("pdsc_rgbd_odometry_workspace_bytes", F, H, W, P))
    iu = torch.triu_indices(6, 6, device=dev)
    JtJ = torch.zeros((P, 6, 6), dtype=torch.float64, device=dev)
    JtJ[:, iu[0], iu[1]] = sums[:, :21]
    JtJ[:, iu[1], iu[0]] = sums[:, :21]
    return corr, JtJ, sums[:, 21:27], sums[:, 27].round().long(), scales


def rgbd_odometry_pyramid(intensity, depth, level: int = 0, min_depth: float = 0.0, max_depth: float = 4.0):
    """Pyramid `level` of all F frames as rgbd_odometry builds it (pdsc_rgbd_odometry_pyramid:
    step 1 alone): a dict of the six fp32 [F, H_l, W_l] images I, D, Idx, Idy, Ddx, Ddy."""
    intensity, depth = _dev(intensity, "intensity"), _dev(depth, "depth")
    if intensity.dim() != 3 or tuple(intensity.shape) != tuple(depth.shape):
        raise ValueError(f"intensity {tuple(intensity.shape)} and depth {tuple(depth.shape)} must both be [F,H,W]")
    dev = intensity.device
    F, H, W = intensity.shape
    level = int(level)
    shape = (F, H >> level, W >> level) if 0 <= level < 3 else (F, 1, 1)  # a bad level is the entry's error
    out = {k: torch.empty(shape, dtype=torch.float32, device=dev) for k in ("I", "D", "Idx", "Idy", "Ddx", "Ddy")}
    call("pdsc_rgbd_odometry_pyramid", intensity, depth, F, H, W, float(min_depth), float(max_depth), level,
         *out.values(), device=dev, ws=("pdsc_rgbd_odometry_workspace_bytes", F, H, W, 1))
    return out


class TSDFVolume:
    """o3d.integration.ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) on the
    device (include/pdsc.h f14): at most `max_blocks` blocks of 16^3 voxels, 80 KB
    each, in one device buffer this object owns."""

    def __init__(self, voxel_length: float, sdf_trunc: float, max_blocks: int, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume lives on the device (there is no CPU fallback)")
        if not (voxel_length > 0 and sdf_trunc > 0):
            raise ValueError("voxel_length and sdf_trunc must be > 0")
        self.voxel_length, self.sdf_trunc, self.max_blocks = float(voxel_length), float(sdf_trunc), int(max_blocks)
        nbytes = query("pdsc_tsdf_workspace_bytes", self.max_blocks, required=False)
        if nbytes == 0:
            raise ValueError(f"max_blocks={max_blocks} is not supported (need 1 .. 2^17)")
        self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._ws = (self._state, nbytes)
        self.reset()

    def reset(self):
        call("pdsc_tsdf_reset", self.max_blocks, device=self.device, ws=self._ws)

    @property
    def n_blocks(self) -> int:
        return int(self._state[:4].view(torch.int32).item())

    def integrate(self, depth: torch.Tensor, colour: torch.Tensor, intrinsic, extrinsic: torch.Tensor):
        """o3d volume.integrate(rgbd, intrinsic, extrinsic): depth fp32 [H,W] metres,
        colour uint8 [H,W,3], extrinsic [4,4] world -> camera (a device tensor).
        Raises RuntimeError when the volume is full; that frame changes no voxel."""
        depth, colour = _dev(depth, "depth"), _dev(colour, "colour", torch.uint8)
        if depth.dim() != 2 or tuple(colour.shape) != tuple(depth.shape) + (3,):
            raise ValueError(f"depth {tuple(depth.shape)} must be [H,W] and colour {tuple(colour.shape)} [H,W,3]")
        if not isinstance(extrinsic, torch.Tensor) or not extrinsic.is_cuda or tuple(extrinsic.shape) != (4, 4):
            raise RuntimeError("extrinsic must be a [4,4] device tensor (there is no CPU fallback)")
        ext = extrinsic.to(torch.float64).contiguous()
        H, W = depth.shape
        call("pdsc_tsdf_integrate", depth, colour, H, W, *_intrinsic(intrinsic), ext, self.voxel_length, self.sdf_trunc,
             self.max_blocks, device=self.device, ws=self._ws)

    def extract_surface_points(self):
        """The vertices and vertex colours of o3d extract_triangle_mesh, in (block
        key, voxel index, axis) order: (points fp64 [n,3], colours fp64 [n,3])."""
        n = ctypes.c_int64(0)
        call("pdsc_tsdf_count_surface_points", self.max_blocks, ctypes.byref(n), device=self.device, ws=self._ws)
        points = torch.empty((n.value, 3), dtype=torch.float64, device=self.device)
        colours = torch.empty((n.value, 3), dtype=torch.float64, device=self.device)
        if n.value == 0:
            return points, colours
        call("pdsc_tsdf_emit_surface_points", self.voxel_length, self.max_blocks, points, colours, n.value,
             device=self.device, ws=self._ws)
        return points, colours

    def blocks(self):
        """(coords int32 [n,3], tsdf fp32 [n,4096], weight fp32 [n,4096], colour fp32
        [n,4096,3]) in ascending block-key order; voxel index x + 16 y + 256 z."""
        n = self.n_blocks
        d = self.device
        coords = torch.empty((n, 3), dtype=torch.int32, device=d)
        tsdf = torch.empty((n, BLOCK_VOXELS), dtype=torch.float32, device=d)
        weight = torch.empty((n, BLOCK_VOXELS), dtype=torch.float32, device=d)
        colour = torch.empty((n, BLOCK_VOXELS, 3), dtype=torch.float32, device=d)
        call("pdsc_tsdf_read_blocks", self.max_blocks, n, coords, tsdf, weight, colour, device=d, ws=self._ws)
        c = coords.long() + (1 << 20)
        order = torch.argsort((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2])
        return coords[order], tsdf[order], weight[order], colour[order]

    def write_blocks(self, coords, tsdf, weight, colour):
        """Insert the blocks `coords` int32 [n,3] (if absent) and overwrite their voxels."""
        coords = _dev(coords, "coords", torch.int32)
        n = coords.shape[0]
        tsdf, weight, colour = _dev(tsdf, "tsdf"), _dev(weight, "weight"), _dev(colour, "colour")
        if tuple(tsdf.shape) != (n, BLOCK_VOXELS) or tuple(weight.shape) != (n, BLOCK_VOXELS) \
                or tuple(colour.shape) != (n, BLOCK_VOXELS, 3):
            raise ValueError("coords [n,3], tsdf / weight [n,4096], colour [n,4096,3]")
        call("pdsc_tsdf_write_blocks", coords, n, tsdf, weight, colour, self.max_blocks, device=self.device, ws=self._ws)


def _aff_mul(A, B):
    """A B for rigid [4,4] fp64 arrays, every entry ((a0 b0 + a1 b1) + a2 b2) (+ a3): f12's product order."""
    C = np.eye(4)
    C[:3] = (A[:3, 0:1] * B[0] + A[:3, 1:2] * B[1]) + A[:3, 2:3] * B[2]
    C[:3, 3] += A[:3, 3]
    return C


def _aff_inv(T):
    """(R^T, -R^T t) in f12's product order."""
    inv = np.eye(4)
    Rt = T[:3, :3].T
    inv[:3, :3] = Rt
    inv[:3, 3] = -((Rt[:, 0] * T[0, 3] + Rt[:, 1] * T[1, 3]) + Rt[:, 2] * T[2, 3])
    return inv


def odometry_chain(trans):
    """make_fragments.py:69-92 on the host in fp64: trans [F-1,4,4] (frame k-1 -> frame
    k) -> node poses [F,4,4], node 0 the identity, node k = inv(T_k .. T_1).  The prefix
    product is 16 (F - 1) multiply-adds: no device work."""
    odo = np.eye(4)
    nodes = [np.eye(4)]
    for T in np.asarray(trans, dtype=np.float64):
        odo = _aff_mul(T, odo)
        nodes.append(_aff_inv(odo))
    return np.stack(nodes)


def make_fragment(colors: torch.Tensor, depths: torch.Tensor, intrinsic, config=None):
    """multiway/make_fragments.py for one fragment: colors uint8 [F,H,W,3], depths
    uint16 [F,H,W] (device tensors) -> (points fp64 [n,3], colours fp64 [n,3], the
    optimised PoseGraph).  Adjacent-pair odometry in one batched call; the chain
    graph of :69-92 (node k = inv(T_k .. T_1), edge (k - 1, k) with T_k and its
    information matrix, certain); global_optimization; every frame integrated with
    inv(node pose); the surface points."""
    cfg = dict(DEFAULT_CONFIG)
    cfg.update(config or {})
    inten, depth = rgbd_from_color_and_depth(colors, depths, cfg["depth_scale"], cfg["max_depth"])
    dev = inten.device
    F = inten.shape[0]
    eye = torch.eye(4, dtype=torch.float64, device=dev)
    graph = PoseGraph(dev)
    graph.add_node(eye)
    if F > 1:
        pairs = [(s, s + 1) for s in range(F - 1)]
        trans, info, _ = rgbd_odometry(inten, depth, intrinsic, pairs, max_depth_diff=cfg["max_depth_diff"])
        nodes = torch.from_numpy(odometry_chain(trans.cpu().numpy())).to(dev)  # the call has synchronised
        graph = PoseGraph(dev, nodes, torch.arange(0, F - 1, dtype=torch.int32, device=dev),
                          torch.arange(1, F, dtype=torch.int32, device=dev), trans.contiguous(), info.contiguous(),
                          torch.zeros(F - 1, dtype=torch.int32, device=dev))
        graph = global_optimization(graph, max_correspondence_distance=cfg["max_depth_diff"],
                                    preference_loop_closure=cfg["preference_loop_closure_odometry"])
    volume = TSDFVolume(cfg["tsdf_cubic_size"] / 512.0, cfg["sdf_trunc"], cfg["max_blocks"], dev)
    extrinsics = torch.from_numpy(np.stack([_aff_inv(T) for T in graph.nodes.cpu().numpy()])).to(dev)
    for i in range(F):
        volume.integrate(depth[i], colors[i], intrinsic, extrinsics[i])
    points, colours = volume.extract_surface_points()
    return points, colours, graph
