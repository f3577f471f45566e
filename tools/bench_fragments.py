"""Times make_fragment and its three stages (odometry, pose graph, TSDF integration +
extraction) on a synthetic sequence with device events.

    python tools/bench_fragments.py [--frames 100] [--height 480] [--width 640] [--steps 3] [--warmup 1]

Prints one JSON line: per stage the median of `steps` timed runs in milliseconds, and
under "spread_ms" the [min, max] of the same runs."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pointdsc_amd import fragments as F  # noqa: E402
from pointdsc_amd.multiway import PoseGraph, global_optimization  # noqa: E402


# three textured planes n . p = d (a back wall, a floor, a side wall) seen from near the origin along +z
PLANES = [((0.1, 0.05, 1.0), 2.0), ((0.0, 1.0, 0.15), 0.9), ((1.0, 0.0, 0.2), 1.2)]


def render(pose, K, H, W):
    """(colour uint8 [H,W,3], depth uint16 [H,W] in mm) of the scene from camera `pose` (camera -> world)."""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rw = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ pose[:3, :3].T
    t = pose[:3, 3]
    best = np.full((H, W), np.inf)
    for n, d in PLANES:
        n = np.asarray(n) / np.linalg.norm(n)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (d - n @ t) / (rw @ n)
        best = np.minimum(best, np.where(s > 0, s, np.inf))
    depth = np.where(np.isfinite(best), best, 0.0)
    p = t + rw * depth[..., None]
    g = 0.5 + 0.1 * (np.sin(5 * p[..., 0] + 1) + np.sin(6 * p[..., 1] + 2 * p[..., 2]) + np.sin(4 * p[..., 2] - 3 * p[..., 0]))
    colour = np.clip(np.round(np.stack([g, 0.5 * g + 0.25, 1.0 - g], -1) * 255.0), 0, 255).astype(np.uint8)
    return colour, np.round(depth * 1000.0).astype(np.uint16)


def step_pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, t[0]],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, t[1]],
                     [-sy, cy * sx, cy * cx, t[2]], [0.0, 0.0, 0.0, 1.0]])


SPREAD = {}


def timed(fn, steps, warmup, name=None):
    out, ms = None, []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    if name:
        SPREAD[name] = [min(ms), max(ms)]
    return out, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, n = a.height, a.width, a.frames
    K = (0.875 * W, 0.875 * W, W / 2 - 0.5, H / 2 - 0.5)
    step = step_pose(0.0005, -0.0015, 0.0008, (0.002, -0.001, 0.0015))
    poses = [np.eye(4)]
    for _ in range(n - 1):
        poses.append(poses[-1] @ step)
    frames = [render(p, K, H, W) for p in poses]
    colors = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
    depth16 = torch.from_numpy(np.stack([f[1] for f in frames]).view(np.int16)).to(dev)
    cfg = dict(F.DEFAULT_CONFIG)

    (inten, depth), t_conv = timed(lambda: F.rgbd_from_color_and_depth(colors, depth16, 1000.0, cfg["max_depth"]),
                                   a.steps, a.warmup, "convert")
    pairs = [(s, s + 1) for s in range(n - 1)]
    (trans, info, ok), t_odo = timed(lambda: F.rgbd_odometry(inten, depth, K, pairs, max_depth_diff=cfg["max_depth_diff"]),
                                     a.steps, a.warmup, "odometry")
    nodes = torch.from_numpy(F.odometry_chain(trans.cpu().numpy())).to(dev)
    graph = PoseGraph(dev, nodes, torch.arange(0, n - 1, dtype=torch.int32, device=dev),
                      torch.arange(1, n, dtype=torch.int32, device=dev), trans.contiguous(), info.contiguous(),
                      torch.zeros(n - 1, dtype=torch.int32, device=dev))
    opt, t_pg = timed(lambda: global_optimization(graph, max_correspondence_distance=cfg["max_depth_diff"],
                                                  preference_loop_closure=0.1), a.steps, a.warmup, "pose_graph")
    ext = torch.linalg.inv(opt.nodes)

    def integrate():
        vol = F.TSDFVolume(cfg["tsdf_cubic_size"] / 512.0, cfg["sdf_trunc"], cfg["max_blocks"], dev)
        for i in range(n):
            vol.integrate(depth[i], colors[i], K, ext[i])
        return vol

    vol, t_int = timed(integrate, a.steps, a.warmup, "integrate")
    (pts, _), t_ext = timed(vol.extract_surface_points, a.steps, a.warmup, "extract")
    _, t_all = timed(lambda: F.make_fragment(colors, depth16, K, cfg), a.steps, a.warmup, "make_fragment")
    print(json.dumps({"frames": n, "height": H, "width": W, "convert_ms": t_conv, "odometry_ms": t_odo,
                      "pose_graph_ms": t_pg, "integrate_ms": t_int, "extract_ms": t_ext, "make_fragment_ms": t_all,
                      "odometry_success": int(ok.sum()), "blocks": vol.n_blocks, "points": int(pts.shape[0]), "spread_ms": SPREAD}))


if __name__ == "__main__":
    main()
