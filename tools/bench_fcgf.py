#!/usr/bin/env python
"""Time FCGF (pointdsc_amd.fcgf) on the MI355X: hipEvent medians of the
quantisation and of the forward (coordinate levels + kernel maps + network: one
ABI call), the voxel counts per level, and the achieved gather bandwidth and MFMA
rate of the forward against the MI355X figures of SURVEY.md section 8(d).

    python tools/bench_fcgf.py [--steps 20] [--warmup 3]

Inputs: tests/golden/demo_data/cloud_bin_0.ply at voxel 0.05 (conv1_kernel_size
7) and a synthetic ring-structured LiDAR-like sweep of about 120k points at voxel
0.3 (conv1_kernel_size 5).  Work is counted from the kernel maps (one gathered
input row and one C_in x C_out product per present neighbour), so the rates are
useful work over the whole forward's time, map building included.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_S, MFMA_F32_FLOPS = 8.0e12, 157.3e12  # HBM3E peak, fp32 matrix peak


def lidar_sweep(n_rings=64, per_ring=1900, seed=0):
    """Rings of constant elevation over a ground plane with a few box obstacles."""
    rs = np.random.RandomState(seed)
    az = np.tile(np.linspace(0, 2 * np.pi, per_ring, endpoint=False), n_rings)
    el = np.repeat(np.radians(np.linspace(-24.8, 2.0, n_rings)), per_ring)
    r = np.minimum(np.where(el < -0.01, 1.73 / np.maximum(np.sin(-el), 1e-3), 80.0), 80.0)
    r = np.minimum(r, 8.0 + 30.0 * (0.5 + 0.5 * np.sin(3 * az) * np.cos(5 * az)) + 40.0 * (np.sin(7 * az) > 0.6))
    r = r + rs.normal(0, 0.02, r.shape)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(np.float32)


def pairs(out_c, in_c, step, sign=1):
    """Present (output, offset) pairs of a 3^3 map: out reads in at out + sign o step."""
    def key(c):
        c = c.astype(np.int64)
        return ((c[:, 0] * (1 << 21) + c[:, 1] + (1 << 20)) * (1 << 21) + c[:, 2] + (1 << 20)) * (1 << 21) + c[:, 3] + (1 << 20)
    sk = np.sort(key(in_c))
    n = 0
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                q = key(out_c + sign * step * np.array([0, ox, oy, oz]))
                p = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
                n += int((sk[p] == q).sum())
    return n


def work(levels):
    """(gathered bytes, flops) of the MFMA layers from the maps of `levels` (coords per level)."""
    C, T = [32, 64, 128, 256], [64, 64, 128]
    same = [pairs(c, c, 1 << l) for l, c in enumerate(levels)]
    down = [pairs(levels[l + 1], levels[l], 1 << l) for l in range(3)]
    layers = [(same[0], 32, 32)] * 2 + [(same[0], 64, 64)] * 2 + [(len(levels[0]), 96, 64), (len(levels[0]), 64, 32)]
    for l in range(3):
        layers += [(down[l], C[l], C[l + 1]), (down[l], (C[l + 1] + (T[l + 1] if l < 2 else 0)), T[l])]  # conv, conv_tr
        layers += [(same[l + 1], C[l + 1], C[l + 1])] * 2
        if l < 2:
            layers += [(same[l + 1], T[l + 1], T[l + 1])] * 2
    return sum(4 * p * ci for p, ci, _ in layers), sum(2 * p * ci * co for p, ci, co in layers)


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from pointdsc_amd.descriptors import read_ply
    from pointdsc_amd.fcgf import FCGF, fcgf_state_dict, quantize
    dev = torch.device("cuda")
    for name, pts, voxel, ks in (("cloud_bin_0", read_ply(os.path.join(ROOT, "tests/golden/demo_data/cloud_bin_0.ply")), 0.05, 7),
                                 ("lidar_sweep", lidar_sweep(), 0.3, 5)):
        model = FCGF(conv1_kernel_size=ks)
        model.load_state_dict(fcgf_state_dict(0, ks, 32))
        model = model.to(dev).eval()
        xyz = torch.from_numpy(pts).to(dev)
        inds, coords = quantize(xyz, voxel)
        feats = torch.ones((len(inds), 1), device=dev)
        _, taps = model(coords, feats, debug=True)
        levels = [coords.cpu().numpy()] + [taps[k].cpu().numpy() for k in ("coords2", "coords4", "coords8")]
        t_q = median_ms(lambda: quantize(xyz, voxel), a.steps, a.warmup)
        t_f = median_ms(lambda: model(coords, feats), a.steps, a.warmup)
        gbytes, flops = work(levels)
        print(json.dumps({"input": name, "points": len(pts), "voxel": voxel, "conv1_kernel_size": ks,
                          "voxels_per_level": [len(c) for c in levels], "quantize_ms": round(t_q, 3),
                          "forward_ms": round(t_f, 3), "gather_GB_s": round(gbytes / t_f / 1e6, 1),
                          "gather_of_hbm_peak": round(gbytes / (t_f * 1e-3) / HBM_BYTES_S, 4),
                          "mfma_TFLOP_s": round(flops / t_f / 1e9, 2),
                          "mfma_of_f32_peak": round(flops / (t_f * 1e-3) / MFMA_F32_FLOPS, 4)}))


if __name__ == "__main__":
    main()
