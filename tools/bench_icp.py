#!/usr/bin/env python3
"""Wall time per ICP call (pointdsc_amd.icp.registration_icp, include/pdsc.h f5)
for keypoint pairs of 1000 and 5000 points at max_distance 0.1 (icp_refine) and
0.6 (test.py:185-189), and for the voxel-downsampled demo pair, on both paths:
the one-workgroup launch and the launch-per-step path (PDSC_ICP_ONE_WG=0).

Every (shape, path) step runs in a child process of its own under its own time
limit; the first step that fails ends the run.  Times are host wall clock around
calls that end in the call's own stream synchronise, after warm-up.

    python tools/bench_icp.py [--calls 50] [--warmup 5] [--step-timeout 120]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# kp512: the largest size of the one-workgroup path (above it both settings take the multi-launch path)
SHAPES = [("kp512", 0.1), ("kp512", 0.6), ("kp1000", 0.1), ("kp1000", 0.6), ("kp5000", 0.1), ("kp5000", 0.6),
          ("demo", 0.1)]


def make_pair(shape, dev):
    import numpy as np
    import torch
    import icp_reference as R
    if shape == "demo":
        from pointdsc_amd.descriptors import read_ply, voxel_down_sample
        raw = torch.from_numpy(read_ply(os.path.join(ROOT, "tests", "golden", "demo_data", "cloud_bin_0.ply")))
        src = voxel_down_sample(raw.to(dev), 0.05)[0].cpu().numpy()
        true = R.rigid([0.2, 1.0, -0.4], 30.0, [0.4, -0.3, 0.2])
        tgt = R.transform(true, src).astype(np.float32)[np.random.RandomState(21).permutation(len(src))]
        init = R.rigid([1.0, 0.3, 0.5], 1.0, [0.012, -0.012, 0.011]) @ true
    else:
        n = int(shape[2:])
        src, tgt, init, _ = R.make_case(0, n, n + n // 2)
    return (torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), torch.from_numpy(init).to(dev))


def child(shape, r, calls, warmup):
    import torch
    from pointdsc_amd.icp import registration_icp
    dev = torch.device("cuda:0")
    src, tgt, init = make_pair(shape, dev)
    for _ in range(warmup):
        res = registration_icp(src, tgt, r, init)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        res = registration_icp(src, tgt, r, init)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / calls * 1e3
    print(json.dumps(dict(shape=shape, Ns=int(src.shape[0]), Nt=int(tgt.shape[0]), max_distance=r,
                          one_wg=os.environ.get("PDSC_ICP_ONE_WG", "1") != "0", ms_per_call=round(ms, 4),
                          iterations=res.iterations, n_corr=res.n_corr, fitness=res.fitness,
                          inlier_rmse=res.inlier_rmse)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--shapes", default="", help="instead of the default list: kpN:R,... (e.g. kp512:0.1,kp512:0.6)")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "R"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], float(a.child[1]), a.calls, a.warmup)
        return 0
    shapes = [(x.split(":")[0], float(x.split(":")[1])) for x in a.shapes.split(",")] if a.shapes else SHAPES
    for shape, r in shapes:
        for knob in ("1", "0"):
            env = dict(os.environ, PDSC_ICP_ONE_WG=knob)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, str(r), "--calls", str(a.calls),
                   "--warmup", str(a.warmup)]
            try:
                p = subprocess.run(cmd, env=env, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
            except subprocess.TimeoutExpired:
                print(f"step {shape} r={r} PDSC_ICP_ONE_WG={knob}: time limit of {a.step_timeout:g} s; stopping",
                      file=sys.stderr)
                return 124
            if p.returncode != 0:
                print(f"step {shape} r={r} PDSC_ICP_ONE_WG={knob}: exit status {p.returncode}; stopping", file=sys.stderr)
                return p.returncode if p.returncode > 0 else 1
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
