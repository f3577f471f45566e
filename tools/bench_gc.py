#!/usr/bin/env python3
"""Wall time of GC-RANSAC (pointdsc_amd.gc_ransac, include/pdsc.h f10) on synthetic
pairs (pointdsc_amd/synthetic.py) of 1000, 5000 and 20000 correspondences at 30 %
inliers and 500000 iterations, the fork's budget: the grid, one labelling and the
whole solve separately, the solve with the local optimisation on and off (with the
fork's confidence 0.999 and without an early stop), and f6's RANSAC (ransac_n 3,
no checker, the same confidence) on the same inputs beside them.

Every shape runs in a child process of its own under its own time limit; the
first that fails ends the run.  Times are host wall clock around calls that end in
one synchronise, after warm-up.

    python tools/bench_gc.py [--calls 10] [--warmup 2] [--step-timeout 180]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS, EPS, LAMBDA, CONF = 500000, 0.10, 0.1, 0.999


def timed(f, calls, warmup):
    import torch
    for _ in range(warmup):
        out = f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = f()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / calls * 1e3, 4), out


def child(n, ratio, calls, warmup):
    import torch
    from pointdsc_amd.gc_ransac import gc_grid, gc_label, gc_ransac
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    from pointdsc_amd.synthetic import synthetic_pair
    dev = torch.device("cuda:0")
    pair = synthetic_pair(n, seed=11, inlier_ratio=ratio)
    src = torch.from_numpy(pair["src_keypts"]).to(dev)
    tgt = torch.from_numpy(pair["tgt_keypts"]).to(dev)
    pose = torch.from_numpy(pair["gt_trans"]).to(dev).double().contiguous()
    row = dict(N=n, inlier_ratio=ratio, max_iteration=ITERATIONS)
    row["grid_ms"], grid = timed(lambda: gc_grid(src, tgt), calls, warmup)
    row["n_cells"] = int(grid[3].item())
    row["label_ms"], _ = timed(lambda: gc_label(pose, src, tgt, grid, EPS, LAMBDA), calls, warmup)
    one = gc_grid(src, tgt, 1)  # every row in one cell: the global-memory path of the labelling above 1024 rows
    row["label_one_cell_ms"], _ = timed(lambda: gc_label(pose, src, tgt, one, EPS, LAMBDA), calls, warmup)
    for conf, tag in ((CONF, "conf"), (1.0, "full")):
        for lo in (True, False):
            ms, res = timed(lambda: gc_ransac(src, tgt, EPS, LAMBDA, ITERATIONS, conf, 0, lo), calls, warmup)
            key = f"gc_{tag}_{'lo' if lo else 'nolo'}"
            row[key + "_ms"], row[key + "_iterations"], row[key + "_inliers"] = ms, res.iterations, res.n_inliers
            if lo:
                row[key + "_lo_runs"], row[key + "_lo_steps"] = res.lo_runs, res.lo_steps
        ms, res = timed(lambda: ransac(src, tgt, None, EPS, ransac_n=3, max_iteration=ITERATIONS, confidence=conf,
                                       seed=0), calls, warmup)
        row[f"f6_{tag}_ms"], row[f"f6_{tag}_iterations"], row[f"f6_{tag}_inliers"] = ms, res.iterations, res.n_inliers
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=float, default=180.0)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 5000, 20000])
    ap.add_argument("--child", nargs=2, metavar=("N", "RATIO"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), float(a.child[1]), a.calls, a.warmup)
        return 0
    for n in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "0.3", "--calls", str(a.calls),
               "--warmup", str(a.warmup)]
        what = f"step N={n}"
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"{what}: time limit of {a.step_timeout:g} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"{what}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
