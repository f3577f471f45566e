#!/usr/bin/env python3
"""Wall time per call of the multiway stages (pointdsc_amd.multiway, include/pdsc.h
f11 / f12): information_matrix on keypoint pairs of 1000 x 1500 and 5000 x 7500
points at max_distance 0.07, and global_optimization (pose_graph_optimize: both
passes, pruning included) on known-answer graphs of 33 and 60 nodes with about
n^2 / 4 edges.

Every step runs in a child process of its own under its own time limit; the
first step that fails ends the run.  Times are host wall clock around calls
that end in the call's own stream synchronise: the median over --calls after
--warmup.

    python tools/bench_multiway.py [--calls 30] [--warmup 3] [--step-timeout 180]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEPS = ["info:1000", "info:5000", "graph:33", "graph:60"]


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), out


def child(step, calls, warmup):
    import numpy as np
    import torch
    import icp_reference as R
    import posegraph_reference as P
    from pointdsc_amd import multiway as M
    dev = torch.device("cuda:0")
    kind, n = step.split(":")
    n = int(n)
    if kind == "info":
        src, tgt, init, _ = R.make_case(0, n, n + n // 2)
        s, t, T = (torch.from_numpy(x).to(dev) for x in (src, tgt, init))
        med, best, (info, n_corr) = timed(lambda: M.information_matrix(s, t, M.ICP_DISTANCE, T), calls, warmup)
        print(json.dumps(dict(step=step, Ns=n, Nt=n + n // 2, max_distance=M.ICP_DISTANCE, ms_median=round(med, 4),
                              ms_min=round(best, 4), n_corr=n_corr)))
    else:
        E = n * n // 4
        loops = (E - (n - 1)) * 3 // 5
        g = P.make_graph(1, n, loops, E - (n - 1) - loops, cloud=60)
        a = [torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) for k in ("init", "src", "tgt", "trans", "info", "unc")]
        med, best, (poses, conf, keep, res) = timed(lambda: M.pose_graph_optimize(*a, M.ICP_DISTANCE), calls, warmup)
        unc = g["unc"].astype(bool)
        print(json.dumps(dict(step=step, n=n, E=len(g["src"]), ms_median=round(med, 4), ms_min=round(best, 4),
                              iterations=list(res.iterations), objective=list(res.objective),
                              edges_kept=res.edges_kept, solver_failed=res.solver_failed,
                              false_edges_dropped=bool(np.array_equal(keep.cpu().numpy().astype(bool)[unc],
                                                                      ~g["false"][unc])),
                              gap_to_ground_truth=P.pose_gap(poses.cpu().numpy(), g["gt"]))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=180.0)
    ap.add_argument("--steps", default="", help="instead of the default list: info:N,graph:N,...")
    ap.add_argument("--child", metavar="STEP", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.calls, a.warmup)
        return 0
    for step in (a.steps.split(",") if a.steps else STEPS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--calls", str(a.calls), "--warmup",
               str(a.warmup)]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"step {step}: time limit of {a.step_timeout:g} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {step}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
