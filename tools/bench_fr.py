#!/usr/bin/env python3
"""Stage times of the filtered-RANSAC front end (include/pdsc.h f7,
pointdsc_amd/matching.py, pointdsc_amd/fr.py): nn2, match_ratio, gpf_select,
RANSAC on the kept pairs (ransac_n 4, confidence 0.9999, up to --iters
hypotheses) and refit_inliers, each between two hipEvents on the stream
(median over --calls after --warmup), and FR end to end (host wall clock, it
reads counts back), on synthetic unit-norm descriptors (40 % true matches) at
N0 = N1 in {5000, 20000}, D = 32.

The nn2 time is also given as a fraction of the fp32 vector roofline: 2 N0 N1 D
FLOP against 157.3 TFLOPS (MI355X datasheet).

Every shape runs in a child process of its own under its own time limit; the
first that fails ends the run.

    python tools/bench_fr.py [--calls 20] [--warmup 3] [--iters 100000] [--step-timeout 180]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_FP32_VECTOR = 157.3e12


def child(n, calls, warmup, iters):
    import numpy as np
    import torch
    import fr_reference as F
    from pointdsc_amd import matching as M
    from pointdsc_amd.fr import FR
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    dev = torch.device("cuda:0")
    xyz0, xyz1, f0, f1, T = F.planted_registration(1, N=n)
    xyz0, xyz1, f0, f1 = (torch.from_numpy(x).to(dev) for x in (xyz0, xyz1, f0, f1))
    state = {}

    def s_nn2():
        state["nn"] = M.nn2(f0, f1)

    def s_ratio():
        state["mr"] = M.match_ratio(f0, f1, *state["nn"])

    def s_gpf():
        state["kept"] = M.gpf_select(xyz0, state["mr"][2], state["mr"][3], 10, 1.0)[0].long()

    def s_ransac():
        k = state["kept"]
        state["res"] = ransac(xyz0, xyz1, torch.stack([k, state["nn"][0].long()[k]], 1), 0.6, ransac_n=4,
                              max_iteration=iters, confidence=0.9999, seed=0)

    def s_refit():
        M.refit_inliers(state["res"].transformation, xyz0, xyz1[state["nn"][0].long()], 0.6)

    out = dict(N0=n, N1=n, D=32, iters=iters)
    for name, fn in (("nn2", s_nn2), ("ratio", s_ratio), ("gpf", s_gpf), ("ransac", s_ransac), ("refit", s_refit)):
        ms = []
        for i in range(warmup + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        out[name + "_ms"] = round(float(np.median(ms)), 4)
    out["nn2_of_fp32_vector_peak"] = round(2.0 * n * n * 32 / (out["nn2_ms"] * 1e-3) / PEAK_FP32_VECTOR, 4)
    out["kept"], out["ransac_iterations"] = int(state["kept"].numel()), state["res"].iterations
    args = types.SimpleNamespace(mode="GPF", algo="RANSAC", iters=iters, ELC=False, GPF_grid_wid=10, GPF_factor=1.0)
    for _ in range(warmup):
        FR(xyz0, xyz1, f0, f1, args, T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        FR(xyz0, xyz1, f0, f1, args, T)
    torch.cuda.synchronize()
    out["fr_gpf_end_to_end_ms"] = round((time.perf_counter() - t0) / calls * 1e3, 4)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100000)
    ap.add_argument("--step-timeout", type=float, default=180.0)
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.calls, a.warmup, a.iters)
        return 0
    for n in (5000, 20000):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--calls", str(a.calls), "--warmup",
               str(a.warmup), "--iters", str(a.iters)]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"step N={n}: time limit of {a.step_timeout:g} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step N={n}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
