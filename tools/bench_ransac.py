#!/usr/bin/env python3
"""Wall time per RANSAC call (pointdsc_amd.ransac, include/pdsc.h f6) for the
reference drivers' three configurations -- the baseline (ransac_n 4, 1000
iterations), the PointDSC solver (ransac_n 3, 5000) and the fork's competitor
(ransac_n 4, 500000 iterations, edge_similarity 0.9; once with confidence
0.9999 and once without early stop) -- on synthetic pairs
(pointdsc_amd/synthetic.py) of 1000 and 5000 correspondences at 30 % and 6 %
inliers.

Every configuration runs in a child process of its own under its own time limit;
the first that fails ends the run.  Times are host wall clock around calls that
end in one synchronise (the result's read-back), after warm-up.  Next to the time:
iterations, n_validated and the scored (hypothesis x point) pairs per second.
Each pair costs about 15 fp64 FMA-class operations; the fp64 vector peak to hold
that against is half the 157.3 TFLOPS fp32 vector peak, 78.6 TFLOPS = 39.3e12
FMA/s = 2.6e12 pairs/s (MI355X datasheet).

    python tools/bench_ransac.py [--calls 20] [--warmup 3] [--step-timeout 120]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> ransac_n, max_iteration, edge_similarity, confidence
CONFIGS = {
    "baseline": (4, 1000, 0.0, 1.0),
    "solver": (3, 5000, 0.0, 1.0),
    "fr_conf": (4, 500000, 0.9, 0.9999),
    "fr_full": (4, 500000, 0.9, 1.0),
}
PEAK_PAIRS = 78.6e12 / 2 / 15


def child(cfg, n, ratio, calls, warmup):
    import torch
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    from pointdsc_amd.synthetic import synthetic_pair
    dev = torch.device("cuda:0")
    pair = synthetic_pair(n, seed=11, inlier_ratio=ratio)
    src = torch.from_numpy(pair["src_keypts"]).to(dev)
    tgt = torch.from_numpy(pair["tgt_keypts"]).to(dev)
    ns, it, es, conf = CONFIGS[cfg]
    kw = dict(ransac_n=ns, edge_similarity=es, max_iteration=it, confidence=conf, seed=0)
    for _ in range(warmup):
        res = ransac(src, tgt, None, 0.10, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        res = ransac(src, tgt, None, 0.10, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / calls * 1e3
    pairs = res.n_validated * n / (ms * 1e-3)
    print(json.dumps(dict(config=cfg, N=n, inlier_ratio=ratio, ransac_n=ns, max_iteration=it, edge_similarity=es,
                          confidence=conf, ms_per_call=round(ms, 4), iterations=res.iterations,
                          n_validated=res.n_validated, n_inliers=res.n_inliers,
                          pairs_per_s=float(f"{pairs:.4g}"), of_fp64_vector_peak=round(pairs / PEAK_PAIRS, 4))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--child", nargs=3, metavar=("CONFIG", "N", "RATIO"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), float(a.child[2]), a.calls, a.warmup)
        return 0
    for n in (1000, 5000):
        for ratio in (0.3, 0.06):
            for cfg in CONFIGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", cfg, str(n), str(ratio), "--calls",
                       str(a.calls), "--warmup", str(a.warmup)]
                what = f"step {cfg} N={n} inliers={ratio}"
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
