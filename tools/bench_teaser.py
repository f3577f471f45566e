#!/usr/bin/env python3
"""Wall time of TEASER++ on the GPU (include/pdsc.h f9) and of its stages on
synthetic pairs (pointdsc_amd/synthetic.py, 3dmatch preset, noise bound = the
preset's threshold) of 1000 and 5000 correspondences: the consistency graph, the
maximum clique, the GNC-TLS rotation on the clique's TIM chain, the TLS
translation, and the whole pdsc_teaser_solve.  Then the rotation loop alone at
K = 8192 on TIMs with 30 % outliers, once to convergence and once with a cost
threshold no pass can meet, so that it runs --loop-iterations passes: the time
per pass that bounds a launch of max_iterations = 10000.

Every row runs in a child process of its own under its own time limit; the
first that fails ends the run.  Times are medians of host wall clock around
single calls that end in one synchronise, after warm-up.

    python tools/bench_teaser.py [--calls 5] [--warmup 1] [--step-timeout 120] [--loop-iterations 2000]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pmc import median_ms  # noqa: E402


def child_pair(n, calls, warmup):
    import torch
    from pointdsc_amd import kernels as K
    from pointdsc_amd.synthetic import PRESETS, synthetic_pair
    dev = torch.device("cuda:0")
    tau = PRESETS["3dmatch"]["inlier_threshold"]
    pair = synthetic_pair(n, seed=11)
    src, tgt = (torch.from_numpy(pair[k]).to(dev) for k in ("src_keypts", "tgt_keypts"))
    corr = torch.cat([src, tgt], 1)
    graph_ms, (adj, _) = median_ms(lambda: K.consistency_graph(corr, 2 * tau, "length"), calls, warmup)
    clique_ms, (members, _, cres) = median_ms(lambda: K.max_clique(adj), calls, warmup)
    ci = K.CliqueInfo(cres)
    m = members[:ci.size].long()
    nxt = torch.roll(m, -1)
    a, b = (src[nxt] - src[m]).double(), (tgt[nxt] - tgt[m]).double()
    rot_ms, (R, _, _, info) = median_ms(lambda: K.gnc_tls_rotation(a, b, tau), calls, warmup)
    rotated = src[m].double() @ R.T
    tls_ms, _ = median_ms(lambda: K.tls_translation(rotated, tgt[m].double(), tau), calls, warmup)
    solve_ms, out = median_ms(lambda: K.teaser_solve(src, tgt, tau), calls, warmup)
    ti = K.TeaserInfo(out[3])
    err = float(np.abs(out[0].cpu().numpy() - pair["gt_trans"]).max())
    print(json.dumps(dict(case="synthetic_pair", N=n, graph_ms=graph_ms, max_clique_ms=clique_ms, rotation_ms=rot_ms,
                          translation_ms=tls_ms, teaser_solve_ms=solve_ms, clique_size=ti.clique_size,
                          clique_exact=ti.clique_exact, gnc_iterations=K.GncInfo(info).iterations,
                          n_translation_inliers=ti.n_translation_inliers, max_abs_pose_error=round(err, 6))))


def child_loop(k, iters, calls, warmup):
    import torch
    from pointdsc_amd import kernels as K
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(3)
    a = rng.randn(k, 3) * 3.0
    th = 0.7
    Rz = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    b = a @ Rz.T + 0.05 * rng.randn(k, 3)
    out = rng.permutation(k)[:int(0.3 * k)]
    b[out] = rng.randn(len(out), 3) * 3.0
    a, b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    conv_ms, o = median_ms(lambda: K.gnc_tls_rotation(a, b, 0.3), calls, warmup)
    n_conv = K.GncInfo(o[3]).iterations
    # cost_threshold -1: |cost - prev| < -1 never holds, the loop runs max_iterations passes (gnc_factor close to
    # 1 keeps mu finite over them)
    loop_ms, o = median_ms(lambda: K.gnc_tls_rotation(a, b, 0.3, gnc_factor=1.001, max_iterations=iters,
                                                      cost_threshold=-1.0), calls, warmup)
    n_loop = K.GncInfo(o[3]).iterations
    print(json.dumps(dict(case="rotation_loop", K=k, converged_ms=conv_ms, converged_iterations=n_conv,
                          loop_ms=loop_ms, loop_iterations=n_loop, us_per_iteration=round(loop_ms * 1e3 / n_loop, 3),
                          ms_at_10000_iterations=round(loop_ms / n_loop * 10000, 2))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--loop-iterations", type=int, default=2000)
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "pair":
            child_pair(int(a.child[1]), a.calls, a.warmup)
        else:
            child_loop(int(a.child[1]), int(a.child[2]), a.calls, a.warmup)
        return 0
    steps = [["pair", "1000"], ["pair", "5000"], ["loop", "8192", str(a.loop_iterations)]]
    for step in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--child", *step]
        what = "step " + " ".join(step)
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
