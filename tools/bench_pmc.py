#!/usr/bin/env python3
"""Wall time of the PMC baseline (pointdsc_amd.baselines.PMC, include/pdsc.h f8)
and of its pieces: the consistency graph, the greedy lower bound
(pdsc_greedy_clique), the whole maximum-clique call (pdsc_max_clique; "exact" is
that minus the lower bound, which it contains) and the whole PMC call, on
synthetic pairs (pointdsc_amd/synthetic.py, 3dmatch preset) of 1000 and 5000
correspondences in both edge modes.  Then the case the default node budget is
sized by: a dense random graph G(2048, 0.9) in which no root finishes, so every
root spends its whole budget (--budgets to try others; 0 = the default).

Every row runs in a child process of its own under its own time limit; the
first that fails ends the run.  Times are medians of host wall clock around
single calls that end in one synchronise, after warm-up.  Next to the times:
the result's size, exact, heuristic_size, roots_incomplete and nodes.

    python tools/bench_pmc.py [--calls 5] [--warmup 1] [--step-timeout 120] [--budgets 0]
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


def median_ms(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4), out


def info_fields(info):
    return dict(size=info.size, exact=info.exact, heuristic_size=info.heuristic_size,
                roots_incomplete=info.roots_incomplete, nodes=info.nodes)


def child_pair(n, mode, calls, warmup):
    import torch
    from pointdsc_amd import kernels as K
    from pointdsc_amd.baselines import PMC
    from pointdsc_amd.synthetic import synthetic_pair
    dev = torch.device("cuda:0")
    pair = synthetic_pair(n, seed=11)
    corr, src, tgt = (torch.from_numpy(pair[k][None]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    graph_ms, (adj, degree) = median_ms(lambda: K.consistency_graph(corr[0], 0.10, mode), calls, warmup)
    heur_ms, _ = median_ms(lambda: K.max_clique(adj, heuristic_only=True), calls, warmup)
    clique_ms, (_, _, result) = median_ms(lambda: K.max_clique(adj), calls, warmup)
    pmc_ms, _ = median_ms(lambda: PMC(corr, src, tgt, 0.10, mode), calls, warmup)
    print(json.dumps(dict(case="synthetic_pair", N=n, mode=mode, edges=int(degree.sum().item()) // 2,
                          graph_ms=graph_ms, heuristic_ms=heur_ms, max_clique_ms=clique_ms,
                          exact_ms=round(clique_ms - heur_ms, 4), pmc_ms=pmc_ms, **info_fields(K.CliqueInfo(result)))))


def child_dense(n, p, budget, calls, warmup):
    import numpy as np
    import torch
    from pointdsc_amd import _lib, kernels as K
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(7)
    e = np.triu(rng.random_sample((n, n)) < p, 1)
    e = e | e.T
    W = (n + 63) // 64
    pad = np.zeros((n, W * 64), np.uint8)
    pad[:, :n] = e
    adj = torch.from_numpy(np.packbits(pad, axis=1, bitorder="little").view("<u8").astype(np.uint64).view(np.int64)
                           .reshape(n, W)).to(dev)
    heur_ms, _ = median_ms(lambda: K.max_clique(adj, heuristic_only=True), calls, warmup)
    clique_ms, (_, _, result) = median_ms(lambda: K.max_clique(adj, node_budget=budget), calls, warmup)
    print(json.dumps(dict(case=f"G({n},{p})", N=n, node_budget=budget or int(_lib.load().pdsc_max_clique_default_budget()),
                          edges=int(e.sum()) // 2, heuristic_ms=heur_ms, max_clique_ms=clique_ms,
                          exact_ms=round(clique_ms - heur_ms, 4), **info_fields(K.CliqueInfo(result)))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=float, default=120.0)
    ap.add_argument("--budgets", type=int, nargs="+", default=[0], help="node budgets of the G(2048, 0.9) case")
    ap.add_argument("--only-dense", action="store_true", help="skip the synthetic pairs")
    ap.add_argument("--child", nargs="+", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "pair":
            child_pair(int(a.child[1]), a.child[2], a.calls, a.warmup)
        else:
            child_dense(int(a.child[1]), float(a.child[2]), int(a.child[3]), a.calls, a.warmup)
        return 0
    steps = [] if a.only_dense else [["pair", str(n), mode] for n in (1000, 5000) for mode in ("squared", "length")]
    steps += [["dense", "2048", "0.9", str(b)] for b in a.budgets]
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
