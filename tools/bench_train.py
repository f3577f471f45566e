#!/usr/bin/env python3
"""Training timings (DESIGN.md §7 "Training") at B=16 N=1000, B=1 N=1000 and
B=1 N=5000:

  op        pointdsc_amd.training.nonlocal_attention, forward + backward
  composed  the same function from torch ops on the same device (the baseline:
            softmax(M * q k^T / sqrt(C)) v under autograd, [B,N,N] materialised)
  step      one full training step at L = 12: TrainablePointDSC forward, the
            BCE + spectral-matching loss, backward, Adam

and the spectral-matching loss leg (--legs sm_loss, or all), each shape in turn:

  sm_fused     SpectralMatchingLoss on a FeatureSimilarity (the fused kernel of
               csrc/sm_loss_fused.hip), forward + backward into normed and sigma
  sm_composed  the same loss on FeatureSimilarity.dense(): torch ops, [B,N,N] materialised
  step         as above (model.dense_M = True), in the same run for the comparison
  step_fused   the full step with model.dense_M = False

Every (shape, what) step runs in a child process of its own under its own time
limit; the first step that fails ends the run.  Times are medians of per-call
device times between HIP events on the current stream, after warm-up; each child
also reports the peak device memory torch allocated.

    python tools/bench_train.py [--calls 20] [--warmup 3] [--step-timeout 180] [--legs {attention,sm_loss,all}]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 1000), (1, 1000), (1, 5000)]
WHAT = ["op", "composed", "step"]
SM_WHAT = ["sm_fused", "sm_composed", "step", "step_fused"]


def child(what, B, N, calls, warmup):
    import numpy as np
    import torch
    from pointdsc_amd import kernels
    from pointdsc_amd.synthetic import PRESETS, synthetic_batch
    from pointdsc_amd.training import (ClassificationLoss, FeatureSimilarity, SpectralMatchingLoss, TrainablePointDSC,
                                       composed_attention, nonlocal_attention)
    dev = torch.device("cuda:0")
    batch = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_batch(B, N, 11, "3dmatch", 0.3).items()}
    if what in ("step", "step_fused"):
        p = PRESETS["3dmatch"]
        model = TrainablePointDSC(in_dim=6, num_layers=12, inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"],
                                  nms_radius=p["nms_radius"]).to(dev).train()
        model.dense_M = what == "step"
        opt = torch.optim.Adam([q for q in model.parameters() if q.requires_grad], lr=1e-4, weight_decay=1e-6)
        cls, sm = ClassificationLoss(balanced=False), SpectralMatchingLoss(balanced=False)

        def run():
            res = model(batch)
            loss = cls(res["final_labels"], batch["gt_labels"])["loss"] + sm(res["M"], batch["gt_labels"])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    elif what in ("sm_fused", "sm_composed"):
        gen = torch.Generator(device="cpu").manual_seed(5)
        gt = batch["gt_labels"]
        # inliers share a direction: their pairs sit near s = 0.5, the rest near 0
        x = torch.randn(B, N, 128, generator=gen).to(dev) + gt[:, :, None] * torch.randn(B, 1, 128, generator=gen).to(dev)
        normed = torch.nn.functional.normalize(x, p=2, dim=-1).requires_grad_()
        sigma = torch.nn.Parameter(torch.tensor([1.0], device=dev))
        sm = SpectralMatchingLoss(balanced=False)

        def run():
            normed.grad = sigma.grad = None
            fs = FeatureSimilarity(normed, sigma)
            sm(fs if what == "sm_fused" else fs.dense(), gt).backward()
    else:
        gen = torch.Generator(device="cpu").manual_seed(5)
        q, k, v, g = (torch.randn(B, N, 128, generator=gen).to(dev) for _ in range(4))
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        M = kernels.compat(batch["src_keypts"], batch["tgt_keypts"], torch.tensor([0.1], device=dev))
        fn = nonlocal_attention if what == "op" else composed_attention

        def run():
            q.grad = k.grad = v.grad = None
            fn(q, k, v, M).backward(g)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps(dict(what=what, B=B, N=N, calls=calls, ms_median=round(float(np.median(ms)), 4),
                          ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
                          peak_mib=round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=float, default=180.0)
    ap.add_argument("--legs", choices=["attention", "sm_loss", "all"], default="all")
    ap.add_argument("--child", nargs=3, metavar=("WHAT", "B", "N"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), a.calls, a.warmup)
        return 0
    legs = [WHAT] * (a.legs != "sm_loss") + [SM_WHAT] * (a.legs != "attention")
    for B, N, what in ((B, N, what) for leg in legs for B, N in SHAPES for what in leg):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, str(B), str(N), "--calls", str(a.calls),
               "--warmup", str(a.warmup)]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"step {what} B={B} N={N}: time limit of {a.step_timeout:g} s; stopping", file=sys.stderr)
            return 124
        if p.returncode != 0:
            print(f"step {what} B={B} N={N}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
