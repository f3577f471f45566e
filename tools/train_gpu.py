#!/usr/bin/env python3
"""Train PointDSC on the GPU on synthetic pairs: the device counterpart of
tools/train_synthetic.py.  pointdsc_amd.training.TrainablePointDSC (the HIP
attention forward and backward under autograd), the reference's default losses
(plain-mean BCE + MSE spectral matching, config.py:43-46) and its optimizer
(Adam, lr 1e-4, weight decay 1e-6, config.py:51-56; batch 16 x 1000
correspondences, :74-79).  Prints the loss and the classification accuracy;
writes the weights (an .npz of the state dict, loadable into
pointdsc_amd.PointDSC.PointDSC) only to the path given with --out.

    python tools/train_gpu.py {3dmatch,kitti} [--iters 400] [--layers 12] [--bs 16] [--num-node 1000]
                               [--fused_sm_loss] [--out W.npz]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("preset", choices=["3dmatch", "kitti"])
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--num-node", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-6)
    ap.add_argument("--balanced", action="store_true", help="the balanced forms of both losses")
    ap.add_argument("--fused_sm_loss", action="store_true",
                    help="the spectral-matching loss on the fused kernel: M is never built (model.dense_M = False)")
    ap.add_argument("--out", default=None, help="write the trained state dict here (.npz); nothing is written without it")
    a = ap.parse_args()

    import torch
    from pointdsc_amd.synthetic import PRESETS, synthetic_pair, synthetic_state_dict
    from pointdsc_amd.training import ClassificationLoss, SpectralMatchingLoss, TrainablePointDSC

    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    p = PRESETS[a.preset]
    model = TrainablePointDSC(in_dim=6, num_layers=a.layers, num_channels=128, num_iterations=10, ratio=0.1,
                              inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40,
                              nms_radius=p["nms_radius"])
    init = synthetic_state_dict(a.layers, 128, seed=7, sigma_d=p["sigma_d"], cls_bias=0.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()}, strict=True)
    model = model.to(dev).train()
    model.dense_M = not a.fused_sm_loss
    opt = torch.optim.Adam([q for q in model.parameters() if q.requires_grad], lr=a.lr, weight_decay=a.weight_decay)
    cls, sm = ClassificationLoss(balanced=a.balanced), SpectralMatchingLoss(balanced=a.balanced)
    rng = np.random.RandomState(1234)
    t0 = time.time()
    for it in range(a.iters):
        pairs = [synthetic_pair(a.num_node, int(rng.randint(1 << 30)), a.preset, float(rng.uniform(0.05, 0.5)))
                 for _ in range(a.bs)]
        data = {k: torch.from_numpy(np.stack([q[k] for q in pairs])).to(dev)
                for k in ("corr_pos", "src_keypts", "tgt_keypts")}
        gt = torch.from_numpy(np.stack([q["gt_labels"] for q in pairs])).to(dev)
        res = model(data)
        stats = cls(res["final_labels"], gt)
        loss = stats["loss"] + sm(res["M"], gt)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if all(bool(torch.isfinite(q.grad).all()) for q in model.parameters() if q.grad is not None):
            opt.step()
        if it % 25 == 0 or it == a.iters - 1:
            acc = ((res["final_labels"].detach() > 0).float() == gt).float().mean().item()
            print(f"[{a.preset}] it {it:4d} loss {loss.item():.4f} cls {stats['loss'].item():.4f} acc {acc:.3f} "
                  f"t {time.time() - t0:.0f}s", flush=True)
    if a.out:
        np.savez_compressed(a.out, **{k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
        print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
