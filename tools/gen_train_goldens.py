#!/usr/bin/env python3
"""Generate tests/golden/train_step_small.npz: one training step of the
*reference* PointDSC (models/PointDSC.py, ``.train()``, CPU) on a small batch,
in fp32 and in fp64, for tests/test_gpu_train_step.py and
tests/test_training_reference.py.  The reference is imported at run time from
the checkout given on the command line; the fixture holds data only.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_goldens.py <reference checkout>

Case: L = 2, N = 130, B = 3, preset 3dmatch, inlier ratios 0.3 / 0.1 / 0.6, the
weights ``trained_state_dict("3dmatch", 2)`` (the file keeps their sha256, not a
copy).  Loss: plain-mean BCE on the logits + the MSE spectral-matching loss,
both as libs/loss.py calls them with ``balanced=False``.

The fp64 run replaces ``cal_seed_trans`` (not fp64-clean in rigid_transform_3d;
it carries no gradient) with a stub.

Recorded: inputs, labels, per run the loss, the logits and the BatchNorm running
statistics after the step; M of the fp64 run (its strict upper triangle: M is
symmetric with a zero diagonal) and the fp32 run's error against it; every
parameter's fp64 gradient rounded to fp32 (one rounding, 6e-8 relative: the
fp64 and fp32 gradients side by side would not fit a committed file), and per
tensor ``e32 = max|g32 - g64| / max|g64|`` computed here from the unrounded
fp64.  Ten tensors -- the biases ahead of a batch-statistics BatchNorm -- have
a mathematically zero gradient: for them ``z32 = max|g32| / G`` with G the
global max|g64|.  Asserted here: worst e32 <= 1e-4, and the zero set (max|g64| <
1e-9 G) is exactly those ten.
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pointdsc_amd.synthetic import PRESETS, synthetic_pair, trained_state_dict  # noqa: E402

L, N, PRESET, RATIOS, SEED0 = 2, 130, "3dmatch", (0.3, 0.1, 0.6), 4100


def state_sha256(sd):
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def expected_zero_set(num_layers):
    z = ["encoder.layer0.bias"]
    for i in range(num_layers):
        z.append(f"encoder.blocks.PointCN_layer_{i}.0.bias")
        p = f"encoder.blocks.NonLocal_layer_{i}"
        z += [f"{p}.fc_message.0.bias", f"{p}.fc_message.3.bias", f"{p}.projection_v.bias"]
    z.append("encoder.blocks.NonLocal_layer_0.fc_message.6.bias")
    return sorted(z)


def main(ref):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ref)
    import models.PointDSC as refmod

    torch.manual_seed(0)
    p = PRESETS[PRESET]
    sd = trained_state_dict(PRESET, L)
    pairs = [synthetic_pair(N, SEED0 + i, PRESET, r) for i, r in enumerate(RATIOS)]
    inputs = {k: np.stack([q[k] for q in pairs]) for k in pairs[0]}

    def run(dtype, stub):
        model = refmod.PointDSC(in_dim=6, num_layers=L, num_channels=128, num_iterations=10, ratio=0.1,
                                inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40,
                                nms_radius=p["nms_radius"])
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model = model.to(dtype).train()
        if stub:
            eye = torch.eye(4, dtype=dtype)[None].repeat(len(pairs), 1, 1)
            model.cal_seed_trans = lambda seeds, feats, src, tgt: (None, None, eye, None)
        data = {k: torch.from_numpy(inputs[k]).to(dtype) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
        gt = torch.from_numpy(inputs["gt_labels"]).to(dtype)
        res = model(data)
        gt_M = ((gt[:, None, :] + gt[:, :, None]) == 2).to(dtype)
        for i in range(gt_M.shape[0]):
            gt_M[i].fill_diagonal_(0)
        loss = F.binary_cross_entropy_with_logits(res["final_labels"], gt, reduction="mean") \
            + F.mse_loss(res["M"], gt_M, reduction="mean")
        loss.backward()
        grads = {n: q.grad.detach().numpy().copy() for n, q in model.named_parameters() if q.grad is not None}
        stats = {n: b.detach().numpy().copy() for n, b in model.named_buffers() if b.dtype == dtype}
        return (loss.item(), res["final_labels"].detach().numpy().copy(), res["M"].detach().numpy().copy(),
                grads, stats, res["final_trans"].detach().numpy().copy())

    loss32, logits32, M32, g32, rs32, trans32 = run(torch.float32, False)
    loss64, logits64, M64, g64, rs64, _ = run(torch.float64, True)
    assert list(g32) == list(g64)

    G = max(np.abs(v).max() for v in g64.values())
    names = list(g64)
    zero = sorted(n for n in names if np.abs(g64[n]).max() < 1e-9 * G)
    assert zero == expected_zero_set(L), zero
    e32 = np.array([np.nan if n in zero else np.abs(g32[n] - g64[n]).max() / np.abs(g64[n]).max() for n in names])
    z32 = np.array([np.abs(g32[n]).max() / G if n in zero else np.nan for n in names])
    worst = np.nanmax(e32)
    assert worst <= 1e-4, worst
    iu = np.triu_indices(N, 1)
    assert np.abs(M64 - M64.transpose(0, 2, 1)).max() < 1e-14 and np.abs(M64[:, np.arange(N), np.arange(N)]).max() == 0
    out = dict(inputs)
    out.update(num_layers=np.int32(L), preset=np.array(PRESET), ratio=np.float64(0.1),
               state_sha256=np.array(state_sha256(sd)),
               loss32=np.float32(loss32), loss64=np.float64(loss64), logits32=logits32, logits64=logits64,
               M64_triu=M64[:, iu[0], iu[1]], e_M32=np.float64(np.abs(M32 - M64).max() / np.abs(M64).max()),
               final_trans32=trans32, grad_names=np.array(names), zero_names=np.array(zero), grad_e32=e32,
               grad_z32=z32, grad_G=np.float64(G))
    for n in names:
        out["g64." + n] = g64[n].astype(np.float32)
    for n in rs64:
        out["rs64." + n] = rs64[n]
        out["rs32." + n] = rs32[n]
    path = os.path.join(REPO, "tests", "golden", "train_step_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; loss32 {loss32:.8f} loss64 {loss64:.12f}; "
          f"worst e32 {worst:.3g}; e_M32 {float(out['e_M32']):.3g}; zero-gradient tensors {len(zero)}, "
          f"worst z32 {np.nanmax(z32):.3g}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["POINTDSC_REFERENCE"])
