"""One training step of pointdsc_amd.training.TrainablePointDSC on the GPU -- the
HIP attention forward and backward under autograd, torch ops around it --
against the reference's recorded step (tests/golden/train_step_small.npz,
tools/gen_train_goldens.py): L = 2, N = 130, B = 3, plain-mean BCE + MSE
spectral-matching loss.

Bars (tests/_train_fixture.py: check_step): the loss, the logits, M, every
parameter gradient and the BatchNorm running statistics after the step against
the fp64 record within 4 x the reference's own fp32 error, e(x) = max|x - x64| /
max|x64| (gradients: 4 x the worst tensor's); the ten mathematically zero
gradients by max|g| / G within 4 x the reference's fp32 figure."""
import numpy as np
import pytest
import torch

from _train_fixture import check_step, fixture, hparams, state_tensors, step_loss

pytestmark = pytest.mark.gpu


def _data(fx, dev):
    g = fx["g"]
    data = {k: torch.from_numpy(g[k]).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    return data, torch.from_numpy(g["gt_labels"]).to(dev)


def _model(fx, dev):
    from pointdsc_amd.training import TrainablePointDSC
    model = TrainablePointDSC(**hparams(fx))
    model.load_state_dict(state_tensors(fx), strict=True)
    return model.to(dev).train()


def test_train_step_matches_reference():
    dev = torch.device("cuda")
    fx = fixture()
    model = _model(fx, dev)
    data, gt = _data(fx, dev)
    res = model(data)
    loss = step_loss(res, gt)
    loss.backward()
    B = gt.shape[0]
    trans = res["final_trans"]
    assert trans.shape == (B, 4, 4) and not trans.requires_grad and trans.grad_fn is None
    assert bool(torch.isfinite(trans).all())
    grads = {n: p.grad.cpu().numpy() for n, p in model.named_parameters() if p.grad is not None}
    stats = {n: b.detach().cpu().numpy() for n, b in model.named_buffers()}
    bad = check_step(fx, loss.item(), res["final_labels"].detach().cpu().numpy(), res["M"].detach().cpu().numpy(),
                     grads, stats)
    assert not bad, "\n".join(bad)


def test_adam_step_then_inference_roundtrip():
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.training import TrainablePointDSC
    dev = torch.device("cuda")
    fx = fixture()
    model = _model(fx, dev)
    data, gt = _data(fx, dev)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-6)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    step_loss(model(data), gt).backward()
    opt.step()
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert "encoder.blocks.NonLocal_layer_0.projection_q.weight" in moved and "sigma_spat" not in moved
    infer = PointDSC(**hparams(fx)).to(dev)
    infer.load_state_dict(model.state_dict(), strict=True)
    infer.eval()
    one = {k: v[:1].contiguous() for k, v in data.items()}
    out = infer(dict(one, testing=True))
    assert out["final_trans"].shape == (1, 4, 4) and bool(torch.isfinite(out["final_trans"]).all())
    # ... and back, and the trainable module's own 'testing' call is that model's
    back = TrainablePointDSC(**hparams(fx)).to(dev)
    back.load_state_dict(infer.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), model.state_dict().values()))
    own = model(dict(one, testing=True))
    assert torch.equal(own["final_trans"], out["final_trans"]) and torch.equal(own["final_labels"], out["final_labels"])


def test_eval_mode_uses_running_statistics():
    dev = torch.device("cuda")
    fx = fixture()
    model = _model(fx, dev).eval()
    data, _ = _data(fx, dev)
    stats = {n: b.clone() for n, b in model.named_buffers()}
    with torch.no_grad():
        a, b = model(data), model({k: v[:1] for k, v in data.items()})
    assert all(torch.equal(t, stats[n]) for n, t in model.named_buffers())
    # no batch statistics: a pair's logits do not depend on its batch
    assert (a["final_labels"][:1] - b["final_labels"]).abs().max().item() < 1e-3 * a["final_labels"].abs().max().item()


def test_inference_module_still_refuses_training():
    from pointdsc_amd.PointDSC import PointDSC
    dev = torch.device("cuda")
    fx = fixture()
    data, _ = _data(fx, dev)
    with pytest.raises(NotImplementedError):
        PointDSC(**hparams(fx)).to(dev).train()(data)
