"""The fused spectral-matching loss (csrc/sm_loss_fused.hip) on the GPU against its
restatement in fp64 torch on the CPU (tests/_sm_fused_ref.py), on the same fp32 inputs.

Bars, with e(x) = max|x - x64| / max|x64| and e32 the same restatement in fp32:
  dnormed        e(hip) <= 4 e32 of the same case (tests/test_gpu_attention_backward.py's rule)
  loss, dsigma   scalars, whose fp32 error in one case can be small by accident:
                 e(hip) <= 4 max(own e32, the worst e32 of that quantity over the shape
                 table, every sigma and both modes), computed here, not hard-coded
  where x64 is identically zero (N = 1, every pair clamped, no gradient-carrying
  pair, zero upstream gradient) the kernel's output is exactly 0: G is 0 there.
Precondition of every case (check_precondition): no gt pair within 64 eps / sigma^2
of u = 0 and no other pair that close to u = 1, where dL/du jumps."""
import ctypes

import numpy as np
import pytest
import torch

from _sm_fused_ref import C, SHAPES, SIGMAS, case, check_precondition, err, make_inputs, restate, table_worst_e32

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
ERR_ARG, ERR_UNSUPPORTED = 1, 3  # include/pdsc.h: PDSC_ERR_ARG, PDSC_ERR_UNSUPPORTED


def _run(normed, sigma, labels, balanced, grads=True):
    from pointdsc_amd import kernels
    out = kernels.sm_loss_fused(normed.to(DEV), torch.tensor([sigma], dtype=torch.float32, device=DEV),
                                labels.to(DEV), balanced, grads)
    return tuple(None if t is None else t.cpu() for t in out)


def _hold(what, hip, r64, e32, sigma):
    """The module docstring's bars; returns the failures, each with both figures."""
    check_precondition(r64, sigma)
    bad = []
    for key, x in zip(("loss", "dnormed", "dsigma"), hip):
        e = err(x, r64[key])
        if e is None:
            nz = int(np.count_nonzero(np.asarray(x)))
            print(f"{what} {key}: x64 == 0, {nz} non-zero outputs")
            if nz:
                bad.append(f"{what} {key}: {nz} non-zero outputs where x64 is identically zero")
            continue
        bar = e32[key] if key == "dnormed" else max(e32[key], table_worst_e32(key))
        line = f"{what} {key}: e = {e:.3e}, bar 4 x {bar:.3e}"
        print(line)
        if not e <= 4 * bar:
            bad.append(line)
    return bad


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("B,N", SHAPES)
def test_matches_fp64_restatement(B, N, sigma):
    bad = []
    for balanced in (True, False):
        normed, labels, r64, e32 = case(B, N, sigma, balanced)
        bad += _hold(f"({B},{N}) sigma {sigma} balanced {balanced}", _run(normed, sigma, labels, balanced), r64, e32,
                     sigma)
    assert not bad, "\n".join(bad)


def test_streamed_tiles_are_split_at_700():
    """(1,700) of the table runs more than one split: its workspace holds at least two [N,C] partials."""
    from pointdsc_amd.kernels import query
    assert query("pdsc_sm_loss_fused_workspace_bytes", 1, 700, C) >= 2 * 700 * C * 4
    # ... and none where B x ceil(N / 128) workgroups fill the chip
    assert query("pdsc_sm_loss_fused_workspace_bytes", 64, 1024, C) < 64 * 1024 * C * 4


def _with_labels(labels, seed):
    """make_inputs' recipe on given labels."""
    gen = torch.Generator().manual_seed(seed)
    B, N = labels.shape
    x = torch.randn(B, N, C, generator=gen) + labels[:, :, None] * torch.randn(B, 1, C, generator=gen)
    return torch.nn.functional.normalize(x, p=2, dim=-1)


def _label_cases():
    B, N = 2, 130
    one = torch.zeros(B, N)
    one[0, 17] = one[1, 129] = 1
    normed, labels = make_inputs(B, N)
    twin = normed.clone()
    for b in range(B):  # two identical rows, both labelled 1: u ~ 1 on a gt pair
        i, j = torch.nonzero(labels[b] == 1)[[0, -1], 0]
        twin[b, j] = twin[b, i]
    return {"all labels 0": (_with_labels(torch.zeros(B, N), 1), torch.zeros(B, N)),
            "all labels 1": (_with_labels(torch.ones(B, N), 2), torch.ones(B, N)),
            "one label 1": (_with_labels(one, 3), one),
            "identical rows": (twin, labels)}


# sigma 0.7 for the two cases that must be identically zero: with k_b <= 1 every pair is a
# negative, whose s stays below 0.45 here (128 channels: s ~ N(0, 1/128) among random rows,
# 0.5 / sqrt(2) between the labelled row and the rest), and u < 0 needs s < 1 - sigma^2 = 0.51
# (sigma 0.8 would need s < 0.36, which a few pairs exceed; their u ~ 1e-3 then carries the
# whole loss at fp32's absolute error of u, 1e-7).  The cases with gt pairs stay at 0.8, where
# check_precondition holds (at 0.7 their u straddles 0).
@pytest.mark.parametrize("name,sigma", [("all labels 0", 0.7), ("all labels 0", 1.0), ("all labels 1", 0.8),
                                        ("all labels 1", 1.0), ("one label 1", 0.7), ("one label 1", 1.0),
                                        ("identical rows", 0.8), ("identical rows", 1.0)])
def test_label_edge_cases(name, sigma):
    normed, labels = _label_cases()[name]
    if sigma == 0.7:  # k_b <= 1 and every u < 0: nothing carries a gradient
        r64 = restate(normed, sigma, labels, True)
        assert float(r64["u"][~torch.eye(130, dtype=torch.bool).expand(2, -1, -1)].max()) < 0
        assert float(r64["dnormed"].abs().max()) == 0 and float(r64["dsigma"]) == 0 and float(r64["loss"]) == 0
    bad = []
    for balanced in (True, False):
        r64 = restate(normed, sigma, labels, balanced)
        r32 = restate(normed, sigma, labels, balanced, torch.float32)
        e32 = {k: err(r32[k], r64[k]) for k in ("loss", "dnormed", "dsigma")}
        bad += _hold(f"{name} sigma {sigma} balanced {balanced}", _run(normed, sigma, labels, balanced), r64, e32, sigma)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("balanced", [True, False])
def test_bitwise_properties(balanced):
    """Two calls, a non-contiguous input, a permuted batch and the loss-only variant."""
    normed, labels = make_inputs(2, 130)
    a, b = _run(normed, 1.0, labels, balanced), _run(normed, 1.0, labels, balanced)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    from pointdsc_amd import kernels
    wide = torch.zeros(2, 130, 2 * C, device=DEV)
    wide[:, :, ::2] = normed.to(DEV)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    sig = torch.tensor([1.0], device=DEV)
    v = kernels.sm_loss_fused(view, sig, labels.to(DEV), balanced)
    assert all(torch.equal(x, y.cpu()) for x, y in zip(a, v))
    p = _run(normed.flip(0), 1.0, labels.flip(0), balanced)
    assert torch.equal(p[1], a[1].flip(0))
    only = _run(normed, 1.0, labels, balanced, grads=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], a[0])


@pytest.mark.parametrize("upstream", [0.0, 3.5])
def test_autograd_scales_the_unit_gradients(upstream):
    from pointdsc_amd.training import FeatureSimilarity, SpectralMatchingLoss
    normed, labels = make_inputs(2, 130)
    _, dn, ds = _run(normed, 1.0, labels, True)
    n = normed.to(DEV).requires_grad_(True)
    sigma = torch.nn.Parameter(torch.tensor([1.0], device=DEV))
    loss = SpectralMatchingLoss()(FeatureSimilarity(n, sigma), labels.to(DEV))
    assert loss.dtype == torch.float64 and loss.shape == ()
    (loss * upstream).backward()
    assert n.grad.dtype == torch.float32 and sigma.grad.dtype == torch.float32 and sigma.grad.shape == (1,)
    assert torch.equal(n.grad.cpu(), torch.tensor(upstream) * dn)
    assert torch.equal(sigma.grad.cpu(), (upstream * ds).float().reshape(1))
    if upstream == 0.0:
        assert not n.grad.any() and not sigma.grad.any()
    else:
        assert n.grad.any() and sigma.grad.any()


def test_no_grad_computes_the_loss_alone(monkeypatch):
    from pointdsc_amd import kernels, training
    normed, labels = make_inputs(2, 130)
    seen, fused = [], kernels.sm_loss_fused

    def spy(*args, **kw):
        out = fused(*args, **kw)
        seen.append(out)
        return out

    monkeypatch.setattr(training.kernels, "sm_loss_fused", spy, raising=True)
    n = normed.to(DEV).requires_grad_(True)
    sigma = torch.nn.Parameter(torch.tensor([1.0], device=DEV))
    with torch.no_grad():
        a = training.SpectralMatchingLoss()(training.FeatureSimilarity(n, sigma), labels.to(DEV))
    b = training.SpectralMatchingLoss()(training.FeatureSimilarity(n.detach(), sigma.detach()), labels.to(DEV))
    c = training.SpectralMatchingLoss()(training.FeatureSimilarity(n, sigma), labels.to(DEV))
    assert [s[1] is None and s[2] is None for s in seen] == [True, True, False]
    assert not a.requires_grad and not b.requires_grad and c.requires_grad
    assert torch.equal(a, c.detach()) and torch.equal(b, a)


def test_peak_memory_is_below_one_dense_M():
    """B = 1, N = 2048: outputs 1 MiB, at most 8 split partials of 1 MiB, against 4 B N^2 = 16 MiB."""
    from pointdsc_amd.training import FeatureSimilarity, SpectralMatchingLoss
    B, N = 1, 2048
    normed, labels = make_inputs(B, N)
    n = normed.to(DEV).requires_grad_(True)
    sigma = torch.nn.Parameter(torch.tensor([1.0], device=DEV))
    labels = labels.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    SpectralMatchingLoss()(FeatureSimilarity(n, sigma), labels).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak {peak} bytes over the fused forward + backward, one dense M is {4 * B * N * N}")
    assert peak < 4 * B * N * N
    assert n.grad.any() and sigma.grad.any()


def test_abi_errors_on_the_host():
    """Checked before any device work (dummy non-null pointers: nothing is dereferenced)."""
    from pointdsc_amd import _lib
    lib = _lib.load()
    p, big = ctypes.c_void_p(256), 1 << 30
    fn = lib.pdsc_sm_loss_fused_f32
    need = lib.pdsc_sm_loss_fused_workspace_bytes(2, 130, C)
    assert need > 0 and need % 256 == 0
    for k in (0, 1, 2, 7, 10):  # normed, sigma, gt_labels, loss, workspace
        args = [p, p, p, 2, 130, C, 1, p, p, p, p, big, None]
        args[k] = None
        assert fn(*args) == ERR_ARG and b"null" in lib.pdsc_last_error(), k
    assert fn(p, p, p, 0, 130, C, 1, p, p, p, p, big, None) == ERR_ARG
    assert fn(p, p, p, 2, 0, C, 1, p, p, p, p, big, None) == ERR_ARG
    assert fn(p, p, p, 2, 130, C, 1, p, p, None, p, big, None) == ERR_ARG  # one gradient pointer only
    assert fn(p, p, p, 2, 130, C, 1, p, None, p, p, big, None) == ERR_ARG
    assert b"both or neither" in lib.pdsc_last_error()
    assert fn(p, p, p, 2, 130, 64, 1, p, p, p, p, big, None) == ERR_UNSUPPORTED
    assert lib.pdsc_sm_loss_fused_workspace_bytes(2, 130, 64) == 0
    assert lib.pdsc_sm_loss_fused_workspace_bytes(0, 130, C) == 0 and lib.pdsc_sm_loss_fused_workspace_bytes(2, 0, C) == 0
    assert fn(p, p, p, 2, 130, C, 1, p, p, p, p, need - 1, None) == ERR_ARG
    assert b"workspace too small" in lib.pdsc_last_error()
