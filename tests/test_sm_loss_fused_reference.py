"""The formulas the fused spectral-matching loss implements, and its CPU-side
plumbing -- no GPU needed.

The analytic d loss / d normed and d loss / d sigma of tests/_sm_fused_ref.py
(clamp mask included) against autograd through the composed torch path
(FeatureSimilarity.dense() + SpectralMatchingLoss) in fp64; a FeatureSimilarity
on the CPU takes exactly the dense path; dense_M defaults to True."""
import pytest
import torch

from _sm_fused_ref import err, make_inputs, restate


@pytest.mark.parametrize("balanced", [True, False])
@pytest.mark.parametrize("sigma", [0.8, 1.0, 2.0])
@pytest.mark.parametrize("B,N", [(2, 33), (3, 130)])
def test_analytic_gradients_equal_autograd_fp64(B, N, sigma, balanced):
    from pointdsc_amd.training import FeatureSimilarity, SpectralMatchingLoss
    normed, labels = make_inputs(B, N)
    n64 = normed.double().requires_grad_(True)
    s64 = torch.tensor([sigma], dtype=torch.float32).double().requires_grad_(True)
    loss = SpectralMatchingLoss(balanced)(FeatureSimilarity(n64, s64).dense(), labels)
    loss.backward()
    r = restate(normed, sigma, labels, balanced)
    assert abs(float(r["loss"]) - loss.item()) <= 1e-12 * abs(loss.item())
    assert float(s64.grad.abs().max()) > 0 and float(n64.grad.abs().max()) > 0
    assert err(r["dnormed"], n64.grad) <= 1e-12
    assert err(r["dsigma"], s64.grad) <= 1e-12


@pytest.mark.parametrize("balanced", [True, False])
def test_feature_similarity_on_cpu_is_the_dense_call(balanced):
    from pointdsc_amd.training import FeatureSimilarity, SpectralMatchingLoss
    normed, labels = make_inputs(2, 33)
    out = []
    for wrap in (lambda fs: fs, lambda fs: fs.dense()):
        n = normed.clone().requires_grad_(True)
        sigma = torch.nn.Parameter(torch.tensor([1.2]))
        fs = FeatureSimilarity(n, sigma)
        assert fs.shape == (2, 33, 33)
        loss = SpectralMatchingLoss(balanced)(wrap(fs), labels)
        loss.backward()
        out.append((loss.detach(), n.grad, sigma.grad))
    assert out[0][0].dtype == torch.float64
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_dense_M_defaults_to_true_and_encode_returns_a_tensor():
    from pointdsc_amd.training import FeatureSimilarity, TrainablePointDSC, composed_attention
    torch.manual_seed(0)
    model = TrainablePointDSC(num_layers=1).train()
    assert TrainablePointDSC.dense_M is True and model.dense_M is True
    corr_pos, compat = torch.randn(2, 20, 6), torch.rand(2, 20, 20)
    M = model.encode(corr_pos, compat, attention=composed_attention)[3]
    assert isinstance(M, torch.Tensor) and M.shape == (2, 20, 20)
    model.eval()  # the same batch statistics do not matter: running statistics, no update
    with torch.no_grad():
        dense = model.encode(corr_pos, compat, attention=composed_attention)[3]
        model.dense_M = False
        fs = model.encode(corr_pos, compat, attention=composed_attention)[3]
        again = model.encode(corr_pos, compat, attention=composed_attention, dense_M=True)[3]
    assert isinstance(fs, FeatureSimilarity) and fs.shape == (2, 20, 20)
    assert torch.equal(fs.dense(), dense) and torch.equal(again, dense)
