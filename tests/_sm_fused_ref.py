"""The fused spectral-matching loss restated in torch on the CPU, its seeded
inputs and its shape table, as the tests of the fused kernel read them: each
case is computed once, shared and left unchanged.

    s_ij = n_i.n_j    u_ij = 1 - (1 - s_ij) / sigma^2    M_ij = clamp(u_ij, 0, 1), M_ii = 0
    gt_ij = (l_i == 1 and l_j == 1 and i != j),  k_b = #{l_i == 1}
    balanced: P_b = max(k_b (k_b - 1) - 1, 0) + 1,  Q_b = max(N^2 - k_b (k_b - 1) - 1, 0) + 1
              L = 1/B sum_b [0.5 / P_b sum_gt (M - 1)^2 + 0.5 / Q_b sum_!gt M^2]
              G_ij = (M_ij - 1) / (B P_b) on gt, M_ij / (B Q_b) elsewhere
    MSE:      L = 1/(B N^2) sum (M - gt)^2,  G_ij = 2 (M_ij - gt_ij) / (B N^2)
    G_ij *= (0 <= u_ij <= 1) and (i != j)
    dL/dn_i = (2 / sigma^2) sum_j G_ij n_j     dL/dsigma = (2 / sigma^3) sum_ij G_ij (1 - s_ij)
"""
import functools

import numpy as np
import torch

C = 128
SHAPES = ((1, 1), (1, 2), (2, 33), (1, 95), (3, 130), (1, 257), (2, 300), (1, 700))  # (B, N)
SIGMAS = (0.5, 0.8, 1.0, 2.0)
EPS32 = float(np.finfo(np.float32).eps)
# (B, N, sigma) -> seed, where the seed 1000 N + B trips check_precondition:
# (3,130) at sigma 0.8 has one gt pair (both orders) within the margin of u = 0
MOVED_SEEDS = {(3, 130, 0.8): 130004}


def make_inputs(B, N, seed=None):
    """l ~ Bernoulli(0.4), n = normalize(randn(B,N,128) + l c), one c ~ randn per
    pair; seed 1000 N + B.  (normed fp32 [B,N,128], labels fp32 [B,N])."""
    gen = torch.Generator().manual_seed(1000 * N + B if seed is None else seed)
    labels = (torch.rand(B, N, generator=gen) < 0.4).float()
    c = torch.randn(B, 1, C, generator=gen)
    x = torch.randn(B, N, C, generator=gen) + labels[:, :, None] * c
    return torch.nn.functional.normalize(x, p=2, dim=-1), labels


def restate(normed, sigma, labels, balanced, dtype=torch.float64):
    """dict(loss, dnormed, dsigma, u, gt) of the formulas above in ``dtype`` on the given fp32 inputs."""
    n = normed.to(dtype)
    sig = torch.as_tensor(sigma, dtype=torch.float32).reshape(()).to(dtype)
    B, N, _ = n.shape
    eye = torch.eye(N, dtype=torch.bool)
    s = n @ n.transpose(1, 2)
    u = 1 - (1 - s) / sig ** 2
    M = u.clamp(0, 1).masked_fill(eye, 0)
    pos = labels == 1
    gt = pos[:, :, None] & pos[:, None, :] & ~eye
    gtf = gt.to(dtype)
    if balanced:
        k = pos.sum(1).to(dtype)
        P = (k * (k - 1) - 1).clamp(min=0) + 1
        Q = (N * N - k * (k - 1) - 1).clamp(min=0) + 1
        loss = (0.5 / P * ((M - 1) ** 2 * gtf).sum((1, 2)) + 0.5 / Q * (M ** 2 * (1 - gtf)).sum((1, 2))).sum() / B
        G = torch.where(gt, (M - 1) / (B * P)[:, None, None], M / (B * Q)[:, None, None])
    else:
        loss = ((M - gtf) ** 2).sum() / (B * N * N)
        G = 2 * (M - gtf) / (B * N * N)
    G = G * ((u >= 0) & (u <= 1) & ~eye).to(dtype)
    return dict(loss=loss, dnormed=2 / sig ** 2 * (G @ n), dsigma=2 / sig ** 3 * (G * (1 - s)).sum(), u=u, gt=gt)


def err(x, x64):
    """e(x) = max|x - x64| / max|x64| (fp64); None where x64 is identically zero."""
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    scale = np.abs(x64).max()
    return float(np.abs(x - x64).max() / scale) if scale > 0 else None


def check_precondition(r64, sigma):
    """dL/du jumps where a gt pair has u = 0 or another pair has u = 1: no such
    pair (off the diagonal) within 64 eps / sigma^2 of the jump."""
    u, gt = r64["u"], r64["gt"]
    off = ~torch.eye(u.shape[1], dtype=torch.bool)
    margin = 64 * EPS32 / float(sigma) ** 2
    near0 = int((gt & (u.abs() < margin)).sum())
    near1 = int((~gt & off & ((u - 1).abs() < margin)).sum())
    assert near0 == 0 and near1 == 0, f"{near0} gt pairs at u = 0, {near1} other pairs at u = 1: move the seed"


@functools.lru_cache(maxsize=None)
def case(B, N, sigma, balanced):
    """(normed, labels, r64, e32) of a table case: e32 = dict(loss, dnormed, dsigma) of the fp32 restatement."""
    normed, labels = make_inputs(B, N, MOVED_SEEDS.get((B, N, sigma)))
    r64 = restate(normed, sigma, labels, balanced)
    r32 = restate(normed, sigma, labels, balanced, torch.float32)
    return normed, labels, r64, {k: err(r32[k], r64[k]) for k in ("loss", "dnormed", "dsigma")}


@functools.lru_cache(maxsize=None)
def table_worst_e32(key):
    """The worst fp32 error of a scalar ('loss' or 'dsigma') over the shape table, every sigma and both modes."""
    es = [case(B, N, s, bal)[3][key] for B, N in SHAPES for s in SIGMAS for bal in (True, False)]
    return max(e for e in es if e is not None)
