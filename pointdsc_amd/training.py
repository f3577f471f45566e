"""Training on the MI355X: autograd through the SCNonlocal encoder with the N x N
attention of every NonLocal block, forward and backward, on the hand-written
gfx950 kernels of ``libpdsc.so`` (csrc/attention_bwd.hip), and everything that
is O(N C) -- the 1x1 convolutions, batch-statistics BatchNorm, ReLU, the
classifier, ``F.normalize`` and the classification loss -- as torch ops
(DESIGN.md §7 "Training").  The feature-similarity M and its spectral-matching
loss are torch ops on a [B,N,N] tensor by default; with ``model.dense_M = False``
M stays a ``FeatureSimilarity`` (normed and sigma) and ``SpectralMatchingLoss``
computes the loss and both gradients in one fused kernel
(csrc/sm_loss_fused.hip) that stores nothing N x N.

``pointdsc_amd.PointDSC.PointDSC`` stays the inference module and keeps refusing
``model.train()``; train with ``TrainablePointDSC`` and move the weights across
with ``state_dict()`` / ``load_state_dict(strict=True)``, either way::

    model = TrainablePointDSC(in_dim=6, num_layers=12, ...).cuda().train()
    res = model({'corr_pos': ..., 'src_keypts': ..., 'tgt_keypts': ...})
    loss = ClassificationLoss()(res['final_labels'], gt)['loss'] + SpectralMatchingLoss()(res['M'], gt)
    loss.backward()
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels
from .PointDSC import NonLocalNet, PointDSC


class _NonlocalAttention(torch.autograd.Function):
    """msg_i = sum_j softmax_j(M_ij q_i.k_j / sqrt(C)) v_j on the HIP kernels: saves
    q, k, v, msg and the row log-sum-exp; the backward recomputes the softmax."""

    @staticmethod
    def forward(ctx, q, k, v, M):
        q, k, v, M = q.contiguous(), k.contiguous(), v.contiguous(), M.contiguous()
        msg, lse = kernels.attention_lse(q, k, v, M)
        ctx.save_for_backward(q, k, v, M, msg, lse)
        return msg

    @staticmethod
    def backward(ctx, dmsg):
        q, k, v, M, msg, lse = ctx.saved_tensors
        dq, dk, dv = kernels.attention_backward(q, k, v, M, msg, lse, dmsg.contiguous())
        return dq, dk, dv, None


def nonlocal_attention(q, k, v, M):
    """The attention core of one NonLocalBlock (models/PointDSC.py:36-42) with
    gradients for q, k and v [B,N,128] (row-major; made contiguous here).  M
    [B,N,N], the symmetric non-negative spatial compatibility, gets none."""
    return _NonlocalAttention.apply(q, k, v, M)


def composed_attention(q, k, v, M):
    """The same function composed from torch ops (any device, any dtype): what
    tools/bench_train.py times the kernels against, and the stand-in the CPU
    tests pass to ``TrainablePointDSC.encode``.  Materialises [B,N,N] twice."""
    S = torch.matmul(q, k.transpose(1, 2)) / math.sqrt(q.shape[-1])
    return torch.matmul(torch.softmax(M * S, dim=-1), v)


class FeatureSimilarity:
    """The feature-similarity M of models/PointDSC.py:158-163 held as its factors:
    ``normed`` [B,N,C] and ``sigma``, with their autograd graphs.  ``dense()`` is
    the [B,N,N] tensor; ``SpectralMatchingLoss`` takes the object itself and, on a
    device, never builds that tensor."""

    def __init__(self, normed, sigma):
        self.normed, self.sigma = normed, sigma

    @property
    def shape(self):
        B, N, _ = self.normed.shape
        return torch.Size((B, N, N))

    def dense(self):
        M = torch.matmul(self.normed, self.normed.permute(0, 2, 1))
        M = torch.clamp(1 - (1 - M) / self.sigma ** 2, min=0, max=1)
        return M * (1 - torch.eye(M.shape[1], dtype=M.dtype, device=M.device))  # the diagonal := 0 (:163)


class _FusedSpectralMatchingLoss(torch.autograd.Function):
    """SpectralMatchingLoss(FeatureSimilarity(normed, sigma).dense(), gt_labels) on
    the HIP kernel of csrc/sm_loss_fused.hip.  The upstream gradient of a scalar
    is a scalar, so the forward's one pass also leaves d loss / d normed and
    d loss / d sigma; the backward scales them.  ``grads`` False: the loss alone."""

    @staticmethod
    def forward(ctx, normed, sigma, gt_labels, balanced, grads):
        loss, dnormed, dsigma = kernels.sm_loss_fused(normed.detach().float(), sigma.detach().float(),
                                                      gt_labels.detach().float(), balanced, grads)
        ctx.grads = grads
        ctx.meta = (normed.dtype, sigma.dtype, sigma.shape)
        if grads:
            ctx.save_for_backward(dnormed, dsigma)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if not ctx.grads:
            raise RuntimeError("the fused spectral-matching loss was computed without gradients")
        dnormed, dsigma = ctx.saved_tensors
        ndt, sdt, sshape = ctx.meta
        return ((dloss.to(dnormed.dtype) * dnormed).to(ndt), (dloss * dsigma).to(sdt).reshape(sshape),
                None, None, None)


class TrainablePointDSC(nn.Module):
    """models/PointDSC.py:80-197 for training: the reference's constructor
    arguments, parameter and buffer names (``state_dict()`` loads with
    ``strict=True`` into ``pointdsc_amd.PointDSC.PointDSC`` and back).

    ``forward(data)`` without the 'testing' key returns the reference's training
    branch: ``final_labels`` = the classifier logits, ``M`` = the clamped feature
    similarity with a zero diagonal (both with autograd graphs; M as a
    ``FeatureSimilarity`` when ``self.dense_M`` is False), ``final_trans``
    [B,4,4] detached.  BatchNorm uses batch statistics and updates its running
    statistics while ``self.training``, and the running statistics in ``eval()``
    (the validation loop).  With 'testing' in ``data`` the call is delegated to an
    inference ``PointDSC`` that is loaded with this module's current weights."""

    def __init__(self, in_dim=6, num_layers=6, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10):
        super().__init__()
        if num_channels != kernels.CH:
            raise ValueError(f"num_channels={num_channels}: the attention kernels implement {kernels.CH}")
        self.in_dim = in_dim
        self.num_layers = num_layers
        self.num_iterations = num_iterations
        self.ratio = ratio
        self.num_channels = num_channels
        self.inlier_threshold = inlier_threshold
        self.sigma = nn.Parameter(torch.Tensor([1.0]).float(), requires_grad=True)
        self.sigma_spat = nn.Parameter(torch.Tensor([sigma_d]).float(), requires_grad=False)
        self.k = k
        self.nms_radius = nms_radius
        self.encoder = NonLocalNet(in_dim=in_dim, num_layers=num_layers, num_channels=num_channels)
        self.classification = nn.Sequential(
            nn.Conv1d(num_channels, 32, kernel_size=1, bias=True), nn.ReLU(inplace=True),
            nn.Conv1d(32, 32, kernel_size=1, bias=True), nn.ReLU(inplace=True),
            nn.Conv1d(32, 1, kernel_size=1, bias=True),
        )
        for m in self.modules():  # the reference's initialisation (:115-121)
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                nn.init.xavier_normal_(m.weight, gain=1)
            elif isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    # False: ``encode`` and ``forward`` return M as a ``FeatureSimilarity`` (no
    # [B,N,N] tensor; SpectralMatchingLoss takes it on the fused kernel).  An
    # attribute, not a constructor argument: the constructor stays the reference's.
    dense_M = True

    def encode(self, corr_pos, compatibility, attention=nonlocal_attention, dense_M=None):
        """(corr_features [B,N,C], normed [B,N,C], logits [B,N], M [B,N,N]) of
        models/PointDSC.py:155-163 and :171 from torch ops, the attention through
        ``attention(q, k, v, compatibility)`` on [B,N,C] rows.  ``attention`` is
        the hook the CPU tests use (``composed_attention``); nothing else here
        needs a device.  ``dense_M`` (None: ``self.dense_M``) False leaves M as
        the ``FeatureSimilarity`` of normed and sigma."""
        enc = self.encoder
        feat = enc.layer0(corr_pos.permute(0, 2, 1))
        for i in range(enc.num_layers):
            feat = enc.blocks[f"PointCN_layer_{i}"](feat)
            blk = enc.blocks[f"NonLocal_layer_{i}"]
            q, k, v = (p(feat).transpose(1, 2) for p in (blk.projection_q, blk.projection_k, blk.projection_v))
            message = attention(q, k, v, compatibility).transpose(1, 2)
            feat = feat + blk.fc_message(message)
        features = feat.permute(0, 2, 1)
        normed = F.normalize(features, p=2, dim=-1)
        M = FeatureSimilarity(normed, self.sigma)
        if self.dense_M if dense_M is None else dense_M:
            M = M.dense()
        logits = self.classification(features.permute(0, 2, 1)).squeeze(1)
        return features, normed, logits, M

    @torch.no_grad()
    def seed_transform(self, normed, logits, src_keypts, tgt_keypts):
        """final_trans [B,4,4] of the training branch (:176, :182) on the stage
        kernels, in exact fp32: the int(N * ratio) largest logits as seeds, their
        k nearest neighbours in feature space, the NSM weights, one weighted
        Kabsch hypothesis per seed and the best of them by inlier count."""
        N = logits.shape[1]
        num_seeds = int(N * self.ratio)
        if num_seeds < 1:
            raise ValueError(f"int(N * ratio) = 0 seeds for N={N}, ratio={self.ratio}")
        seeds = torch.argsort(logits, dim=1, descending=True)[:, :num_seeds].to(torch.int32)
        normed = normed.detach().contiguous()
        knn = kernels.seed_knn(normed, seeds, min(self.k, N - 1), precision="f32")
        weights, _ = kernels.nsm_weights(normed, src_keypts, tgt_keypts, knn, self.num_iterations,
                                         self.sigma.detach(), self.sigma_spat.detach(), precision="f32")
        return kernels.seed_hypotheses(src_keypts, tgt_keypts, knn, weights, self.inlier_threshold)[3]

    def inference_model(self, precision="h3"):
        """An eval-mode ``PointDSC`` with this module's hyper-parameters and its
        current weights (copied: later optimizer steps do not reach it)."""
        key = ("_inference", precision)
        m = self.__dict__.get(key)
        if m is None:
            m = self.__dict__[key] = PointDSC(
                in_dim=self.in_dim, num_layers=self.num_layers, num_channels=self.num_channels,
                num_iterations=self.num_iterations, ratio=self.ratio, inlier_threshold=self.inlier_threshold,
                sigma_d=float(self.sigma_spat.detach().cpu()), k=self.k, nms_radius=self.nms_radius,
                precision=precision)
        m.load_state_dict(self.state_dict(), strict=True)
        return m.to(self.sigma.device).eval()

    def forward(self, data):
        corr_pos, src, tgt = data["corr_pos"], data["src_keypts"], data["tgt_keypts"]
        if "testing" in data.keys():
            return self.inference_model()(data)
        corr_pos, src, tgt = (kernels._dev(corr_pos, "corr_pos"), kernels._dev(src, "src_keypts"),
                              kernels._dev(tgt, "tgt_keypts"))
        with torch.no_grad():
            compatibility = kernels.compat(src, tgt, self.sigma_spat)
        _, normed, logits, M = self.encode(corr_pos, compatibility)
        final_trans = self.seed_transform(normed, logits.detach(), src, tgt)
        return {"final_trans": final_trans.detach(), "final_labels": logits, "M": M}


def _mean64(x):
    """mean(x) summed in fp64 and returned as an fp64 scalar (autograd casts the
    gradient back): the loss is then as exact as its fp32 terms, not one more fp32
    reduction away -- pdsc_spectral_matching_loss sums in fp64 for the same reason."""
    return x.double().mean()


class ClassificationLoss(nn.Module):
    """libs/loss.py:66-112 in torch ops: BCE on the logits -- weighted by
    ``weight``, plain mean (``balanced=False``) or with pos_weight = #neg / #pos
    -- and the statistics dict, whose precision / recall / f1 are those of the
    batch's first pair as in the reference (sklearn's binary scores restated: 0
    where the denominator is 0).  The loss is an fp64 scalar (``_mean64``)."""

    def __init__(self, balanced=True):
        super().__init__()
        self.balanced = balanced

    def forward(self, pred, gt, weight=None):
        gt = gt.to(pred.dtype)
        num_pos = torch.relu(torch.sum(gt) - 1) + 1
        num_neg = torch.relu(torch.sum(1 - gt) - 1) + 1
        if weight is not None:
            loss = _mean64(F.binary_cross_entropy_with_logits(pred, gt, reduction="none") * weight)
        elif self.balanced is False:
            loss = _mean64(F.binary_cross_entropy_with_logits(pred, gt, reduction="none"))
        else:
            loss = _mean64(F.binary_cross_entropy_with_logits(pred, gt, pos_weight=num_neg * 1.0 / num_pos,
                                                              reduction="none"))
        with torch.no_grad():
            p, g = pred.detach(), gt.detach()
            lab0, g0 = (p[0] > 0).to(p.dtype), g[0]
            tp = float((lab0 * g0).sum())
            n_pred, n_true = float(lab0.sum()), float(g0.sum())
            precision = tp / n_pred if n_pred > 0 else 0.0
            recall = tp / n_true if n_true > 0 else 0.0
            f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
            logit_true = float((p * g).sum()) / max(1.0, float(g.sum()))
            logit_false = float((p * (1 - g)).sum()) / max(1.0, float((1 - g).sum()))
        return {"loss": loss, "precision": precision, "recall": recall, "f1": f1,
                "logit_true": logit_true, "logit_false": logit_false}


class SpectralMatchingLoss(nn.Module):
    """libs/loss.py:115-139 in torch ops: gt_ij = (l_i + l_j == 2) with a zero
    diagonal; balanced: mean over pairs of half the positives' mean (M - 1)^2 plus
    half the negatives' mean M^2; else mean((M - gt)^2).  Sums in fp64; an fp64 scalar.
    M is a [B,N,N] tensor or a ``FeatureSimilarity``: the latter goes to the fused
    kernel on a device (loss alone when nothing requires a gradient or under
    ``no_grad``) and through ``dense()`` and the same ops on the CPU."""

    def __init__(self, balanced=True):
        super().__init__()
        self.balanced = balanced

    def forward(self, M, gt_labels):
        if isinstance(M, FeatureSimilarity):
            if M.normed.is_cuda:
                grads = torch.is_grad_enabled() and (M.normed.requires_grad or M.sigma.requires_grad)
                return _FusedSpectralMatchingLoss.apply(M.normed, M.sigma, gt_labels, self.balanced, grads)
            M = M.dense()
        gt_labels = gt_labels.to(M.dtype)
        gt_M = ((gt_labels[:, None, :] + gt_labels[:, :, None]) == 2).to(M.dtype)
        gt_M = gt_M * (1 - torch.eye(M.shape[1], dtype=M.dtype, device=M.device))
        if self.balanced:
            gt64 = gt_M.double()
            sm_p = ((M - 1) ** 2 * gt_M).double().sum((-1, -2)) / (torch.relu(gt64.sum((-1, -2)) - 1.0) + 1.0)
            sm_n = (M ** 2 * (1 - gt_M)).double().sum((-1, -2)) / (torch.relu((1 - gt64).sum((-1, -2)) - 1.0) + 1.0)
            return torch.mean(sm_p * 0.5 + sm_n * 0.5)
        return _mean64((M - gt_M) ** 2)


class TransformationLoss(nn.Module):
    """libs/loss.py:12-63: (loss, recall %, RE deg, TE cm, RMSE), batch means.
    The loss value is returned DETACHED: ``final_trans`` comes from the stage
    kernels without a graph, and the gradient through the Kabsch SVD is out of
    scope (the reference's default ``weight_transformation`` is 0, so its
    training never uses it).  As in the reference, each pair's warped source is
    compared against the whole batch's ``tgt_keypts`` (:47, :61 broadcast)."""

    def __init__(self, re_thre=15, te_thre=30):
        super().__init__()
        self.re_thre = re_thre
        self.te_thre = te_thre

    @torch.no_grad()
    def forward(self, trans, gt_trans, src_keypts, tgt_keypts, probs):
        bs = trans.shape[0]
        R, t = trans[:, :3, :3], trans[:, :3, 3]
        gt_R, gt_t = gt_trans[:, :3, :3], gt_trans[:, :3, 3]
        recall = 0
        RE, TE, RMSE, loss = (torch.zeros((), dtype=trans.dtype, device=trans.device) for _ in range(4))
        for i in range(bs):
            re = torch.acos(torch.clamp((torch.trace(R[i].T @ gt_R[i]) - 1) / 2.0, min=-1, max=1)) * 180 / math.pi
            te = torch.sqrt(torch.sum((t[i] - gt_t[i]) ** 2)) * 100
            warped = src_keypts[i] @ R[i].T + t[i]
            if te < self.te_thre and re < self.re_thre:
                recall += 1
            RE += re
            TE += te
            RMSE += torch.norm(warped - tgt_keypts, dim=-1).mean()
            if int((probs[i] > 0).sum()) >= 1:
                loss += ((warped - tgt_keypts) ** 2).sum(-1).mean()
        return loss / bs, recall * 100.0 / bs, RE / bs, TE / bs, RMSE / bs
