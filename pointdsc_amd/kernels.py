"""torch-facing wrappers of the libpdsc C ABI (one function per hot-path op).

Tensors must live on a HIP device (``torch.device('cuda')`` on ROCm); every
call runs the hand-written gfx950 kernels on torch's current stream.  There is
no CPU or eager-PyTorch fallback: a CPU tensor or a missing library raises.
Index outputs are int32 (the C ABI's index type).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._call import _p, _stream, _workspace, call, query, read_struct, struct_buffer, trans_view  # noqa: F401
from ._lib import check

CH = 128


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the pointdsc_amd HIP path needs device tensors "
                           "(there is no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


# --------------------------------------------------------------------- a1
def compat(src: torch.Tensor, tgt: torch.Tensor, sigma_d: torch.Tensor) -> torch.Tensor:
    """M [B,N,N] (models/PointDSC.py:150-153).  src/tgt [B,N,3]; sigma_d: device scalar tensor."""
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    sigma_d = _dev(sigma_d.reshape(-1), "sigma_d")
    B, N, _ = src.shape
    M = torch.empty((B, N, N), dtype=torch.float32, device=src.device)
    call("pdsc_compat_f32", src, tgt, B, N, sigma_d, M, device=src.device)
    return M


def compat_packed(src: torch.Tensor, tgt: torch.Tensor, sigma_d: torch.Tensor) -> torch.Tensor:
    """The forward's symmetric-packed M (include/pdsc.h: pdsc_compat_packed_f32),
    unpacked to dense [B,N,N] on the device for inspection."""
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    sigma_d = _dev(sigma_d.reshape(-1), "sigma_d")
    B, N, _ = src.shape
    Mp = torch.empty((B, query("pdsc_compat_packed_floats", N)), dtype=torch.float32, device=src.device)
    call("pdsc_compat_packed_f32", src, tgt, B, N, sigma_d, Mp, device=src.device)
    T = 32
    nt = (N + T - 1) // T
    ti, tj = torch.triu_indices(nt, nt)
    tiles = Mp.view(B, -1, T, T)  # upper-triangle tiles in row-major (ti, tj) order
    full = torch.zeros((B, nt, nt, T, T), dtype=torch.float32, device=src.device)
    full[:, ti, tj] = tiles
    full[:, tj, ti] = tiles.transpose(-1, -2)
    return full.permute(0, 1, 3, 2, 4).reshape(B, nt * T, nt * T)[:, :N, :N].contiguous()


# ------------------------------------------------------------------ weights
def pack_weights(cfg: _lib.PdscConfig, named: dict) -> torch.Tensor:
    """Pack reference state-dict tensors (on device) into the kernels' blob."""
    L = _lib.load()
    n = L.pdsc_param_count(cfg)
    tensors, ptrs = [], (ctypes.c_void_p * n)()
    device = None
    for i in range(n):
        key = L.pdsc_param_name(cfg, i).decode()
        if key not in named:
            raise KeyError(f"missing parameter {key}")
        t = _dev(named[key].detach(), key)
        device = t.device
        tensors.append(t)
        ptrs[i] = t.data_ptr()
    packed = torch.empty(L.pdsc_packed_weights_floats(cfg), dtype=torch.float32, device=device)
    call("pdsc_pack_weights", cfg, ptrs, packed, device=device)
    torch.cuda.current_stream(device).synchronize()  # keep `tensors` alive until the copies ran
    return packed


# ------------------------------------------------------------------- a2-a4
def encoder(cfg, packed, corr_pos, M, want_features=True):
    """(corr_features [B,N,C] | None, normed [B,N,C], confidence [B,N])."""
    corr_pos, M = _dev(corr_pos, "corr_pos"), _dev(M, "M")
    B, N, _ = corr_pos.shape
    dev = corr_pos.device
    feat = torch.empty((B, N, CH), dtype=torch.float32, device=dev) if want_features else None
    normed = torch.empty((B, N, CH), dtype=torch.float32, device=dev)
    conf = torch.empty((B, N), dtype=torch.float32, device=dev)
    call("pdsc_encoder_f32", cfg, packed, corr_pos, M, B, N, feat, normed, conf, device=dev,
         ws=("pdsc_encoder_workspace_bytes", cfg, B, N))
    return feat, normed, conf


def attention(q, k, v, M, precision="h3"):
    """softmax_j(M_ij q_i.k_j / sqrt(C)) v_j  (models/PointDSC.py:36-42); q,k,v [B,N,128]."""
    q, k, v, M = (_dev(t, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (M, "M")))
    B, N, C = q.shape
    if k.shape != q.shape or v.shape != q.shape or M.shape != (B, N, N):
        raise ValueError(f"q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} M {tuple(M.shape)}")
    pc = _lib.precision_code(precision)
    msg = torch.empty_like(q)
    call("pdsc_attention_f32", q, k, v, M, B, N, C, pc, msg, device=q.device,
         ws=("pdsc_attention_workspace_bytes", B, N, C, pc))
    return msg


def _attention_args(q, k, v, M):
    q, k, v, M = (_dev(t, n) for t, n in ((q, "q"), (k, "k"), (v, "v"), (M, "M")))
    B, N, C = q.shape
    if k.shape != q.shape or v.shape != q.shape or M.shape != (B, N, N):
        raise ValueError(f"q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} M {tuple(M.shape)}")
    return q, k, v, M, B, N, C


def attention_lse(q, k, v, M):
    """(msg [B,N,128], lse [B,N]): ``attention(..., precision='f32')`` bit for bit, and
    the row log-sum-exp of the logits M_ij q_i.k_j / sqrt(C) its backward needs."""
    q, k, v, M, B, N, C = _attention_args(q, k, v, M)
    msg = torch.empty_like(q)
    lse = torch.empty((B, N), dtype=torch.float32, device=q.device)
    call("pdsc_attention_lse_f32", q, k, v, M, B, N, C, msg, lse, device=q.device,
         ws=("pdsc_attention_lse_workspace_bytes", B, N, C))
    return msg, lse


def attention_backward(q, k, v, M, msg, lse, dmsg):
    """(dq, dk, dv) [B,N,128] of ``attention_lse`` for the gradient dmsg of msg; the
    softmax is recomputed from lse, not stored (include/pdsc.h).  M gets no gradient."""
    q, k, v, M, B, N, C = _attention_args(q, k, v, M)
    msg, lse, dmsg = _dev(msg, "msg"), _dev(lse, "lse"), _dev(dmsg, "dmsg")
    if msg.shape != q.shape or dmsg.shape != q.shape or lse.shape != (B, N):
        raise ValueError(f"msg {tuple(msg.shape)} dmsg {tuple(dmsg.shape)} lse {tuple(lse.shape)} for q {tuple(q.shape)}")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    call("pdsc_attention_backward_f32", q, k, v, M, msg, lse, dmsg, B, N, C, dq, dk, dv, device=q.device,
         ws=("pdsc_attention_backward_workspace_bytes", B, N, C))
    return dq, dk, dv


def sm_loss_fused(normed, sigma, gt_labels, balanced=True, grads=True):
    """``(loss, dnormed | None, dsigma | None)``: SpectralMatchingLoss of the clamped
    feature similarity of normed [B,N,128] (unit rows) and the device scalar sigma
    against gt_labels [B,N], and d loss / d normed [B,N,128] fp32 and d loss / d sigma
    (fp64 scalars, like the loss) from the same pass; no [B,N,N] tensor is made
    (include/pdsc.h).  grads=False computes the loss alone."""
    normed, gt = _dev(normed, "normed"), _dev(gt_labels, "gt_labels")
    sigma = _dev(sigma.reshape(-1), "sigma")
    if normed.dim() != 3 or gt.shape != normed.shape[:2] or sigma.numel() != 1:
        raise ValueError(f"normed {tuple(normed.shape)} must be [B,N,C], gt_labels {tuple(gt.shape)} [B,N] and "
                         f"sigma ({sigma.numel()} elements) a scalar")
    B, N, C = normed.shape
    dev = normed.device
    loss = torch.empty((), dtype=torch.float64, device=dev)
    dnormed = torch.empty_like(normed) if grads else None
    dsigma = torch.empty((), dtype=torch.float64, device=dev) if grads else None
    call("pdsc_sm_loss_fused_f32", normed, sigma, gt, B, N, C, int(bool(balanced)), loss, dnormed, dsigma, device=dev,
         ws=("pdsc_sm_loss_fused_workspace_bytes", B, N, C))
    return loss, dnormed, dsigma


# ---------------------------------------------------------------------- a5
def pick_seeds(src, conf, radius: float, max_num: int):
    """(seeds int32 [B,S], is_local_max [B,N]) (models/PointDSC.py:199-217)."""
    src, conf = _dev(src, "src"), _dev(conf, "conf")
    B, N = conf.shape
    seeds = torch.empty((B, max_num), dtype=torch.int32, device=src.device)
    lm = torch.empty((B, N), dtype=torch.float32, device=src.device)
    call("pdsc_pick_seeds", src, conf, B, N, float(radius), int(max_num), seeds, lm, device=src.device)
    return seeds, lm


# ---------------------------------------------------------------------- a6
def seed_knn(normed, seeds, k: int, precision="h3"):
    """knn indices [B,S,k] int32 of the seed rows (models/common.py:48-69)."""
    normed, seeds = _dev(normed, "normed"), _dev(seeds, "seeds", torch.int32)
    B, N, C = normed.shape
    S = seeds.shape[1]
    out = torch.empty((B, S, k), dtype=torch.int32, device=normed.device)
    call("pdsc_seed_knn", normed, seeds, B, N, C, S, int(k), _lib.precision_code(precision), out,
         device=normed.device, ws=("pdsc_seed_knn_workspace_bytes", B, N, S))
    return out


# ------------------------------------------------------------------- a7-a8
def nsm_weights(normed, src, tgt, knn, num_iterations, sigma, sigma_d, precision="h3"):
    """(weights [B,S,k], iterations used [B]) (models/PointDSC.py:257-282, :338-358)."""
    normed, src, tgt = _dev(normed, "normed"), _dev(src, "src"), _dev(tgt, "tgt")
    knn = _dev(knn, "knn", torch.int32)
    sigma, sigma_d = _dev(sigma.reshape(-1), "sigma"), _dev(sigma_d.reshape(-1), "sigma_d")
    B, N, C = normed.shape
    _, S, k = knn.shape
    w = torch.empty((B, S, k), dtype=torch.float32, device=normed.device)
    it = torch.empty((B,), dtype=torch.int32, device=normed.device)
    call("pdsc_nsm_weights", normed, src, tgt, knn, B, N, C, S, k, int(num_iterations),
         _lib.precision_code(precision), sigma, sigma_d, w, it, device=normed.device,
         ws=("pdsc_nsm_workspace_bytes", B, N, S, k, int(num_iterations)))
    return w, it


# ---------------------------------------------------------------------- a9
def rigid_transform_3d(A, B, weights=None):
    """[nb,4,4] weighted Kabsch (models/common.py:7-45); A,B [nb,n,3], weights [nb,n]."""
    A, B = _dev(A, "A"), _dev(B, "B")
    w = _dev(weights, "weights") if weights is not None else None
    nb, n, _ = A.shape
    out = torch.empty((nb, 4, 4), dtype=torch.float32, device=A.device)
    call("pdsc_rigid_transform_3d", A, B, w, nb, n, out, device=A.device)
    return out


# --------------------------------------------------------------------- a10
def seed_hypotheses(src, tgt, knn, weights, tau: float):
    """(seed_trans [B,S,4,4], fitness [B,S], best [B], trans [B,4,4], labels [B,N])."""
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    knn, weights = _dev(knn, "knn", torch.int32), _dev(weights, "weights")
    B, N, _ = src.shape
    _, S, k = knn.shape
    dev = src.device
    seed_trans = torch.empty((B, S, 4, 4), dtype=torch.float32, device=dev)
    fitness = torch.empty((B, S), dtype=torch.float32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    trans = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty((B, N), dtype=torch.float32, device=dev)
    call("pdsc_seed_hypotheses", src, tgt, knn, weights, B, N, S, k, float(tau), seed_trans, fitness, best, trans,
         labels, device=dev, ws=("pdsc_seed_hypotheses_workspace_bytes", B, S))
    return seed_trans, fitness, best, trans, labels


# --------------------------------------------------------------------- a11
def post_refine(trans, src, tgt, thr: float):
    """Refined [B,4,4] (models/PointDSC.py:403-438); `trans` is not modified."""
    out = _dev(trans, "trans").clone()
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    B, N, _ = src.shape
    call("pdsc_post_refine", out, src, tgt, B, N, float(thr), device=src.device)
    return out


# ----------------------------------------------------------------- forward
PDSC_ERR_RANGE = 4


class RangeError(RuntimeError):
    """PDSC_ERR_RANGE (include/pdsc.h, fp16 range guard): pairs whose activations
    left fp16's range under PDSC_PRECISION_H3 (or, in either precision, whose
    logits are non-finite).  ``pairs``: their indices in the call; ``outputs``:
    the call's return value, valid for every other pair (the marked pairs'
    final_trans are NaN, their final_labels 0)."""

    def __init__(self, pairs, outputs):
        super().__init__(f"pairs {pairs} left the fp16 range of the 3xfp16 contractions "
                         f"(rerun them with precision='f32')")
        self.pairs, self.outputs = list(pairs), outputs


def range_flags(ws, B, device):
    """The forward's per-pair range marks from its workspace (pdsc_range_status;
    synchronises the device's current stream): a list of marked pair indices."""
    flags = (ctypes.c_int32 * B)()
    st = _lib.load().pdsc_range_status(_p(ws), B, flags, _stream(device))
    if st not in (0, PDSC_ERR_RANGE):
        check(st, "pdsc_range_status")
    return [b for b in range(B) if flags[b]]


def _range_check(ws, B, device, outputs):
    bad = range_flags(ws, B, device)
    if bad:
        raise RangeError(bad, outputs)
    return outputs


def _check_inputs(cfg, corr_pos, src, tgt):
    """Shapes the forward kernels assume (the reference's Conv1d(in_dim) raises on a wrong width)."""
    if src.dim() != 3 or src.shape[2] != 3 or tgt.shape != src.shape or corr_pos.dim() != 3 \
            or corr_pos.shape[:2] != src.shape[:2] or corr_pos.shape[2] != cfg.in_dim:
        raise ValueError(f"shape mismatch: corr_pos {tuple(corr_pos.shape)} (expected [B,N,{cfg.in_dim}]), "
                         f"src {tuple(src.shape)}, tgt {tuple(tgt.shape)} (expected [B,N,3])")


def _forward_bytes(cfg, B, N, size_query="pdsc_forward_workspace_bytes"):
    """The forward's workspace size for (cfg, B, N); 0 means unsupported: raises with pdsc_last_error."""
    return query(size_query, cfg, B, N, required=True)


def _forward_setup(cfg, corr_pos, src, tgt, size_query="pdsc_forward_workspace_bytes", ws=None):
    """What every forward entry point starts with: the inputs as contiguous fp32
    device tensors, their shape check and the workspace -- the caller-kept ``ws``
    if it is large enough and on the inputs' device, else a fresh one.  Returns
    (corr_pos, src, tgt, B, N, device, (workspace, its size query's bytes))."""
    corr_pos, src, tgt = _dev(corr_pos, "corr_pos"), _dev(src, "src_keypts"), _dev(tgt, "tgt_keypts")
    B, N, _ = src.shape
    _check_inputs(cfg, corr_pos, src, tgt)
    dev = src.device
    nb = _forward_bytes(cfg, B, N, size_query)
    if ws is None or ws.numel() < nb or ws.device != dev:
        ws = _workspace(nb, dev)
    return corr_pos, src, tgt, B, N, dev, (ws, nb)


def _stage_outputs(cfg, B, N, dev):
    """The five stage tensors of pdsc_forward_debug and the struct that points at them."""
    S, k = int(N * cfg.ratio), min(cfg.k, N - 1)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    st = {"conf": torch.empty((B, N), **f32), "seeds": torch.empty((B, S), **i32),
          "knn": torch.empty((B, S, k), **i32), "weights": torch.empty((B, S, k), **f32),
          "trans_pre_refine": torch.empty((B, 4, 4), **f32)}
    return st, _lib.PdscForwardDebug(*(st[n].data_ptr() for n in ("conf", "seeds", "knn", "weights",
                                                                   "trans_pre_refine")))


def forward_testing(cfg, packed, corr_pos, src, tgt, debug=False, check_range=True, ws=None):
    """Full testing forward for B pairs: (final_trans [B,4,4], final_labels [B,N])
    (+ (confidence [B,N], seeds [B,S]) when ``debug``).  check_range: read the
    fp16 range guard's marks (synchronises the stream) and raise RangeError if
    any; with check_range=False the call stays asynchronous and the caller reads
    the marks itself (``range_flags(ws, B, device)``) before trusting a pose.
    ws: a caller-kept uint8 device workspace of at least
    pdsc_forward_workspace_bytes (else one is allocated per call)."""
    corr_pos, src, tgt, B, N, dev, ws = _forward_setup(cfg, corr_pos, src, tgt, ws=ws)
    trans = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty((B, N), dtype=torch.float32, device=dev)
    conf = seeds = None
    if debug:
        conf = torch.empty((B, N), dtype=torch.float32, device=dev)
        seeds = torch.empty((B, int(N * cfg.ratio)), dtype=torch.int32, device=dev)
    call("pdsc_forward_testing", cfg, packed, corr_pos, src, tgt, B, N, trans, labels, conf, seeds, device=dev, ws=ws)
    out = (trans, labels, conf, seeds) if debug else (trans, labels)
    return _range_check(ws[0], B, dev, out) if check_range else out


def forward_stages(cfg, packed, corr_pos, src, tgt, check_range=True):
    """The full testing forward for B pairs with every stage's output
    (pdsc_forward_testing_debug): dict of final_trans [B,4,4], final_labels
    [B,N], conf [B,N], seeds [B,S], knn [B,S,k], weights [B,S,k],
    trans_pre_refine [B,4,4] (int32 indices)."""
    corr_pos, src, tgt, B, N, dev, ws = _forward_setup(cfg, corr_pos, src, tgt)
    st, dbg = _stage_outputs(cfg, B, N, dev)
    out = {"final_trans": torch.empty((B, 4, 4), dtype=torch.float32, device=dev),
           "final_labels": torch.empty((B, N), dtype=torch.float32, device=dev), **st}
    call("pdsc_forward_testing_debug", cfg, packed, corr_pos, src, tgt, B, N, out["final_trans"], out["final_labels"],
         dbg, device=dev, ws=ws)
    return _range_check(ws[0], B, dev, out) if check_range else out


def forward_ragged(cfg, packed, corr_pos, src, tgt, counts, debug=False, check_range=True):
    """B pairs of different sizes in one call (pdsc_forward_testing_ragged): pair
    b occupies the first counts[b] rows of the padded [B,N,.] inputs.  Returns
    (final_trans [B,4,4], final_labels [B,N], rows past counts[b] zero); with
    ``debug``, also the dict of stage outputs (conf, seeds, knn, weights,
    trans_pre_refine) at the batch's strides."""
    corr_pos, src, tgt, B, N, dev, ws = _forward_setup(cfg, corr_pos, src, tgt)
    counts = [int(c) for c in counts]
    if len(counts) != B:
        raise ValueError(f"{len(counts)} counts for {B} pairs")
    trans = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty((B, N), dtype=torch.float32, device=dev)
    st, dbg = _stage_outputs(cfg, B, N, dev) if debug else (None, None)
    call("pdsc_forward_testing_ragged", cfg, packed, corr_pos, src, tgt, B, N, (ctypes.c_int32 * B)(*counts), trans,
         labels, dbg, device=dev, ws=ws)
    out = (trans, labels, st) if debug else (trans, labels)
    return _range_check(ws[0], B, dev, out) if check_range else out


def pad_pairs(tensors, N=None):
    """Stack [n_b, C] (or [1, n_b, C]) tensors into a zero-padded [B, N, C] batch
    (N = the largest n_b by default); returns (batch, counts)."""
    ts = [t[0] if t.dim() == 3 else t for t in tensors]
    counts = [int(t.shape[0]) for t in ts]
    N = max(counts) if N is None else int(N)
    out = torch.zeros((len(ts), N, ts[0].shape[1]), dtype=ts[0].dtype, device=ts[0].device)
    for b, t in enumerate(ts):
        out[b, :t.shape[0]] = t
    return out, counts


def forward_training(cfg, packed, corr_pos, src, tgt, want_M=True, want_seeds=False, check_range=True):
    """Training-mode forward (models/PointDSC.py:158-163, :176, :182, :189-191) for
    B pairs: (final_trans [B,4,4], confidence [B,N], M [B,N,N] | None,
    seeds [B,S] | None).  Forward only: no gradients flow through the HIP path."""
    corr_pos, src, tgt, B, N, dev, ws = _forward_setup(cfg, corr_pos, src, tgt,
                                                       "pdsc_forward_training_workspace_bytes")
    trans = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((B, N), dtype=torch.float32, device=dev)
    M = torch.empty((B, N, N), dtype=torch.float32, device=dev) if want_M else None
    seeds = torch.empty((B, int(N * cfg.ratio)), dtype=torch.int32, device=dev) if want_seeds else None
    call("pdsc_forward_training", cfg, packed, corr_pos, src, tgt, B, N, trans, conf, M, seeds, device=dev, ws=ws)
    out = (trans, conf, M, seeds)
    return _range_check(ws[0], B, dev, out) if check_range else out


def spectral_matching_loss(M, gt_labels, balanced=True):
    """SpectralMatchingLoss (libs/loss.py:115-139) forward: a device scalar tensor."""
    M, gt = _dev(M, "M"), _dev(gt_labels, "gt_labels")
    if M.dim() != 3 or M.shape[1] != M.shape[2] or gt.shape != M.shape[:2]:
        raise ValueError(f"M {tuple(M.shape)} must be [B,N,N] and gt_labels {tuple(gt.shape)} [B,N]")
    B, N = gt.shape
    loss = torch.empty((), dtype=torch.float32, device=M.device)
    call("pdsc_spectral_matching_loss", M, gt, B, N, int(bool(balanced)), loss, device=M.device,
         ws=("pdsc_spectral_matching_loss_workspace_bytes", B, N))
    return loss


# --------------------------------------------------------------------- f8
def consistency_graph(corr_pos, threshold: float, mode: str = "squared"):
    """The PMC baseline's graph (include/pdsc.h f8, baseline_3DMatch.py:60-68):
    ``(adj int64 [N, ceil(N/64)], degree int32 [N])`` for corr_pos [N,6]; bit
    j % 64 of word j // 64 of row i is set iff i != j and the pair is
    consistent.  mode 'squared' is the reference as written, 'length' the
    difference of the lengths themselves."""
    corr_pos = _dev(corr_pos, "corr_pos")
    if corr_pos.dim() != 2 or corr_pos.shape[1] != 6:
        raise ValueError(f"corr_pos {tuple(corr_pos.shape)} must be [N,6]")
    if mode not in _lib.EDGE_MODES:
        raise ValueError(f"mode must be one of {sorted(_lib.EDGE_MODES)}, got {mode!r}")
    N, dev = corr_pos.shape[0], corr_pos.device
    adj = torch.empty((N, (N + 63) // 64), dtype=torch.int64, device=dev)
    degree = torch.empty(N, dtype=torch.int32, device=dev)
    call("pdsc_consistency_graph", corr_pos, N, float(threshold), _lib.EDGE_MODES[mode], adj, degree, device=dev)
    return adj, degree


class _Info:
    """The fields ``__slots__`` names of the struct ``_struct``, read back from its
    device tensor (one synchronising copy): ints for the C integers, floats for doubles."""
    __slots__ = ()
    _struct = None

    def __init__(self, result: torch.Tensor):
        r = read_struct(result, self._struct)
        for k in self.__slots__:
            setattr(self, k, getattr(r, k))

    def __repr__(self):
        return type(self).__name__ + "(" + ", ".join(f"{k}={getattr(self, k)}" for k in self.__slots__) + ")"


class CliqueInfo(_Info):
    """``pdsc_clique_result`` read back from the device (one synchronising copy)."""
    __slots__ = ("size", "exact", "heuristic_size", "roots_incomplete", "nodes")
    _struct = _lib.PdscCliqueResult


def max_clique(adj, node_budget: int = 0, heuristic_only: bool = False):
    """A maximum clique of the bitset graph adj int64 [N, ceil(N/64)] (include/pdsc.h
    f8): ``(members int32 [N], labels fp32 [N], result)`` -- members ascending
    and -1 past the size, result the device copy of ``pdsc_clique_result`` (an
    int32 [6] tensor; ``CliqueInfo(result)`` reads it).  node_budget: expanded
    nodes per root, 0 = the library default.  heuristic_only: the greedy lower
    bound alone (pdsc_greedy_clique)."""
    adj = _dev(adj, "adj", torch.int64)
    N = adj.shape[0]
    if adj.dim() != 2 or adj.shape[1] != (N + 63) // 64:
        raise ValueError(f"adj {tuple(adj.shape)} must be [N, ceil(N/64)]")
    dev = adj.device
    ws = ("pdsc_max_clique_workspace_bytes", N)
    members = torch.empty(N, dtype=torch.int32, device=dev)
    labels = torch.empty(N, dtype=torch.float32, device=dev)
    result = struct_buffer(_lib.PdscCliqueResult, dev).view(torch.int32)
    if heuristic_only:
        call("pdsc_greedy_clique", adj, N, members, result, labels, device=dev, ws=ws)
    else:
        call("pdsc_max_clique", adj, N, int(node_budget), members, result, labels, device=dev, ws=ws)
    return members, labels, result


# --------------------------------------------------------------------- f9
GNC_FACTOR, GNC_MAX_ITERATIONS, GNC_COST_THRESHOLD = 1.4, 10000, 1e-16  # TEASER_plus_plus.py:89-91


class GncInfo(_Info):
    """``pdsc_gnc_info`` read back from the device (one synchronising copy)."""
    __slots__ = ("iterations", "stop_reason", "cost", "mu")
    _struct = _lib.PdscGncInfo


class TeaserInfo(_Info):
    """``pdsc_teaser_result`` read back from the device (one synchronising copy)."""
    __slots__ = ("valid", "clique_size", "clique_exact", "roots_incomplete", "gnc_iterations", "n_rotation_inliers",
                 "n_translation_inliers")
    _struct = _lib.PdscTeaserResult


def _tims(a, b, na, nb):
    a, b = _dev(a, na, torch.float64), _dev(b, nb, torch.float64)
    if a.dim() != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"{na} {tuple(a.shape)} / {nb} {tuple(b.shape)} must both be [K,3]")
    return a, b


def gnc_tls_rotation(src_tims, dst_tims, noise_bound: float, gnc_factor: float = GNC_FACTOR,
                     max_iterations: int = GNC_MAX_ITERATIONS, cost_threshold: float = GNC_COST_THRESHOLD):
    """pdsc_gnc_tls_rotation (include/pdsc.h f9) on fp64 TIMs [K,3]: ``(R fp64
    [3,3], weights fp64 [K], inliers int32 [K], info)`` -- info the device copy of
    ``pdsc_gnc_info`` (a uint8 tensor of its size; ``GncInfo(info)`` reads it and
    synchronises)."""
    a, b = _tims(src_tims, dst_tims, "src_tims", "dst_tims")
    K, dev = a.shape[0], a.device
    R = torch.empty((3, 3), dtype=torch.float64, device=dev)
    w = torch.empty(K, dtype=torch.float64, device=dev)
    inl = torch.empty(K, dtype=torch.int32, device=dev)
    info = struct_buffer(_lib.PdscGncInfo, dev)
    call("pdsc_gnc_tls_rotation", a, b, K, float(noise_bound), float(gnc_factor), int(max_iterations),
         float(cost_threshold), R, w, inl, info, device=dev)
    return R, w, inl, info


def tls_translation(src, dst, noise_bound: float):
    """pdsc_tls_translation on fp64 points [K,3] (src already rotated):
    ``(t fp64 [3], inliers int32 [K])``."""
    a, b = _tims(src, dst, "src", "dst")
    K, dev = a.shape[0], a.device
    t = torch.empty(3, dtype=torch.float64, device=dev)
    inl = torch.empty(K, dtype=torch.int32, device=dev)
    call("pdsc_tls_translation", a, b, K, float(noise_bound), t, inl, device=dev,
         ws=("pdsc_tls_translation_workspace_bytes", K))
    return t, inl


def teaser_solve(src, tgt, noise_bound: float, node_budget: int = 0, gnc_factor: float = GNC_FACTOR,
                 max_iterations: int = GNC_MAX_ITERATIONS, cost_threshold: float = GNC_COST_THRESHOLD):
    """pdsc_teaser_solve on matched fp32 points src[i] <-> tgt[i] [N,3]: ``(trans
    fp64 [4,4], trans fp32 [4,4], labels fp32 [N], result)`` -- result the device
    copy of ``pdsc_teaser_result`` (a uint8 tensor of its size whose leading 16
    doubles are trans; ``TeaserInfo(result)`` reads the counters and synchronises)."""
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    if src.dim() != 2 or src.shape[1] != 3 or src.shape != tgt.shape:
        raise ValueError(f"src {tuple(src.shape)} / tgt {tuple(tgt.shape)} must both be [N,3]")
    N, dev = src.shape[0], src.device
    result = struct_buffer(_lib.PdscTeaserResult, dev)
    t32 = torch.empty((4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty(N, dtype=torch.float32, device=dev)
    call("pdsc_teaser_solve", src, tgt, N, float(noise_bound), float(gnc_factor), int(max_iterations),
         float(cost_threshold), int(node_budget), result, t32, labels, device=dev,
         ws=("pdsc_teaser_solve_workspace_bytes", N))
    return trans_view(result), t32, labels, result


class ForwardPlan:
    """Reusable workspace + outputs for repeated batched forwards of one (B, N).

    Avoids the per-call allocator round trip in throughput loops (bench.py)."""

    def __init__(self, cfg, packed, B, N, device):
        self.cfg, self.packed, self.B, self.N = cfg, packed, B, N
        self.nb = _forward_bytes(cfg, B, N)
        self.ws = _workspace(self.nb, device)
        self.trans = torch.empty((B, 4, 4), dtype=torch.float32, device=device)
        self.labels = torch.empty((B, N), dtype=torch.float32, device=device)

    def run(self, corr_pos, src, tgt, stream=None):
        if getattr(self, "graph", None) is not None:
            self.graph.replay()
            return self.trans, self.labels
        _check_inputs(self.cfg, corr_pos, src, tgt)
        if tuple(src.shape[:2]) != (self.B, self.N):
            raise ValueError(f"plan is for B={self.B} N={self.N}, got {tuple(src.shape[:2])}")
        call("pdsc_forward_testing", self.cfg, self.packed, corr_pos, src, tgt, self.B, self.N, self.trans,
             self.labels, None, None, device=src.device, ws=(self.ws, self.nb), stream=stream)
        return self.trans, self.labels

    def range_flags(self):
        """The last forward's fp16 range marks (pdsc_range_status; synchronises)."""
        return range_flags(self.ws, self.B, self.ws.device)

    def capture(self, corr_pos, src, tgt):
        """Record one forward over these (resident) inputs into a HIP graph;
        later run() calls replay it (one launch instead of ~40), reading
        whatever the same input buffers hold at replay time."""
        self.run(corr_pos, src, tgt)  # warm (first-touch) outside the capture
        torch.cuda.synchronize(src.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.run(corr_pos, src, tgt)
        self.graph = g
        return self
