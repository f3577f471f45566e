"""The training attention (include/pdsc.h: pdsc_attention_lse_f32,
pdsc_attention_backward_f32; pointdsc_amd.training.nonlocal_attention) against
this file's restatement of its math in torch on the CPU:

    S = q k^T / sqrt(128), X = M S, L = logsumexp_j X, P = exp(X - L), msg = P v

with autograd for (dq, dk, dv) of sum(msg * dmsg).  Reference: the restatement in
fp64 on the same fp32 inputs.  Yardstick: the restatement in fp32.  For each x
of msg, lse, dq, dk, dv with e(x) = max|x - x64| / max|x64|:

    e(hip) <= 4 e(torch32)

(both are fp32 sums of the same lengths in other orders, and the kernels' exp
adds about an ulp; a dropped D_i, a missing M_ij or a missing 1/sqrt(128) is off
by orders of magnitude).

Where x64 is identically zero the ratio is undefined.  That happens at N = 1: P
= 1, so dP - D = dmsg.v - dmsg.msg cancels exactly and dq = dk = 0.  The kernels
form the two dot products in different orders (an MFMA chain, a wavefront sum),
so they cancel to rounding only: each is a length-128 fp32 dot product, off by
at most 128 eps sum_c|dmsg_c v_c|, and dq, dk scale the difference by at most
N max|M| max(|q|, |k|) / sqrt(128).  That product is the bar there."""
import ctypes
import math

import numpy as np
import pytest
import torch

from pointdsc_amd.synthetic import synthetic_pair

pytestmark = pytest.mark.gpu

C = 128
SHAPES = [(1, 1), (1, 7), (2, 33), (1, 95), (3, 130), (1, 257), (2, 300)]
NAMES = ("msg", "lse", "dq", "dk", "dv")
EPS = float(np.finfo(np.float32).eps)
_REF = {}


def _inputs(B, N, seed=0):
    """q, k, v, dmsg ~ N(0,1) (CPU fp32) and the pairs' points for kernels.compat."""
    gen = torch.Generator().manual_seed(1000 * N + B + seed)
    q, k, v, dmsg = (torch.randn(B, N, C, generator=gen) for _ in range(4))
    pairs = [synthetic_pair(N, 77 + b + seed, "3dmatch", 0.4) for b in range(B)]
    src = torch.from_numpy(np.stack([p["src_keypts"] for p in pairs]))
    tgt = torch.from_numpy(np.stack([p["tgt_keypts"] for p in pairs]))
    return q, k, v, dmsg, src, tgt


def _compat(src, tgt, dev):
    from pointdsc_amd import kernels
    return kernels.compat(src.to(dev), tgt.to(dev), torch.tensor([0.1], device=dev))


def restate(q, k, v, M, dmsg, dtype):
    q, k, v = (t.detach().to(dtype).requires_grad_() for t in (q, k, v))
    X = M.to(dtype) * (torch.matmul(q, k.transpose(1, 2)) / math.sqrt(C))
    lse = torch.logsumexp(X, dim=-1)
    msg = torch.matmul(torch.exp(X - lse[..., None]), v)
    (msg * dmsg.to(dtype)).sum().backward()
    return dict(msg=msg.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def _hip(q, k, v, M, dmsg, dev):
    from pointdsc_amd import kernels
    q, k, v, dmsg = (t.to(dev) for t in (q, k, v, dmsg))
    msg, lse = kernels.attention_lse(q, k, v, M)
    dq, dk, dv = kernels.attention_backward(q, k, v, M, msg, lse, dmsg)
    return dict(msg=msg, lse=lse, dq=dq, dk=dk, dv=dv)


def _hold(got, q, k, v, M, dmsg, what=""):
    """got (device or CPU tensors by name) against the fp64 restatement within 4 x the fp32 restatement's error."""
    r64, r32 = restate(q, k, v, M, dmsg, torch.float64), restate(q, k, v, M, dmsg, torch.float32)
    bad = []
    for n in NAMES:
        x64 = r64[n]
        scale = x64.abs().max().item()
        eh = (got[n].detach().cpu().double() - x64).abs().max().item()
        et = (r32[n].double() - x64).abs().max().item()
        if scale > 0:
            eh, et, bar = eh / scale, et / scale, 4 * et / scale
        else:  # identically zero in exact arithmetic: the cancellation bound of the docstring
            dots = torch.matmul(dmsg.abs().double(), v.abs().double().transpose(1, 2)).max().item()
            bar = 2 * C * EPS * dots * q.shape[1] * M.abs().max().item() * max(q.abs().max().item(),
                                                                                 k.abs().max().item()) / math.sqrt(C)
        line = f"{what}{n}: e(hip) = {eh:.3e}, e(torch32) = {et:.3e}, bar {bar:.3e}"
        print(line)
        if not eh <= bar:
            bad.append(line)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,N", SHAPES)
def test_forward_backward_against_fp64(B, N):
    dev = torch.device("cuda")
    q, k, v, dmsg, src, tgt = _inputs(B, N)
    M = _compat(src, tgt, dev)
    _hold(_hip(q, k, v, M, dmsg, dev), q, k, v, M.cpu(), dmsg, f"({B},{N}) ")


def _case130(dev):
    q, k, v, dmsg, src, tgt = _inputs(2, 130, seed=5)
    return q, k, v, dmsg, _compat(src, tgt, dev)


def test_zero_rows_of_M_have_uniform_softmax():
    dev = torch.device("cuda")
    q, k, v, dmsg, M = _case130(dev)
    dead = [0, 64, 129]
    M[:, dead, :] = 0
    M[:, :, dead] = 0
    got = _hip(q, k, v, M, dmsg, dev)
    _hold(got, q, k, v, M.cpu(), dmsg, "zero rows ")
    want = v.double().mean(dim=1)  # uniform softmax: the mean of v
    assert (got["msg"][:, dead].cpu().double() - want[:, None]).abs().max() < 1e-5
    assert (got["lse"][:, dead].cpu() - math.log(130)).abs().max() < 1e-5


def test_large_logits_rebase_the_max():
    dev = torch.device("cuda")
    q, k, v, dmsg, M = _case130(dev)
    X = M.cpu() * (torch.matmul(q, k.transpose(1, 2)) / math.sqrt(C))
    f = math.sqrt(60.0 / X.abs().max().item())
    q, k = q * f, k * f
    got = _hip(q, k, v, M, dmsg, dev)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _hold(got, q, k, v, M.cpu(), dmsg, "|X| ~ 60 ")


def test_zero_dmsg_gives_exact_zeros():
    dev = torch.device("cuda")
    q, k, v, dmsg, M = _case130(dev)
    got = _hip(q, k, v, M, torch.zeros_like(dmsg), dev)
    for n in ("dq", "dk", "dv"):
        assert torch.count_nonzero(got[n]).item() == 0, n


def test_function_takes_non_contiguous_inputs():
    from pointdsc_amd.training import nonlocal_attention
    dev = torch.device("cuda")
    q, k, v, dmsg, M = _case130(dev)
    # [B,C,N] storage seen as [B,N,C], as the encoder's Conv1d outputs are
    qd, kd, vd = (t.transpose(1, 2).contiguous().to(dev).transpose(1, 2).requires_grad_() for t in (q, k, v))
    gd = dmsg.transpose(1, 2).contiguous().to(dev).transpose(1, 2)
    assert not qd.is_contiguous() and not gd.is_contiguous()
    Mg = M.clone().requires_grad_()
    msg = nonlocal_attention(qd, kd, vd, Mg)
    msg.backward(gd)
    assert Mg.grad is None
    ref = _hip(q, k, v, M, dmsg, dev)
    for n, t in (("msg", msg), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
        assert torch.equal(t.detach(), ref[n]), n
    _hold(dict(ref, msg=msg, dq=qd.grad, dk=kd.grad, dv=vd.grad), q, k, v, M.cpu(), dmsg, "strided ")


@pytest.mark.parametrize("B,N", [(2, 130), (2, 300)])
def test_bit_equality(B, N):
    from pointdsc_amd import kernels
    dev = torch.device("cuda")
    q, k, v, dmsg, src, tgt = _inputs(B, N, seed=9)
    M = _compat(src, tgt, dev)
    a, b = _hip(q, k, v, M, dmsg, dev), _hip(q, k, v, M, dmsg, dev)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n
    assert torch.equal(a["msg"], kernels.attention(q.to(dev), k.to(dev), v.to(dev), M, precision="f32"))


def test_abi_errors_launch_nothing():
    from pointdsc_amd import _lib
    dev = torch.device("cuda")
    L = _lib.load()
    B, N = 1, 40
    t = [torch.randn(B, N, C, device=dev) for _ in range(5)]  # q k v msg dmsg
    M, lse = torch.rand(B, N, N, device=dev), torch.zeros(B, N, device=dev)
    out = [torch.full((B, N, C), 7.0, device=dev) for _ in range(3)]
    nb = L.pdsc_attention_backward_workspace_bytes(B, N, C)
    assert nb > 0 and L.pdsc_attention_backward_workspace_bytes(B, N, 64) == 0
    assert L.pdsc_attention_lse_workspace_bytes(B, N, C) > 0 and L.pdsc_attention_lse_workspace_bytes(B, N, 64) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def bwd(Cc=C, dq=p(out[0]), nbytes=nb):
        return L.pdsc_attention_backward_f32(p(t[0]), p(t[1]), p(t[2]), p(M), p(t[3]), p(lse), p(t[4]), B, N, Cc, dq,
                                             p(out[1]), p(out[2]), p(ws), nbytes, s)

    ERR_ARG = 1  # include/pdsc.h: PDSC_ERR_ARG
    assert bwd(Cc=64) == ERR_ARG
    assert bwd(dq=None) == ERR_ARG and b"null" in L.pdsc_last_error()
    assert bwd(nbytes=nb - 1) == ERR_ARG and b"workspace" in L.pdsc_last_error()
    msg = torch.full((B, N, C), 7.0, device=dev)

    def fwd(Cc=C, lsep=p(lse), nbytes=None):
        n = L.pdsc_attention_lse_workspace_bytes(B, N, C)
        w = torch.empty(n, dtype=torch.uint8, device=dev)
        return L.pdsc_attention_lse_f32(p(t[0]), p(t[1]), p(t[2]), p(M), B, N, Cc, p(msg), lsep, p(w),
                                        n if nbytes is None else nbytes, s)

    assert fwd(Cc=64) == ERR_ARG and fwd(lsep=None) == ERR_ARG and fwd(nbytes=16) == ERR_ARG
    torch.cuda.synchronize()
    for o in out + [msg]:
        assert bool((o == 7.0).all())
    assert bwd() == 0 and fwd() == 0
    torch.cuda.synchronize()
