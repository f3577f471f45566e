"""FCGF descriptors on the GPU: misc/fcgf.py's ``ResUNetBN2C`` (the sparse 3-D
ResUNet of AmnonDrory/PointDSC's ``demo_registration.py:11-35``,
``misc/cal_fcgf.py:12-85`` and ``datasets/LidarFeatureExtractor.py:166-200``)
in eval mode on the gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f8).

MinkowskiEngine is not needed: quantisation, coordinate maps, kernel maps and
the network are restated (include/pdsc.h fixes every choice).  MinkowskiEngine
and the released FCGF checkpoints are not available to this build, so parity
with them is unpinned; if MinkowskiEngine orders kernel offsets differently,
``fcgf_checkpoint_index`` in ``csrc/fcgf.hip`` is the one function to change.

There is no CPU path and no training path: tensors must be HIP device tensors
and the module must be in eval mode.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._call import call, query

CHANNELS = [None, 32, 64, 128, 256]      # ResUNetBN2C (misc/fcgf.py:864-868)
TR_CHANNELS = [None, 64, 64, 64, 128]
BATCH_MAX = 64


class _Conv(nn.Module):
    """MinkowskiConvolution / MinkowskiConvolutionTranspose: ``kernel`` [K^3, C_in,
    C_out] ([C_in, C_out] for a 1x1x1 kernel; [1, C_in, C_out] is accepted on
    load) and an optional ``bias`` [1, C_out]."""

    def __init__(self, cin, cout, kernel_size, bias=False):
        super().__init__()
        k3 = kernel_size ** 3
        self.kernel = nn.Parameter(torch.zeros((k3, cin, cout) if k3 > 1 else (cin, cout)))
        self.bias = nn.Parameter(torch.zeros(1, cout)) if bias else None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = state_dict.get(prefix + "kernel")
        if k is not None and self.kernel.dim() == 2 and k.dim() == 3 and k.shape[0] == 1:
            state_dict[prefix + "kernel"] = k[0]
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class _Norm(nn.Module):
    """MinkowskiBatchNorm: a BatchNorm1d on the feature rows, under ``.bn``."""

    def __init__(self, c, momentum):
        super().__init__()
        self.bn = nn.BatchNorm1d(c, momentum=momentum)


class _Block(nn.Module):
    """BasicBlockBN (misc/fcgf.py:107-162)."""

    def __init__(self, c, momentum):
        super().__init__()
        self.conv1, self.norm1 = _Conv(c, c, 3), _Norm(c, momentum)
        self.conv2, self.norm2 = _Conv(c, c, 3), _Norm(c, momentum)


class FCGF(nn.Module):
    """ResUNetBN2C(in_channels, out_channels, bn_momentum, conv1_kernel_size,
    normalize_feature) with the reference's parameter names; inference only."""

    def __init__(self, in_channels=1, out_channels=32, bn_momentum=0.05, conv1_kernel_size=7, normalize_feature=True):
        super().__init__()
        if in_channels != 1:
            raise NotImplementedError("FCGF: in_channels must be 1 (the occupancy feature of misc/cal_fcgf.py:67-68)")
        if conv1_kernel_size not in (5, 7):
            raise NotImplementedError(f"FCGF: conv1_kernel_size {conv1_kernel_size} not 5 or 7")
        if not 1 <= out_channels <= 32:
            raise NotImplementedError(f"FCGF: out_channels {out_channels} not in [1, 32]")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.conv1_kernel_size, self.normalize_feature = conv1_kernel_size, bool(normalize_feature)
        C, T, mo = CHANNELS, TR_CHANNELS, bn_momentum
        self.conv1, self.norm1, self.block1 = _Conv(in_channels, C[1], conv1_kernel_size), _Norm(C[1], mo), _Block(C[1], mo)
        self.conv2, self.norm2, self.block2 = _Conv(C[1], C[2], 3), _Norm(C[2], mo), _Block(C[2], mo)
        self.conv3, self.norm3, self.block3 = _Conv(C[2], C[3], 3), _Norm(C[3], mo), _Block(C[3], mo)
        self.conv4, self.norm4, self.block4 = _Conv(C[3], C[4], 3), _Norm(C[4], mo), _Block(C[4], mo)
        self.conv4_tr, self.norm4_tr, self.block4_tr = _Conv(C[4], T[4], 3), _Norm(T[4], mo), _Block(T[4], mo)
        self.conv3_tr, self.norm3_tr, self.block3_tr = _Conv(C[3] + T[4], T[3], 3), _Norm(T[3], mo), _Block(T[3], mo)
        self.conv2_tr, self.norm2_tr, self.block2_tr = _Conv(C[2] + T[3], T[2], 3), _Norm(T[2], mo), _Block(T[2], mo)
        self.conv1_tr = _Conv(C[1] + T[2], T[1], 1)
        self.final = _Conv(T[1], out_channels, 1, bias=True)
        self._packed = None

    # ------------------------------------------------------------- weights
    def _flat_tensors(self):
        """The tensors of pdsc_fcgf_pack_weights' flat buffer, in its order (state-dict
        order without num_batches_tracked)."""
        return [v for k, v in self.state_dict(keep_vars=True).items() if not k.endswith("num_batches_tracked")]

    def packed_weights(self, device):
        ts = self._flat_tensors()
        stamp = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is None or self._packed[0] != stamp:
            ks, co = self.conv1_kernel_size, self.out_channels
            flat = torch.cat([t.detach().reshape(-1).to(device=device, dtype=torch.float32) for t in ts])
            assert flat.numel() == query("pdsc_fcgf_param_floats", ks, co, required=True), flat.numel()
            packed = torch.empty(query("pdsc_fcgf_packed_floats", ks, co, required=True), dtype=torch.float32,
                                 device=device)
            call("pdsc_fcgf_pack_weights", flat, ks, co, packed, device=device)
            self._packed = (stamp, packed)
        return self._packed[1]

    # ------------------------------------------------------------- forward
    def forward(self, coords: torch.Tensor, feats: torch.Tensor, debug: bool = False):
        """coords int32 [m,4] (batch, x, y, z; unique rows), feats [m,1] -> features
        [m, out_channels] (row i belongs to coords row i).  debug: also a dict of the
        intermediate tensors of ``pdsc_fcgf_debug``."""
        if self.training:
            raise NotImplementedError("FCGF: inference only (call .eval()); training and batch-statistics BN are out of scope")
        coords, feats = _dev(coords, "coords", dtype=torch.int32), _dev(feats, "feats")
        m = coords.shape[0]
        if coords.dim() != 2 or coords.shape[1] != 4 or tuple(feats.shape) != (m, 1):
            raise ValueError(f"coords {tuple(coords.shape)} must be [m,4] and feats {tuple(feats.shape)} [m,1]")
        dev = coords.device
        ks, co = self.conv1_kernel_size, self.out_channels
        out = torch.empty((m, co), dtype=torch.float32, device=dev)
        dbg, taps = None, None
        if debug:
            widths = {"block1": 32, "block2": 64, "block3": 128, "block4": 256, "block4_tr": 128, "block3_tr": 64,
                      "block2_tr": 64, "conv1_tr": 64}
            taps = {k: torch.zeros((m, c), dtype=torch.float32, device=dev) for k, c in widths.items()}
            for k in ("coords2", "coords4", "coords8"):
                taps[k] = torch.zeros((m, 4), dtype=torch.int32, device=dev)
            taps["counts"] = torch.zeros(4, dtype=torch.int32, device=dev)
            dbg = _lib.PdscFcgfDebug(**{k: ctypes.c_void_p(v.data_ptr()) for k, v in taps.items()})
        call("pdsc_fcgf_forward", self.packed_weights(dev), ks, co, int(self.normalize_feature), coords, feats, m, out,
             dbg, device=dev, ws=("pdsc_fcgf_workspace_bytes", m, 1, ks, co))
        if not debug:
            return out
        n = taps.pop("counts").cpu().numpy()
        level = {"block1": 0, "block2": 1, "block3": 2, "block4": 3, "block4_tr": 2, "block3_tr": 1, "block2_tr": 0,
                 "conv1_tr": 0, "coords2": 1, "coords4": 2, "coords8": 3}
        taps = {k: v[:int(n[level[k]])] for k, v in taps.items()}
        taps["final"] = out
        return out, taps


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"pointdsc_amd.fcgf: {name} must be a HIP device tensor; there is no CPU fallback")
    return t.to(dtype).contiguous()


def quantize(xyz: torch.Tensor, voxel_size: float, batch_offsets=None):
    """misc/cal_fcgf.py:73-77 on the GPU: coords = floor(xyz / voxel_size) (fp32),
    one point per voxel (the lowest input index), voxels in ascending (batch, x, y,
    z) order.  Returns (inds int64 [m], coords int32 [m,4]).  batch_offsets: the
    first point of every cloud of a concatenated batch, plus the total."""
    xyz = _dev(xyz, "xyz")
    n, dev = xyz.shape[0], xyz.device
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz {tuple(xyz.shape)} must be [n,3]")
    off, batch = None, 1
    if batch_offsets is not None:
        batch = len(batch_offsets) - 1
        off = torch.as_tensor(np.asarray(batch_offsets, np.int32), device=dev)
    inds = torch.empty(n, dtype=torch.int32, device=dev)
    coords = torch.empty((n, 4), dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    call("pdsc_fcgf_quantize", xyz, n, off, batch, float(voxel_size), inds, coords, cnt, device=dev,
         ws=("pdsc_fcgf_workspace_bytes", n, batch, 7, 32))
    m = int(cnt.item())
    return inds[:m].long(), coords[:m]


def extract_features(model: FCGF, xyz, voxel_size: float, device=None):
    """misc/cal_fcgf.py:12-85 (rgb = normal = None): (xyz_down [m,3] = xyz[inds],
    features [m, C_out]) as device tensors."""
    if not isinstance(xyz, torch.Tensor):
        xyz = torch.as_tensor(np.asarray(xyz, np.float32))
    if device is not None:
        xyz = xyz.to(device)
    xyz = _dev(xyz, "xyz")
    inds, coords = quantize(xyz, voxel_size)
    feats = torch.ones((len(inds), 1), dtype=torch.float32, device=xyz.device)
    return xyz[inds], model(coords, feats)


def extract_batch(model: FCGF, clouds, voxel_size: float, device=None):
    """datasets/LidarFeatureExtractor.py:166-200 (process_batch): the clouds
    concatenated with a batch index, one quantisation and one network call.  Returns
    [(xyz_down, features)] per cloud, each bitwise equal to extract_features'."""
    ts = [c if isinstance(c, torch.Tensor) else torch.as_tensor(np.asarray(c, np.float32)) for c in clouds]
    if device is not None:
        ts = [t.to(device) for t in ts]
    ts = [_dev(t, "xyz") for t in ts]
    if not 1 <= len(ts) <= BATCH_MAX:
        raise ValueError(f"extract_batch takes 1..{BATCH_MAX} clouds, got {len(ts)}")
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in ts])])
    xyz = torch.cat(ts)
    inds, coords = quantize(xyz, voxel_size, offsets)
    feats = model(coords, torch.ones((len(inds), 1), dtype=torch.float32, device=xyz.device))
    b = coords[:, 0].contiguous()
    cuts = torch.searchsorted(b, torch.arange(len(ts) + 1, dtype=torch.int32, device=b.device)).tolist()
    return [(xyz[inds[s:e]], feats[s:e]) for s, e in zip(cuts[:-1], cuts[1:])]


# ------------------------------------------------------------------ weights
def state_dict_spec(conv1_kernel_size=7, out_channels=32):
    """[(name, shape)] of ResUNetBN2C(1, out_channels, conv1_kernel_size=...)'s
    state dict in MinkowskiEngine's naming and order (misc/fcgf.py:630-798)."""
    C, T = CHANNELS, TR_CHANNELS
    spec = []

    def conv(name, k, cin, cout):
        spec.append((name + ".kernel", (k ** 3, cin, cout) if k > 1 else (cin, cout)))

    def norm(name, c):
        spec.extend([(f"{name}.bn.weight", (c,)), (f"{name}.bn.bias", (c,)), (f"{name}.bn.running_mean", (c,)),
                     (f"{name}.bn.running_var", (c,)), (f"{name}.bn.num_batches_tracked", ())])

    def stage(tag, k, cin, cout):
        conv("conv" + tag, k, cin, cout)
        norm("norm" + tag, cout)
        for i in (1, 2):
            conv(f"block{tag}.conv{i}", 3, cout, cout)
            norm(f"block{tag}.norm{i}", cout)

    stage("1", conv1_kernel_size, 1, C[1])
    stage("2", 3, C[1], C[2])
    stage("3", 3, C[2], C[3])
    stage("4", 3, C[3], C[4])
    stage("4_tr", 3, C[4], T[4])
    stage("3_tr", 3, C[3] + T[4], T[3])
    stage("2_tr", 3, C[2] + T[3], T[2])
    conv("conv1_tr", 1, C[1] + T[2], T[1])
    conv("final", 1, T[1], out_channels)
    spec.append(("final.bias", (1, out_channels)))
    return spec


def fcgf_state_dict(seed=0, conv1_kernel_size=7, out_channels=32):
    """Deterministic synthetic weights (no checkpoint is distributed): kernels
    Kaiming-normal fan_out (misc/fcgf.py:1080-1087; fan_out = K^3 C_out), BN affine
    near (1, 0) and randomised running statistics.  The running variances are drawn
    around 1.2 (0.08 for norm1: a cloud fills a small part of conv1's K^3 cube), which
    keeps the activations of surface-like and of solid clouds O(1) through all four
    levels (every block's residual adds to them)."""
    rs = np.random.RandomState(seed)
    sd = {}
    for name, shape in state_dict_spec(conv1_kernel_size, out_channels):
        if name.endswith(".kernel"):
            k3 = shape[0] if len(shape) == 3 else 1
            v = rs.standard_normal(shape) * np.sqrt(2.0 / (k3 * shape[-1]))
        elif name.endswith("running_var"):
            first = name == "norm1.bn.running_var"
            v = rs.uniform(0.5, 1.5, shape) * (0.08 if first else 1.2)
        elif name.endswith("bn.weight"):
            v = rs.uniform(0.8, 1.2, shape)
        elif name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(1000, dtype=torch.int64)
            continue
        else:  # bn.bias, running_mean, final.bias
            v = rs.standard_normal(shape) * 0.1
        sd[name] = torch.from_numpy(np.asarray(v, np.float32))
    return sd
