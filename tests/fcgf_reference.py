"""The FCGF semantics of include/pdsc.h (f8), restated in numpy / torch on the
CPU: the yardstick of tests/test_gpu_fcgf.py, itself pinned to torch's dense
conv3d / conv_transpose3d by tests/test_fcgf_reference.py.

What it restates of AmnonDrory/PointDSC (MinkowskiEngine is absent; its
published behaviour is written out):
  misc/cal_fcgf.py:73-77   coords = floor(xyz / voxel_size), sparse_quantize
                           (one point per voxel), xyz[inds]
  misc/fcgf.py:630-798     ResUNet2.__init__ with BN2C's channels
  misc/fcgf.py:142-158     BasicBlockBN.forward
  misc/fcgf.py:800-851     ResUNet2.forward

fp64 by default (the exact-arithmetic yardstick).  dtype=torch.float32 with a
seed is one more fp32 realisation: every reduction (kernel offsets, input
channels) is summed in a seeded random order, like conftest.encoder_torch.
"""
import numpy as np
import torch

CHANNELS = [None, 32, 64, 128, 256]     # misc/fcgf.py:864-868 (ResUNetBN2C)
TR_CHANNELS = [None, 64, 64, 64, 128]


# ------------------------------------------------------------ coordinates
def quantize(xyz, voxel_size, batch_offsets=None):
    """misc/cal_fcgf.py:73-74: floor(xyz / voxel_size) on fp32 (IEEE divide), one
    point per voxel -- the lowest input index --, voxels in ascending (batch, x, y,
    z) order.  Returns (inds [m], coords int64 [m,4])."""
    xyz = np.asarray(xyz, np.float32)
    c = np.floor(xyz / np.float32(voxel_size)).astype(np.int64)
    b = np.zeros(len(xyz), np.int64)
    if batch_offsets is not None:
        for i, (s, e) in enumerate(zip(batch_offsets[:-1], batch_offsets[1:])):
            b[s:e] = i
    rows = np.concatenate([b[:, None], c], 1)
    order = np.lexsort((np.arange(len(rows)), rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))
    srt = rows[order]
    head = np.ones(len(srt), bool)
    head[1:] = np.any(srt[1:] != srt[:-1], 1)
    return order[head], srt[head]


def sort_rows(coords):
    c = np.asarray(coords, np.int64)
    return c[np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))]


def coarsen(coords, stride):
    """The output coordinates of a stride-2 convolution whose outputs have tensor
    stride `stride`: unique(floor(c / stride) stride), ascending."""
    c = np.asarray(coords, np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], stride) * stride  # floor: negatives round down
    return sort_rows(np.unique(c, axis=0))


def kernel_index(o, K):
    """The one ordering of kernel offsets: k = (ox + r) + K (oy + r) + K^2 (oz + r)."""
    r = K // 2
    return (o[0] + r) + K * (o[1] + r) + K * K * (o[2] + r)


def offsets(K):
    """[(k, o)] for the centred HYPER_CUBE of size K, ascending k."""
    r = K // 2
    out = [(kernel_index((x, y, z), K), (x, y, z)) for z in range(-r, r + 1) for y in range(-r, r + 1)
           for x in range(-r, r + 1)]
    assert [k for k, _ in out] == list(range(K ** 3))
    return out


def kernel_map(out_coords, in_coords, K, step, transposed=False):
    """nbr [K^3, n_out]: the row of in_coords that output u reads through offset
    k, or -1.  A convolution reads u + o step; a transposed one is the stride-2
    convolution's map (coarse u' reads fine u' + o step) with input and output
    swapped: fine u reads the coarse u - o step."""
    def key(c):  # one integer per (batch, x, y, z); coordinates within +-2^20
        c = np.asarray(c, np.int64)
        return ((c[:, 0] * (1 << 21) + c[:, 1] + (1 << 20)) * (1 << 21) + c[:, 2] + (1 << 20)) * (1 << 21) + c[:, 3] + (1 << 20)

    ik = key(in_coords)
    order = np.argsort(ik, kind="stable")
    sk = ik[order]
    oc = np.asarray(out_coords, np.int64)
    nbr = np.full((K ** 3, len(oc)), -1, np.int64)
    sign = -1 if transposed else 1
    for k, o in offsets(K):
        q = key(oc + sign * step * np.array((0,) + o, np.int64))
        p = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
        nbr[k] = np.where(sk[p] == q, order[p], -1)
    return nbr


def sparse_conv(x, w, nbr, gen=None):
    """out[u] = sum_k x[nbr[k, u]] @ w[k] over the present neighbours (nbr None:
    a 1x1x1 kernel, the row itself); w [K^3, C_in, C_out] or [C_in, C_out].  gen: a
    RandomState -- offsets and input channels are then summed in a random order."""
    w = w.reshape(-1, w.shape[-2], w.shape[-1])
    n_out = len(x) if nbr is None else nbr.shape[1]
    out = torch.zeros((n_out, w.shape[2]), dtype=x.dtype)
    for k in (range(w.shape[0]) if gen is None else gen.permutation(w.shape[0])):
        rows = np.arange(n_out) if nbr is None else nbr[k]
        have = np.nonzero(rows >= 0)[0]
        if not len(have):
            continue
        a, b = x[rows[have]], w[k]
        if gen is not None:
            p = torch.from_numpy(gen.permutation(a.shape[1]))
            a, b = a[:, p], b[p]
        out[have] += a @ b
    return out


# ----------------------------------------------------------------- network
class Net:
    """ResUNetBN2C(1, C_out, conv1_kernel_size, normalize_feature) in eval mode on
    one set of level-1 coordinates (rows in the caller's order)."""

    def __init__(self, coords, conv1_kernel_size):
        c1 = np.asarray(coords, np.int64)
        self.coords = [c1, coarsen(c1, 2), coarsen(c1, 4), coarsen(c1, 8)]
        C = self.coords
        self.conv1_map = kernel_map(c1, c1, conv1_kernel_size, 1)
        self.nbr = [kernel_map(C[l], C[l], 3, 1 << l) for l in range(4)]
        self.down = [kernel_map(C[l + 1], C[l], 3, 1 << l) for l in range(3)]
        self.up = [kernel_map(C[l], C[l + 1], 3, 1 << l, transposed=True) for l in range(3)]

    def forward(self, sd, feats=None, dtype=torch.float64, seed=None, normalize=True):
        """-> dict of the tensors after block1..4, block4_tr..2_tr, conv1_tr (+ ReLU) and
        final (normalised), as numpy fp64."""
        gen = np.random.RandomState(seed) if seed is not None else None
        W = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

        def conv(x, name, nbr):
            return sparse_conv(x, W[name + ".kernel"], nbr, gen)

        def bn(x, name):  # MinkowskiBatchNorm in eval mode: BatchNorm1d(eps = 1e-5) on the rows
            a = W[name + ".bn.weight"] / torch.sqrt(W[name + ".bn.running_var"] + 1e-5)
            return x * a + (W[name + ".bn.bias"] - W[name + ".bn.running_mean"] * a)

        def block(x, name, nbr):  # misc/fcgf.py:142-158
            out = torch.relu(bn(conv(x, name + ".conv1", nbr), name + ".norm1"))
            out = bn(conv(out, name + ".conv2", nbr), name + ".norm2")
            return torch.relu(out + x)

        n1 = len(self.coords[0])
        x = torch.ones((n1, 1), dtype=dtype) if feats is None else torch.as_tensor(np.asarray(feats)).to(dtype)
        t = {}
        # misc/fcgf.py:801-804
        out_s1 = t["block1"] = block(bn(conv(x, "conv1", self.conv1_map), "norm1"), "block1", self.nbr[0])
        out = torch.relu(out_s1)
        # :806-809
        out_s2 = t["block2"] = block(bn(conv(out, "conv2", self.down[0]), "norm2"), "block2", self.nbr[1])
        out = torch.relu(out_s2)
        # :811-814
        out_s4 = t["block3"] = block(bn(conv(out, "conv3", self.down[1]), "norm3"), "block3", self.nbr[2])
        out = torch.relu(out_s4)
        # :816-819
        out_s8 = t["block4"] = block(bn(conv(out, "conv4", self.down[2]), "norm4"), "block4", self.nbr[3])
        out = torch.relu(out_s8)
        # :821-826
        out = t["block4_tr"] = block(bn(conv(out, "conv4_tr", self.up[2]), "norm4_tr"), "block4_tr", self.nbr[2])
        out = torch.cat([torch.relu(out), out_s4], 1)
        # :828-833
        out = t["block3_tr"] = block(bn(conv(out, "conv3_tr", self.up[1]), "norm3_tr"), "block3_tr", self.nbr[1])
        out = torch.cat([torch.relu(out), out_s2], 1)
        # :835-840
        out = t["block2_tr"] = block(bn(conv(out, "conv2_tr", self.up[0]), "norm2_tr"), "block2_tr", self.nbr[0])
        out = torch.cat([torch.relu(out), out_s1], 1)
        # :841-843
        out = t["conv1_tr"] = torch.relu(conv(out, "conv1_tr", None))
        out = conv(out, "final", None) + W["final.bias"].reshape(1, -1)
        if normalize:  # :845-849
            out = out / (torch.norm(out, p=2, dim=1, keepdim=True) + 1e-8)
        t["final"] = out
        return {k: v.double().numpy() for k, v in t.items()}


TAPS = ("block1", "block2", "block3", "block4", "block4_tr", "block3_tr", "block2_tr", "conv1_tr", "final")
TAP_LEVEL = {"block1": 0, "block2": 1, "block3": 2, "block4": 3, "block4_tr": 2, "block3_tr": 1, "block2_tr": 0,
             "conv1_tr": 0, "final": 0}


def envelope(net, sd, feats=None, seeds=4, normalize=True):
    """(fp64 taps, {tap: max over `seeds` re-ordered fp32 runs of max |fp32 - fp64|})."""
    t64 = net.forward(sd, feats, normalize=normalize)
    noise = {k: 0.0 for k in TAPS}
    for s in range(seeds):
        t32 = net.forward(sd, feats, torch.float32, seed=s, normalize=normalize)
        for k in TAPS:
            noise[k] = max(noise[k], float(np.abs(t32[k] - t64[k]).max()))
    return t64, noise
