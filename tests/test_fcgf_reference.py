"""tests/fcgf_reference.py pinned to something independent of it: torch's dense
conv3d / conv_transpose3d on a scattered volume, brute-force Python for the
coordinate sets, and a fixture of the state dict's names and shapes written down
from misc/fcgf.py.  CPU only."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fcgf_reference as R
from conftest import GOLDEN

ORIGIN = -6  # even, so that a volume index and its coordinate have the same parity
D = 12


def occupancy(seed, frac=0.3):
    """About D^3 * frac occupied voxels with coordinates in [ORIGIN, ORIGIN + D): [n,4], ascending."""
    rs = np.random.RandomState(seed)
    occ = rs.rand(D, D, D) < frac
    x, y, z = np.nonzero(occ)
    c = np.stack([np.zeros_like(x), x + ORIGIN, y + ORIGIN, z + ORIGIN], 1)
    assert (c[:, 1:] < 0).any() and (c[:, 1:] > 0).any()
    return R.sort_rows(c)


def scatter(coords, feats, size, origin, step=1):
    """[1, C, Z, Y, X] volume with feats at (c - origin) / step."""
    vol = torch.zeros((1, feats.shape[1], size, size, size), dtype=torch.float64)
    i = (np.asarray(coords)[:, 1:] - origin) // step
    vol[0, :, i[:, 2], i[:, 1], i[:, 0]] = feats.T
    return vol


def gather(vol, coords, origin, step=1):
    i = (np.asarray(coords)[:, 1:] - origin) // step
    return vol[0, :, i[:, 2], i[:, 1], i[:, 0]].T


def dense_weight(w, K, transposed=False):
    """kernel [K^3, C_in, C_out] with k = (ox+r) + K (oy+r) + K^2 (oz+r) -> conv3d's
    [C_out, C_in, z, y, x] (conv_transpose3d's [C_in, C_out, z, y, x])."""
    w = w.reshape(K, K, K, w.shape[1], w.shape[2])  # [z, y, x, ci, co]
    return w.permute(3, 4, 0, 1, 2) if transposed else w.permute(4, 3, 0, 1, 2)


@pytest.mark.parametrize("K", [3, 5, 7])
def test_stride1_matches_dense_conv3d(K):
    rs = np.random.RandomState(K)
    c = occupancy(10 + K)
    x = torch.from_numpy(rs.standard_normal((len(c), 3)))
    w = torch.from_numpy(rs.standard_normal((K ** 3, 3, 5)))
    ours = R.sparse_conv(x, w, R.kernel_map(c, c, K, 1))
    dense = F.conv3d(scatter(c, x, D, ORIGIN), dense_weight(w, K), padding=K // 2)
    ref = gather(dense, c, ORIGIN)
    assert float((ours - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_stride2_matches_dense_conv3d_at_floor_aligned_outputs():
    rs = np.random.RandomState(2)
    c = occupancy(22)
    c2 = R.coarsen(c, 2)
    # brute force: floor, so negatives round down (-5 -> -6, not -4)
    want = sorted({(0,) + tuple(2 * (v // 2) for v in row[1:]) for row in c.tolist()})
    assert c2.tolist() == [list(t) for t in want]
    assert (c2[:, 1:] % 2 == 0).all() and (c2[:, 1:] < 0).any()
    x = torch.from_numpy(rs.standard_normal((len(c), 4)))
    w = torch.from_numpy(rs.standard_normal((27, 4, 6)))
    ours = R.sparse_conv(x, w, R.kernel_map(c2, c, 3, 1))
    dense = F.conv3d(scatter(c, x, D, ORIGIN), dense_weight(w, 3), stride=2, padding=1)
    ref = gather(dense, c2, ORIGIN, 2)
    assert float((ours - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_transposed_matches_dense_conv_transpose3d_on_the_fine_set():
    rs = np.random.RandomState(3)
    fine = occupancy(33)
    coarse = R.coarsen(fine, 2)
    x = torch.from_numpy(rs.standard_normal((len(coarse), 4)))
    w = torch.from_numpy(rs.standard_normal((27, 4, 6)))
    nbr = R.kernel_map(fine, coarse, 3, 1, transposed=True)
    assert ((nbr >= 0).sum(0) <= 8).all() and ((nbr >= 0).sum(0) >= 1).all()  # <= 8 coarse parents, its own always
    # the stride-2 convolution's map with input and output swapped, same k
    down = R.kernel_map(coarse, fine, 3, 1)
    pairs_down = {(int(down[k, u]), u, k) for k in range(27) for u in range(len(coarse)) if down[k, u] >= 0}
    pairs_up = {(f, int(nbr[k, f]), k) for k in range(27) for f in range(len(fine)) if nbr[k, f] >= 0}
    assert pairs_down == pairs_up
    ours = R.sparse_conv(x, w, nbr)
    dense = F.conv_transpose3d(scatter(coarse, x, D // 2, ORIGIN, 2), dense_weight(w, 3, transposed=True), stride=2,
                               padding=1, output_padding=1)
    assert dense.shape[-1] == D
    ref = gather(dense, fine, ORIGIN)
    assert float((ours - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_strided_levels_use_the_tensor_stride():
    """A 3^3 kernel at tensor stride 4 reaches +-4, and the stride-8 set is floor(c / 8) 8."""
    c = occupancy(44)
    c4, c8 = R.coarsen(c, 4), R.coarsen(c, 8)
    assert c8.tolist() == R.coarsen(c4, 8).tolist() == R.coarsen(R.coarsen(c, 2), 8).tolist()
    nbr = R.kernel_map(c4, c4, 3, 4)
    rows = {tuple(r): i for i, r in enumerate(c4.tolist())}
    for k, o in R.offsets(3):
        for u, r in enumerate(c4.tolist()):
            assert nbr[k, u] == rows.get((r[0], r[1] + 4 * o[0], r[2] + 4 * o[1], r[3] + 4 * o[2]), -1)


def brute_quantize(xyz, v):
    seen, order = {}, []
    for i, p in enumerate(np.asarray(xyz, np.float32)):
        key = tuple(int(np.floor(np.float32(p[a]) / np.float32(v))) for a in range(3))
        if key not in seen:
            seen[key] = i
            order.append(key)
    keys = sorted(order)
    return [seen[k] for k in keys], [[0, *k] for k in keys]


def test_quantize_against_brute_force():
    rs = np.random.RandomState(5)
    v = 0.25
    pts = rs.uniform(-1.0, 1.0, (150, 3)).astype(np.float32)
    pts[20:40] = pts[0:20]                                   # duplicate points
    pts[40:60] = (rs.randint(-4, 4, (20, 3)) * v).astype(np.float32)   # exactly on voxel faces
    pts[60:70] = pts[40:50] - np.float32(1e-6)               # just below a face
    inds, coords = R.quantize(pts, v)
    bi, bc = brute_quantize(pts, v)
    assert inds.tolist() == bi and coords.tolist() == bc
    assert (coords[:, 1:] < 0).any()
    assert len(inds) < len(pts)
    # the kept point is the lowest index of its voxel
    assert all(i < 20 or i >= 40 for i in inds.tolist())
    # a batch: the same cloud twice gives the same voxels under batch 0 and 1
    i2, c2 = R.quantize(np.concatenate([pts, pts]), v, [0, 150, 300])
    assert c2[:len(inds), 1:].tolist() == coords[:, 1:].tolist() == c2[len(inds):, 1:].tolist()
    assert i2.tolist() == inds.tolist() + (inds + 150).tolist()


@pytest.mark.parametrize("ks", [5, 7])
def test_state_dict_keys_match_fixture(ks):
    from pointdsc_amd.fcgf import FCGF, fcgf_state_dict, state_dict_spec
    with open(os.path.join(GOLDEN, "fcgf", "state_dict_keys.json")) as f:
        want = [(n, tuple(s)) for n, s in json.load(f)[str(ks)]]
    assert [(n, tuple(s)) for n, s in state_dict_spec(ks, 32)] == want
    m = FCGF(1, 32, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=True)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    sd = fcgf_state_dict(0, ks, 32)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    again = fcgf_state_dict(0, ks, 32)
    assert all(torch.equal(again[k], sd[k]) for k in sd)


def test_load_state_dict_strict_and_1x1_shapes():
    from pointdsc_amd.fcgf import FCGF, fcgf_state_dict
    sd = fcgf_state_dict(1, 5, 16)
    m = FCGF(out_channels=16, conv1_kernel_size=5)
    m.load_state_dict(sd, strict=True)
    dropped = {k: v for k, v in sd.items() if k != "block3.norm2.bn.running_var"}
    with pytest.raises(RuntimeError, match="running_var"):
        FCGF(out_channels=16, conv1_kernel_size=5).load_state_dict(dropped, strict=True)
    bad = dict(sd)
    bad["conv2.kernel"] = sd["conv2.kernel"].transpose(1, 2).contiguous()
    with pytest.raises(RuntimeError, match="conv2.kernel"):
        FCGF(out_channels=16, conv1_kernel_size=5).load_state_dict(bad, strict=True)
    three = dict(sd)
    three["conv1_tr.kernel"], three["final.kernel"] = sd["conv1_tr.kernel"][None], sd["final.kernel"][None]
    m3 = FCGF(out_channels=16, conv1_kernel_size=5)
    m3.load_state_dict(three, strict=True)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m3.state_dict().items())


def test_module_refuses_cpu_and_training():
    from pointdsc_amd.fcgf import FCGF, extract_features
    m = FCGF(out_channels=16, conv1_kernel_size=5)
    c, f = torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 1))
    with pytest.raises(NotImplementedError, match="inference only"):
        m(c, f)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(c, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        extract_features(m, np.zeros((4, 3), np.float32), 0.05)
    with pytest.raises(NotImplementedError):
        FCGF(in_channels=3)
    with pytest.raises(NotImplementedError):
        FCGF(conv1_kernel_size=3)


def test_abi_argument_errors_without_device():
    """Null pointers, n < 1, a bad kernel size and a short workspace return the
    existing codes before anything touches the device (dummy non-null pointers)."""
    from pointdsc_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(256)
    ws = lib.pdsc_fcgf_workspace_bytes(1000, 1, 7, 32)
    assert ws > 0 and ws == lib.pdsc_fcgf_workspace_bytes(1000, 1, 7, 32)
    assert lib.pdsc_fcgf_workspace_bytes(2000, 1, 7, 32) > ws
    for bad in ((0, 1, 7, 32), (1000, 0, 7, 32), (1000, 65, 7, 32), (1000, 1, 3, 32), (1000, 1, 7, 33)):
        assert lib.pdsc_fcgf_workspace_bytes(*bad) == 0, bad
    assert lib.pdsc_fcgf_param_floats(7, 32) - lib.pdsc_fcgf_param_floats(5, 32) == (343 - 125) * 32
    assert lib.pdsc_fcgf_param_floats(7, 32) - lib.pdsc_fcgf_param_floats(7, 16) == 16 * 65
    assert lib.pdsc_fcgf_param_floats(6, 32) == 0 == lib.pdsc_fcgf_packed_floats(7, 0)
    ARG, UNSUP = 1, 3
    q = lambda *a: lib.pdsc_fcgf_quantize(*a, None)  # noqa: E731
    assert q(None, 1000, None, 1, 0.05, p, p, p, p, ws) == ARG and b"null" in lib.pdsc_last_error()
    assert q(p, 1000, None, 1, 0.05, p, p, None, p, ws) == ARG
    assert q(p, 0, None, 1, 0.05, p, p, p, p, ws) == ARG and b"n=0" in lib.pdsc_last_error()
    assert q(p, 1000, None, 1, 0.0, p, p, p, p, ws) == ARG and b"voxel" in lib.pdsc_last_error()
    assert q(p, 1000, None, 1, float("nan"), p, p, p, p, ws) == ARG
    assert q(p, 1000, None, 2, 0.05, p, p, p, p, ws) == ARG and b"batch_offsets" in lib.pdsc_last_error()
    assert q(p, 1000, p, 65, 0.05, p, p, p, p, ws) == UNSUP and b"batch" in lib.pdsc_last_error()
    assert q(p, 1000, None, 1, 0.05, p, p, p, p, ws - 1) == ARG and b"workspace too small" in lib.pdsc_last_error()
    f = lambda *a: lib.pdsc_fcgf_forward(*a, None)  # noqa: E731
    assert f(None, 7, 32, 1, p, p, 1000, p, None, p, ws) == ARG and b"null" in lib.pdsc_last_error()
    assert f(p, 7, 32, 1, None, p, 1000, p, None, p, ws) == ARG
    assert f(p, 7, 32, 1, p, None, 1000, None, None, p, ws) == ARG
    assert f(p, 7, 32, 1, p, p, 0, p, None, p, ws) == ARG and b"m=0" in lib.pdsc_last_error()
    assert f(p, 3, 32, 1, p, p, 1000, p, None, p, ws) == UNSUP and b"conv1_kernel_size" in lib.pdsc_last_error()
    assert f(p, 7, 64, 1, p, p, 1000, p, None, p, ws) == UNSUP and b"out_channels" in lib.pdsc_last_error()
    assert f(p, 7, 32, 1, p, p, 1000, p, None, p, ws - 1) == ARG and b"workspace too small" in lib.pdsc_last_error()
    assert lib.pdsc_fcgf_pack_weights(None, 7, 32, p, None) == ARG
    assert lib.pdsc_fcgf_pack_weights(p, 4, 32, p, None) == UNSUP
