"""FCGF on the GPU (pointdsc_amd.fcgf, csrc/fcgf.hip) against its restatement
(tests/fcgf_reference.py, pinned by tests/test_fcgf_reference.py).

Structure is exact: inds, the coordinates and the counts of all four levels.
Features are held to the project's envelope rule at every debug tap and at the
output: max |ours - fp64| <= ENVELOPE x (max over 4 seeds of max |fp32
re-ordered - fp64|) + FEAT_FLOOR x max |fp64|, the fp32 noise measured per case
from the restatement.  Worst ratios observed: DESIGN.md section 7.
"""
import os

import numpy as np
import pytest
import torch

import fcgf_reference as R
from conftest import ENVELOPE, FEAT_FLOOR, GOLDEN

pytestmark = pytest.mark.gpu
DEMO = os.path.join(GOLDEN, "demo_data")


# ------------------------------------------------------------------ shapes
def blob(m, seed, spread=None):
    """m distinct voxels around a few centres (a surface-like cluster), straddling 0."""
    rs = np.random.RandomState(seed)
    spread = spread or max(1.0, (m / 4.0) ** (1 / 3))
    got, seen = [], set()
    while len(got) < m:
        p = np.rint(rs.standard_normal((4 * m + 16, 3)) * spread * np.array([1.0, 1.0, 0.35])).astype(np.int64)
        for r in map(tuple, p.tolist()):
            if r not in seen and len(got) < m:
                seen.add(r)
                got.append(r)
    c = np.array(got, np.int64)
    return np.concatenate([np.zeros((m, 1), np.int64), c], 1)


def single_coarsest():
    """All voxels inside one stride-8 cell, on the negative side."""
    c = blob(40, 3, spread=1.5)
    c[:, 1:] = np.clip(c[:, 1:], -3, 3) - 4   # within [-8, 0)
    c = np.unique(c, axis=0)
    assert len(R.coarsen(c, 8)) == 1
    return c


def isolated():
    """Voxels 32 apart: only the centre offset exists, at every level."""
    rs = np.random.RandomState(7)
    g = np.array([(x, y, z) for x in range(-2, 2) for y in range(-1, 2) for z in range(-1, 1)], np.int64) * 32
    g = g + rs.randint(0, 8, g.shape)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)


def dense_block():
    """10^3 voxels straddling 0: all 27 and all K^3 offsets present inside."""
    r = np.arange(-5, 5)
    g = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)


CASES = {
    "m1": (lambda: blob(1, 1), 5, 16),
    "m31": (lambda: blob(31, 2), 7, 32),
    "m32": (lambda: blob(32, 3), 5, 32),
    "m33": (lambda: blob(33, 4), 7, 16),
    "m63": (lambda: blob(63, 5), 5, 16),
    "m65": (lambda: blob(65, 6), 7, 32),
    "m257": (lambda: blob(257, 7), 5, 32),
    "m2000": (lambda: blob(2000, 8), 5, 16),
    "coarsest1": (single_coarsest, 7, 32),
    "isolated": (isolated, 7, 16),
    "dense": (dense_block, 7, 32),
}


def make_model(ks, cout, dev, seed=0, normalize=True):
    from pointdsc_amd.fcgf import FCGF, fcgf_state_dict
    sd = fcgf_state_dict(seed, ks, cout)
    m = FCGF(1, cout, bn_momentum=0.05, conv1_kernel_size=ks, normalize_feature=normalize)
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval(), {k: v.numpy() for k, v in sd.items()}


def hold_to_envelope(ours, t64, noise, what):
    """The envelope rule at every tap; prints and returns the ratio err / noise per tap."""
    ratios, bad = {}, []
    for k in R.TAPS:
        a, ref = ours[k].double().cpu().numpy(), t64[k]
        assert a.shape == ref.shape, (what, k, a.shape, ref.shape)
        err, mx = float(np.abs(a - ref).max()), float(np.abs(ref).max())
        bound = ENVELOPE * noise[k] + FEAT_FLOOR * mx
        ratios[k] = err / noise[k] if noise[k] > 0 else 0.0
        print(f"fcgf envelope {what} {k}: err {err:.3g} noise {noise[k]:.3g} max {mx:.3g} ratio {ratios[k]:.2f}")
        if not err <= bound:
            bad.append(f"{k}: err {err:.3g} > {ENVELOPE} x {noise[k]:.3g} + {FEAT_FLOOR:g} x {mx:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratios


@pytest.mark.parametrize("name", list(CASES))
def test_network_against_restatement(name, gpu_device):
    make, ks, cout = CASES[name]
    c = make()
    rs = np.random.RandomState(len(c))
    c = c[rs.permutation(len(c))]  # level-1 rows in the caller's (arbitrary) order
    model, sd = make_model(ks, cout, gpu_device)
    coords = torch.from_numpy(c.astype(np.int32)).to(gpu_device)
    feats = torch.ones((len(c), 1), device=gpu_device)
    out, taps = model(coords, feats, debug=True)
    net = R.Net(c, ks)
    # structure: exact
    for key, lvl in (("coords2", 1), ("coords4", 2), ("coords8", 3)):
        assert taps[key].cpu().numpy().tolist() == net.coords[lvl].tolist(), (name, key)
    # features: the envelope rule at every tap
    t64, noise = R.envelope(net, sd)
    hold_to_envelope(taps, t64, noise, name)
    norms = out.double().norm(dim=1).cpu().numpy()
    assert np.abs(norms - 1.0).max() <= 1e-6, norms
    # two runs are bitwise equal, and the debug taps change nothing
    assert torch.equal(model(coords, feats), out)


def test_input_feature_and_unnormalized_output(gpu_device):
    """feats is honoured by conv1 (not assumed 1) and normalize_feature=False returns final's rows."""
    c = blob(100, 11)
    model, sd = make_model(5, 32, gpu_device, seed=3, normalize=False)
    rs = np.random.RandomState(0)
    f = rs.uniform(0.5, 1.5, (len(c), 1)).astype(np.float32)
    out, taps = model(torch.from_numpy(c.astype(np.int32)).to(gpu_device), torch.from_numpy(f).to(gpu_device), debug=True)
    net = R.Net(c, 5)
    t64, noise = R.envelope(net, sd, feats=f, normalize=False)
    hold_to_envelope(taps, t64, noise, "feats")
    assert np.abs(out.double().norm(dim=1).cpu().numpy() - 1.0).max() > 1e-3


def cloud(n, seed, shift=(0.0, 0.0, 0.0)):
    """A wavy sheet with duplicates and points exactly on voxel faces, straddling 0."""
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-0.6, 0.6, (n, 2))
    z = 0.1 * np.sin(4 * xy[:, 0]) + 0.05 * rs.standard_normal(n)
    p = np.concatenate([xy, z[:, None]], 1).astype(np.float32) + np.asarray(shift, np.float32)
    p[n // 2:n // 2 + 50] = p[:50]                                    # duplicates
    p[n // 2 + 50:n // 2 + 100] = np.round(p[50:100] / 0.05) * np.float32(0.05)   # on voxel faces
    return p


def test_quantize_is_exact(gpu_device):
    from pointdsc_amd.fcgf import quantize
    v = 0.05
    a, b = cloud(3000, 1), cloud(2500, 2, (0.3, -0.2, 0.1))
    for pts, off in ((a, None), (np.concatenate([a, b]), [0, len(a), len(a) + len(b)])):
        inds, coords = quantize(torch.from_numpy(pts).to(gpu_device), v, off)
        ri, rc = R.quantize(pts, v, off)
        assert inds.cpu().numpy().tolist() == ri.tolist()
        assert coords.cpu().numpy().tolist() == rc.tolist()
        assert (rc[:, 1:] < 0).any() and len(ri) < len(pts)


def test_quantize_range_error(gpu_device):
    from pointdsc_amd.fcgf import quantize
    pts = torch.tensor([[0.0, 0.0, 0.0], [1.0e5, 0.0, 0.0]], device=gpu_device)
    with pytest.raises(RuntimeError, match=r"status 3.*outside"):
        quantize(pts, 0.05)  # 2e6 voxels > 2^18
    inds, coords = quantize(pts, 1.0)
    assert coords.cpu().numpy().tolist() == [[0, 0, 0, 0], [0, 100000, 0, 0]]


def test_extract_batch_equals_single_clouds_bitwise(gpu_device):
    from pointdsc_amd.fcgf import extract_batch, extract_features
    model, _ = make_model(5, 32, gpu_device, seed=2)
    a, b = cloud(3000, 1), cloud(2500, 2, (0.3, -0.2, 0.1))
    xa, fa = extract_features(model, a, 0.05, gpu_device)
    xb, fb = extract_features(model, b, 0.05, gpu_device)
    (ya, ga), (yb, gb) = extract_batch(model, [a, b], 0.05, gpu_device)
    assert torch.equal(xa, ya) and torch.equal(xb, yb)
    assert torch.equal(fa, ga) and torch.equal(fb, gb)
    ri, _ = R.quantize(a, 0.05)
    assert np.array_equal(xa.cpu().numpy(), a[ri])  # the kept ORIGINAL points, not voxel centres
    assert fa.shape == (len(ri), 32)


def test_load_state_dict_round_trip_on_device(gpu_device):
    """A round trip, both 1x1 kernel shapes and an in-place weight edit all reach the packed weights."""
    from pointdsc_amd.fcgf import FCGF
    model, sd = make_model(5, 16, gpu_device, seed=5)
    c = torch.from_numpy(blob(200, 12).astype(np.int32)).to(gpu_device)
    f = torch.ones((200, 1), device=gpu_device)
    out = model(c, f)
    again = FCGF(out_channels=16, conv1_kernel_size=5)
    saved = {k: v.cpu() for k, v in model.state_dict().items()}
    saved["conv1_tr.kernel"], saved["final.kernel"] = saved["conv1_tr.kernel"][None], saved["final.kernel"][None]
    again.load_state_dict(saved, strict=True)
    again = again.to(gpu_device).eval()
    assert torch.equal(again(c, f), out)
    with torch.no_grad():
        again.final.bias.add_(0.5)
    assert not torch.equal(again(c, f), out)


def test_cpu_tensors_raise(gpu_device):
    model, _ = make_model(5, 16, gpu_device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros((4, 4), dtype=torch.int32), torch.ones((4, 1)))


def test_demo_with_fcgf(gpu_device, tmp_path, capsys):
    """--descriptor fcgf --fcgf_weights on the demo's pair runs to a 4x4 pose (random
    weights: the pose itself means nothing), and register()'s src_features on a crop
    of cloud_bin_0 meet the envelope rule."""
    from pointdsc_amd import demo
    from pointdsc_amd.descriptors import read_ply
    from pointdsc_amd.fcgf import fcgf_state_dict
    sd = fcgf_state_dict(0, 7, 32)
    path = str(tmp_path / "fcgf.pth")
    torch.save({"state_dict": sd}, path)
    T = demo.main(["--pcd1", os.path.join(DEMO, "cloud_bin_0.ply"), "--pcd2", os.path.join(DEMO, "cloud_bin_1.ply"),
                   "--descriptor", "fcgf", "--fcgf_weights", path])
    assert T.shape == (4, 4) and np.isfinite(T).all()
    raw = read_ply(os.path.join(DEMO, "cloud_bin_0.ply"))
    lo = np.median(raw, 0) - 0.6
    crop = raw[np.all((raw >= lo) & (raw < lo + 1.2), 1)]
    ri, rc = R.quantize(crop, 0.05)
    assert 500 <= len(ri) <= 3000, len(ri)
    fm = demo.build_fcgf(path, gpu_device)
    pdsc = demo.build_model(demo.RELEASE_3DMATCH, None, gpu_device)
    res = demo.register(pdsc, crop, crop, 0.05, gpu_device, descriptor="fcgf", fcgf_model=fm)
    assert np.array_equal(res["src_pts"].cpu().numpy(), crop[ri])
    t64, noise = R.envelope(R.Net(rc, 7), {k: v.numpy() for k, v in sd.items()})
    err = float(np.abs(res["src_features"].double().cpu().numpy() - t64["final"]).max())
    print(f"fcgf envelope demo final: err {err:.3g} noise {noise['final']:.3g} ratio {err / noise['final']:.2f}")
    assert err <= ENVELOPE * noise["final"] + FEAT_FLOOR * float(np.abs(t64["final"]).max())
