"""correspondence construction (mutual NN in descriptor
space, labels, centred corr_pos) -- the HIP path (pointdsc_amd.correspondence,
C ABI pdsc_build_correspondences) against the oracle's restatement of
datasets/ThreeDMatch.py:285-308.

Parity note: the loader module imports open3d (absent), so the oracle is the
reference's numpy expressions restated, not a reference run ("parity unpinned"
by goldens).  Bars: nearest-neighbour indices exact up to fp32 near-ties of the
descriptor distance (the GPU's FMA order differs from BLAS sgemm); given the
same correspondence list, keypoints and corr_pos bit-exact (the column mean
restates numpy's sequential fp32 axis-0 sum), labels exact away from the
threshold (|d - tau| > 1e-9)."""
import numpy as np
import pytest
import torch

from front_reference import CORR_ORACLE_SEEDS
from oracle import pdsc_oracle as O


def _pair(Ns, Nt, D, seed, overlap=0.6, noise=0.05, dups=0):
    rng = np.random.RandomState(seed)
    src = (rng.rand(Ns, 3) * 3).astype(np.float32)
    th = rng.rand() * np.pi
    ax = rng.randn(3)
    ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = R, rng.rand(3)
    sd = rng.randn(Ns, D).astype(np.float32)
    sd /= np.linalg.norm(sd, axis=1, keepdims=True)
    tgt = (rng.rand(Nt, 3) * 3).astype(np.float32)
    td = rng.randn(Nt, D).astype(np.float32)
    m = min(int(overlap * min(Ns, Nt)), Nt)
    perm = rng.permutation(Nt)[:m]
    tgt[perm] = (src[:m] @ R.T + gt[:3, 3] + 0.01 * rng.randn(m, 3)).astype(np.float32)
    td[perm] = sd[:m] + noise * rng.randn(m, D).astype(np.float32)
    if dups:  # exact descriptor ties: first index must win
        td[Nt - dups:] = td[perm[0]]
        sd[Ns - dups:] = sd[0]
    td /= np.linalg.norm(td, axis=1, keepdims=True)
    return src, tgt, sd, td.astype(np.float32), gt


def test_oracle_mean_is_numpy_sequential_fp32():
    """corr_pos centring: numpy's float32 axis-0 mean is a sequential fp32 sum
    divided in float64 -- the semantics corr_gather_kernel restates."""
    rng = np.random.RandomState(1)
    for n in (7, 1000, 5000):
        x = (rng.rand(n, 6) * 50).astype(np.float32)
        s = np.zeros(6, np.float32)
        for r in range(n):
            s = (s + x[r]).astype(np.float32)
        assert np.array_equal(x.mean(0), (s.astype(np.float64) / n).astype(np.float32))


def test_oracle_mutual_structure():
    src, tgt, sd, td, gt = _pair(400, 350, 32, 3)
    r = O.build_correspondences(src, tgt, sd, td, gt_trans=gt)
    c = r["corr"]
    assert np.all(np.diff(c[:, 0]) > 0)  # np.where order
    assert np.all(r["target_idx"][c[:, 1]] == c[:, 0])
    assert r["labels"].mean() > 0.5  # the planted overlap is recovered
    assert np.allclose(r["corr_pos"].mean(0), 0, atol=1e-4)


def _t(x, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)


def _nn_equivalent(ours, ref, dist, axis, eps=2e-6):
    """Indices equal, or the chosen entries' distances within eps (near-ties)."""
    ours, ref = np.asarray(ours), np.asarray(ref)
    bad = np.nonzero(ours != ref)[0]
    for i in bad:
        a = dist[i, ours[i]] if axis == 1 else dist[ours[i], i]
        b = dist[i, ref[i]] if axis == 1 else dist[ref[i], i]
        assert abs(float(a) - float(b)) <= eps, (i, a, b)
    return len(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("Ns,Nt,D,dups", [(300, 257, 32, 0), (2000, 1500, 33, 0), (5000, 5000, 32, 0),
                                          (1000, 1200, 32, 40), (64, 1, 16, 0), (20000, 18000, 32, 0)])
def test_mutual_nn_vs_oracle(Ns, Nt, D, dups, gpu_device):
    from pointdsc_amd.correspondence import mutual_nn
    src, tgt, sd, td, gt = _pair(Ns, Nt, D, Ns + Nt, dups=dups)
    r = O.build_correspondences(src, tgt, sd, td)
    si, ti = mutual_nn(_t(sd, gpu_device), _t(td, gpu_device))
    si, ti = si.cpu().numpy(), ti.cpu().numpy()
    nbad = _nn_equivalent(si, r["source_idx"], r["distance"], 1) + _nn_equivalent(ti, r["target_idx"], r["distance"], 0)
    assert nbad <= max(2, (Ns + Nt) // 1000)
    if dups:  # identical descriptors tie exactly: the first index wins, as in numpy.argmin
        assert np.array_equal(si[Ns - dups:], r["source_idx"][Ns - dups:])


@pytest.mark.gpu
@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("Ns,Nt", [(1000, 900), (5000, 5000)])
def test_build_correspondences_vs_oracle(Ns, Nt, mutual, gpu_device):
    """The _pair seeds are chosen (front_reference.CORR_ORACLE_SEEDS) so that every row's
    and column's nearest neighbour leads its runner-up by >= 1e-5 in 2 - 2 dot
    (tests/test_front_reference.py asserts it): fp32 reordering moves a dot by ~2e-6,
    so the list IS the oracle's and the bit-exact checks always run."""
    from pointdsc_amd.correspondence import build_correspondences
    src, tgt, sd, td, gt = _pair(Ns, Nt, 32, CORR_ORACLE_SEEDS[Ns, Nt])
    ref = O.build_correspondences(src, tgt, sd, td, use_mutual=mutual, gt_trans=gt, inlier_threshold=0.10)
    out = build_correspondences(_t(src, gpu_device), _t(tgt, gpu_device), _t(sd, gpu_device), _t(td, gpu_device),
                                use_mutual=mutual, gt_trans=gt, inlier_threshold=0.10)
    corr = out["corr"].cpu().numpy()
    assert corr.shape == ref["corr"].shape and np.array_equal(corr, ref["corr"])
    assert np.array_equal(out["src_keypts"].cpu().numpy(), ref["src_keypts"])
    assert np.array_equal(out["tgt_keypts"].cpu().numpy(), ref["tgt_keypts"])
    assert np.array_equal(out["corr_pos"].cpu().numpy(), ref["corr_pos"])
    lab = out["labels"].cpu().numpy()
    far = np.abs(ref["label_distance"] - 0.10) > 1e-9
    assert np.array_equal(lab[far], ref["labels"][far])
    if mutual:
        assert lab.mean() > 0.5


@pytest.mark.gpu
def test_correspondences_feed_forward(gpu_device):
    """End to end: descriptors -> correspondences -> PointDSC forward recovers the
    planted transform (the evaluation loaders' data path on the GPU)."""
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.correspondence import build_correspondences
    from pointdsc_amd.synthetic import trained_state_dict
    src, tgt, sd, td, gt = _pair(1500, 1500, 32, 11, overlap=0.5)
    out = build_correspondences(_t(src, gpu_device), _t(tgt, gpu_device), _t(sd, gpu_device), _t(td, gpu_device),
                                gt_trans=gt)
    model = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                     inlier_threshold=0.10, sigma_d=0.10, k=40, nms_radius=0.10)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in trained_state_dict("3dmatch", 12).items()})
    model = model.to(gpu_device).eval()
    data = {"corr_pos": out["corr_pos"][None], "src_keypts": out["src_keypts"][None],
            "tgt_keypts": out["tgt_keypts"][None], "testing": True}
    with torch.no_grad():
        res = model(data)
    T = res["final_trans"][0].cpu().numpy()
    assert np.linalg.norm(T[:3, 3] - gt[:3, 3]) < 0.3
