"""bench.py's plain run and --dump-outputs: the plain run prints the headline
keys only (everything else is behind --full), and the dump holds the last timed
step's final_trans / final_labels as float32 .npy files, capped at 64 MB by a
fixed seeded sample."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
FULL_ONLY = ("roofline", "roofline_hbm", "roofline_path", "roofline_sm", "stages_ms", "single_pair", "ragged",
             "exact_f32", "cpu_baseline", "parity", "synthetic_recall")


def _bench_module():
    spec = importlib.util.spec_from_file_location("pdsc_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_small_arrays_whole(tmp_path):
    import torch
    bench = _bench_module()
    tr = torch.arange(2 * 16, dtype=torch.float32).reshape(2, 4, 4)
    lab = torch.ones((2, 7), dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"final_trans": tr, "final_labels": lab}, 0, 1)
    a, b = np.load(tmp_path / "d" / "final_trans.npy"), np.load(tmp_path / "d" / "final_labels.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, tr.numpy()) and np.array_equal(b, lab.numpy())


def test_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path, monkeypatch):
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 2 * 100)  # 100 float32 elements per array
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    small = torch.arange(100, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, 0, 1)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and np.array_equal(a, b)  # the same elements every run
    assert np.all(np.diff(a) > 0) and set(a.tolist()) <= set(range(1000))  # distinct elements of the array
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 4 * 2 * 100 + 2 * 128  # the arrays plus two .npy headers


def test_dump_outputs_names_ranks_apart(tmp_path):
    import torch
    bench = _bench_module()
    bench.dump_outputs(str(tmp_path), {"final_trans": torch.zeros((1, 4, 4))}, 1, 2)
    assert os.listdir(tmp_path) == ["final_trans_rank1.npy"]


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_last_step(tmp_path, gpu_device):
    """One plain run (4 pairs of N = 256, 3 timed steps): the headline keys and none of
    --full's; the dump equals a forward of the same pairs through the same plan."""
    import torch
    from pointdsc_amd import dist as pdist, kernels
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.synthetic import BENCH_CLS, PRESETS, synthetic_pair, trained_state_dict
    P, N = 4, 256
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--pairs", str(P), "--num-corr", str(N), "--dump-outputs", str(tmp_path / "out")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = lines[0]
    for k in HEADLINE:
        assert k in res, k
    assert not [k for k in FULL_ONLY if k in res]
    assert res["steps"] == 3 and res["warmup"] == 1 and res["higher_is_better"] is True
    assert res["unit"] == "correspondences/s" and res["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region (both are rounded in the line)
    assert res["value"] == pytest.approx(P * N / (res["ms_per_step"] * 1e-3), rel=1e-3)

    trans, labels = np.load(tmp_path / "out" / "final_trans.npy"), np.load(tmp_path / "out" / "final_labels.npy")
    assert trans.dtype == np.float32 and trans.shape == (P, 4, 4)
    assert labels.dtype == np.float32 and labels.shape == (P, N)
    # the same pairs (bench.py's seeds) and weights through the same entry point, in this process
    p = PRESETS["3dmatch"]
    model = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                     inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40, nms_radius=p["nms_radius"])
    sd = trained_state_dict("3dmatch", 12, *BENCH_CLS)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to(gpu_device).eval()
    ps = [synthetic_pair(N, 1000 * 100003 + g, "3dmatch") for g in pdist.shard_indices(P, 0, 1)]
    corr, src, tgt = (torch.from_numpy(np.stack([q[k] for q in ps])).to(gpu_device)
                      for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    plan = kernels.ForwardPlan(model.pdsc_config(), model.packed_weights(), P, N, gpu_device)
    t, l = plan.run(corr, src, tgt)
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(labels, l.cpu().numpy())
    assert np.array_equal(trans, t.cpu().numpy())  # the forward is deterministic: bitwise
