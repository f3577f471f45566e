"""Parity on bench.py's own headline workload (run with -m gpu).

The bench's 128 pairs (N = 1000, pair g seeded 1000*100003 + g, trained synthetic
weights, 12 layers) through the batched forward at the bench's launch shape
(B = 128: the fused attention + pointwise-chain launches), both precision modes,
against the reference's own outputs on those pairs (tests/golden/bench_*.npz,
tools/gen_goldens.py run_bench).

  * bench_3dmatch_1k_tf -- the weights bench.py runs (classifier rescaled by
    synthetic.BENCH_CLS: every seed score positive).  Labels bit-exact on all 128
    pairs.  Poses within north_star's 1e-4, except where the seed list differs
    from the reference's: the trained network's logits span [-460, 10] before the
    rescale, and its fp32 noise (the reference's own distance from exact
    arithmetic) exceeds some seed-score gaps.  Such a pair must show (1) our logits
    within (ENVELOPE + 1) x the case's fp32 noise of the reference's, (2) a seed list
    that differs from the reference's only by near-ties of that size
    (conftest.assert_seeds_near_ties), and (3) a pose within 1e-4 of the oracle
    run on OUR seed list -- the stages after pick_seeds pinned exactly.
  * bench_3dmatch_1k -- the raw trained weights, whose logits are all negative on
    some pairs: there pick_seeds' ranking (models/PointDSC.py:216-217) is decided
    by the order of tied zero scores, which torch's argsort leaves arbitrary
    (SURVEY.md §7).  Labels are still bit-exact on all 128; poses are checked as
    above where the ranking is tie-free, and against the oracle (same tie rule as
    the kernels: descending score, ascending index) where it is not.

The same holds one stage later: the trained stand-in network maps a few hundred
correspondences of a pair onto practically one feature direction (their
pairwise kNN distances 2 - 2 f.f lie within ~5e-7, the fp32 resolution of that
expression), so a seed's 40 nearest neighbours are a near-tie choice among
them in the reference as in the kernels.  Step (3) therefore runs the oracle on
our seeds AND our kNN rows, after checking that the rows differ from the
oracle's own only by distances within 2e-6 (conftest.assert_knn_equivalent)."""
import numpy as np
import pytest
import torch

from conftest import (ENVELOPE, LOGIT_FLOOR, assert_knn_equivalent, assert_seeds_near_ties, fp32_envelope,
                      load_golden)
from parity_rules import NearTieTally

pytestmark = pytest.mark.gpu

POSE_ATOL = 1e-4


def _run(g, dev, precision, cls):
    from pointdsc_amd import kernels
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.synthetic import PRESETS, synthetic_pair, trained_state_dict
    preset = str(g["preset"])
    p = PRESETS[preset]
    P, N = int(g["pairs"]), int(g["num_corr"])
    m = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40, nms_radius=p["nms_radius"],
                 precision=precision)
    sd = trained_state_dict(preset, 12, *cls)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(dev).eval()
    ps = [synthetic_pair(N, int(g["pair_seed_base"]) + i, preset) for i in range(P)]
    data = {k: torch.from_numpy(np.stack([q[k] for q in ps])).to(dev) for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    with torch.no_grad():
        T, L = m.forward_batched(data["corr_pos"], data["src_keypts"], data["tgt_keypts"])
        # the same launch shape with every stage's output (pdsc_forward_testing_debug)
        st = kernels.forward_stages(m.pdsc_config(), m.packed_weights(), data["corr_pos"], data["src_keypts"],
                                    data["tgt_keypts"])
    assert torch.equal(T, st["final_trans"]) and torch.equal(L, st["final_labels"])
    st = {k: v.cpu().numpy() for k, v in st.items()}
    return T.cpu().numpy(), L.cpu().numpy(), st, ps, sd, p


def _pinned_downstream(i, st, ps, sd, p):
    """Our kNN rows vs the oracle's on our seeds (near-ties only), then the oracle
    on our seeds + kNN: labels equal, pose within 1e-4 of ours."""
    from oracle import pdsc_oracle as O
    pair = ps[i]
    r = O.forward_testing(pair["corr_pos"], pair["src_keypts"], pair["tgt_keypts"], sd, num_layers=12,
                          inlier_threshold=p["inlier_threshold"], nms_radius=p["nms_radius"],
                          seeds=st["seeds"][i], record=True)
    assert_knn_equivalent(st["knn"][i], r["knn_idx"], r["normed"], st["seeds"][i])
    r = O.forward_testing(pair["corr_pos"], pair["src_keypts"], pair["tgt_keypts"], sd, num_layers=12,
                          inlier_threshold=p["inlier_threshold"], nms_radius=p["nms_radius"],
                          seeds=st["seeds"][i], knn_idx=st["knn"][i])
    assert np.array_equal(st["final_labels"][i], r["final_labels"]), f"pair {i}"
    np.testing.assert_allclose(st["final_trans"][i], r["final_trans"], atol=POSE_ATOL,
                               err_msg=f"pair {i} (oracle on our seeds and kNN)")


def _explain(i, g, st, ps, sd, p, dev):
    """A pose farther than 1e-4 from the reference's is accepted only as a seed
    or kNN near-tie (module docstring)."""
    pair = ps[i]
    conf, seeds = st["conf"][i], st["seeds"][i].astype(np.int64)
    if not np.array_equal(seeds, g["seeds"][i]):
        case = {"src_keypts": pair["src_keypts"], "tgt_keypts": pair["tgt_keypts"], "corr_pos": pair["corr_pos"],
                "sigma_d": p["sigma_d"], "num_layers": 12, "nms_radius": p["nms_radius"],
                "corr_features": np.zeros((0, 128), np.float32), "confidence": g["confidence"][i],
                "is_local_max": g["is_local_max"][i].astype(np.float32), "seeds": g["seeds"][i].astype(np.int64)}
        tol = float(np.abs(conf - case["confidence"]).max())
        _, e_c, _, _, _ = fp32_envelope(case, sd, dev)
        assert tol <= (ENVELOPE + 1) * e_c + LOGIT_FLOOR, f"pair {i}: logit error {tol:.3g} vs fp32 noise {e_c:.3g}"
        assert_seeds_near_ties(seeds, conf, case, tol)
    _pinned_downstream(i, st, ps, sd, p)


@pytest.mark.parametrize("precision", ["h3", "f32"])
def test_bench_pairs_tie_free_weights(precision, gpu_device):
    from pointdsc_amd.synthetic import BENCH_CLS
    g = load_golden("bench_3dmatch_1k_tf")
    assert (float(g["cls_bias_shift"]), float(g["cls_scale"])) == BENCH_CLS
    assert int(g["n_nonpositive_seed_scores"].max()) == 0
    T, L, st, ps, sd, p = _run(g, gpu_device, precision, BENCH_CLS)
    assert np.array_equal(L.astype(np.uint8), g["final_labels"])
    d = np.abs(T - g["final_trans"]).reshape(len(T), -1).max(1)
    far = np.nonzero(d > POSE_ATOL)[0]
    assert len(far) <= 8, {int(i): float(d[i]) for i in far}
    for i in far:
        _explain(int(i), g, st, ps, sd, p, gpu_device)


@pytest.mark.parametrize("precision", ["h3", "f32"])
def test_bench_pairs_raw_weights(precision, gpu_device):
    from oracle import pdsc_oracle as O
    g = load_golden("bench_3dmatch_1k")
    T, L, st, ps, sd, p = _run(g, gpu_device, precision, ())
    assert np.array_equal(L.astype(np.uint8), g["final_labels"])
    tied = g["n_nonpositive_seed_scores"] > 0
    assert 0 < tied.sum() < len(tied)
    d = np.abs(T - g["final_trans"]).reshape(len(T), -1).max(1)
    for i in np.nonzero((d > POSE_ATOL) & ~tied)[0]:
        _explain(int(i), g, st, ps, sd, p, gpu_device)
    for i in np.nonzero(tied)[0]:
        # our tie rule, exactly: descending score conf * is_local_max, ascending index
        conf = st["conf"][i]
        sc = (conf * O.local_max(ps[i]["src_keypts"], conf, p["nms_radius"])).astype(np.float32)
        assert np.array_equal(st["seeds"][i], np.argsort(-sc, kind="stable")[:st["seeds"].shape[1]]), i
        _pinned_downstream(int(i), st, ps, sd, p)


def test_b65_both_attention_plans_vs_reference(gpu_device, capsys):
    """The first 65 bench pairs: 65 x 1000 leaves the fused plan for the
    64-query-wave split plan (pdsc_encoder_plan 2, two key splits per query
    block), where the uniform entry runs the stream-K attention and a ragged
    call with unequal padding runs the split grid -- two key partitions, two
    fp32 combine orders, so a pair's bits depend on the plan (round 5 measured
    poses 2.1e-4 apart, profiles/r05_ragged_halves_eq.log).  EACH plan is held
    to the reference's own outputs (tests/golden/bench_3dmatch_1k_tf.npz) by the
    rules above: labels bit-exact on all 65 pairs, poses within 1e-4 or the
    near-tie explanation (logits within the fp32 envelope, seeds / kNN rows
    different only by near-ties, the oracle on our seeds and kNN rows within
    1e-4).  The distances of both plans are printed for the record, and each
    plan's count of pairs that took the explanation (parity_rules.NearTieTally:
    65 pairs, at most 5)."""
    import ctypes
    from pointdsc_amd import _lib, kernels
    from pointdsc_amd.PointDSC import PointDSC
    from pointdsc_amd.synthetic import BENCH_CLS, PRESETS, synthetic_pair, trained_state_dict
    g = load_golden("bench_3dmatch_1k_tf")
    P, N = 65, int(g["num_corr"])
    plan = ctypes.c_int32()
    _lib.check(_lib.load().pdsc_encoder_plan(P, N, 0, ctypes.byref(plan)), "encoder_plan")
    assert plan.value == 2
    p = PRESETS[str(g["preset"])]
    m = PointDSC(in_dim=6, num_layers=12, num_channels=128, num_iterations=10, ratio=0.1,
                 inlier_threshold=p["inlier_threshold"], sigma_d=p["sigma_d"], k=40, nms_radius=p["nms_radius"])
    sd = trained_state_dict(str(g["preset"]), 12, *BENCH_CLS)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to(gpu_device).eval()
    ps = [synthetic_pair(N, int(g["pair_seed_base"]) + i, str(g["preset"])) for i in range(P)]
    data = {k: torch.from_numpy(np.stack([q[k] for q in ps])).to(gpu_device)
            for k in ("corr_pos", "src_keypts", "tgt_keypts")}
    cfg, pk = m.pdsc_config(), m.packed_weights()
    with torch.no_grad():
        uni = kernels.forward_stages(cfg, pk, data["corr_pos"], data["src_keypts"], data["tgt_keypts"])
        # the split grid: a ragged call padded to N + 1 rows (counts all N, not the padded N)
        pad = {k: torch.cat([v, torch.zeros_like(v[:, :1])], 1) for k, v in data.items()}
        T2, L2, st2 = kernels.forward_ragged(cfg, pk, pad["corr_pos"], pad["src_keypts"], pad["tgt_keypts"], [N] * P,
                                             debug=True)
    st2 = dict(st2, final_trans=T2, final_labels=L2[:, :N], conf=st2["conf"][:, :N])
    report = {}
    for name, st in (("stream-K (uniform entry)", uni), ("split grid (ragged entry)", st2)):
        st = {k: v.cpu().numpy() for k, v in st.items()}
        assert np.array_equal(st["final_labels"].astype(np.uint8), g["final_labels"][:P]), name
        d = np.abs(st["final_trans"] - g["final_trans"][:P]).reshape(P, -1).max(1)
        far = np.nonzero(d > POSE_ATOL)[0]
        tally = NearTieTally(f"test_b65_both_attention_plans_vs_reference, {name}")
        for i in range(P):
            tally.add(d[i], fallback=not d[i] <= POSE_ATOL)
        for i in far:
            _explain(int(i), g, st, ps, sd, p, gpu_device)
        tally.finish(capsys)
        assert tally.pairs == 65 and tally.cap == 5
        report[name] = {"max_pose_diff": float(d.max()), "pairs_past_1e-4": far.tolist()}
    dd = float((uni["final_trans"] - T2).abs().max())
    with capsys.disabled():
        print(f"\n[b65] vs reference: {report}; stream-K vs split grid max pose diff {dd:.3g}")
