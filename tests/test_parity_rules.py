"""tests/parity_rules.py on the CPU: the near-tie rule accepts the oracle's own
outputs and a legitimate near-tie, and rejects a logit error, a seed ranking and
a kNN row that the old `1e-3 * max|logit|` fallback let through; the fallback
cap.  One N = 300 pair with the bench classifier (synthetic.BENCH_CLS)."""
import numpy as np
import pytest
import torch

import parity_rules as PR

HP = {"num_layers": 12}
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def ref():
    """The pair, its weights and the oracle's recorded run (read-only)."""
    from oracle import pdsc_oracle as O
    from pointdsc_amd.synthetic import BENCH_CLS, synthetic_pair, trained_state_dict
    sd = trained_state_dict("3dmatch", 12, *BENCH_CLS)
    pair = synthetic_pair(300, 500003)
    r = O.forward_testing(pair["corr_pos"], pair["src_keypts"], pair["tgt_keypts"], sd, record=True, **HP)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pair, sd, r


def _downstream(pair, sd, seeds):
    """The oracle's own result on a given seed list: (labels, pose, kNN rows)."""
    from oracle import pdsc_oracle as O
    r = O.forward_testing(pair["corr_pos"], pair["src_keypts"], pair["tgt_keypts"], sd, seeds=seeds, record=True, **HP)
    return r["final_labels"], r["final_trans"], r["knn_idx"]


def test_oracle_outputs_are_exact(ref):
    pair, sd, r = ref
    tally = PR.NearTieTally("oracle vs itself")
    how = PR.held_to_oracle(pair, r["final_labels"], r["final_trans"], r["confidence"], r["seeds"], r["knn_idx"], sd,
                            CPU, tally=tally, **HP)
    assert how == "exact" and (tally.pairs, tally.fallbacks, tally.max_dist) == (1, 0, 0.0)
    # ... and the strict rule itself holds on them, every step run
    fig = PR.explain_near_tie(pair, r["final_labels"], r["final_trans"], r["confidence"], r["seeds"], r["knn_idx"],
                              sd, CPU, **HP)
    assert fig["tol"] == 0.0 and fig["seeds_moved"] == 0


def test_logit_error_inside_the_old_bound_is_rejected(ref):
    pair, sd, r = ref
    conf = r["confidence"].copy()
    conf[0] += np.float32(5e-3)
    err = float(np.abs(conf.astype(np.float64) - r["confidence"]).max())
    # what the old rule let through: 5e-3 is inside 1e-3 * max(1, max|logit|) ...
    assert 4.9e-3 < err <= 1e-3 * max(1.0, float(np.abs(r["confidence"]).max()))
    bound, _ = PR.logit_bound(pair, sd, CPU, **HP)
    assert bound < 1e-4 < err  # ... and hundreds of strict bounds wide
    with pytest.raises(AssertionError, match=r"logit error 0\.005\d* past the bound"):
        PR.explain_near_tie(pair, r["final_labels"], r["final_trans"], conf, r["seeds"], r["knn_idx"], sd, CPU, **HP)


def test_wrong_seed_ranking_is_rejected(ref):
    pair, sd, r = ref
    seeds = r["seeds"].copy()
    S = len(seeds)
    score = (r["confidence"] * r["is_local_max"]).astype(np.float64)
    rest = np.setdiff1d(np.arange(len(score)), seeds)
    seeds[:S // 2] = rest[np.argsort(score[rest], kind="stable")[:S // 2]]  # the lowest-scoring unchosen points
    labels, trans, knn = _downstream(pair, sd, seeds)
    with pytest.raises(AssertionError, match="seed scores increase by more than 2 tol"):
        PR.explain_near_tie(pair, labels, trans, r["confidence"], seeds, knn, sd, CPU, **HP)


def test_legitimate_near_tie_is_accepted(ref):
    from oracle import pdsc_oracle as O
    pair, sd, r = ref
    n = len(r["confidence"])
    bound, _ = PR.logit_bound(pair, sd, CPU, **HP)
    noise = np.random.RandomState(1).uniform(-1, 1, n) * 0.45 * bound
    conf = (r["confidence"].astype(np.float64) + noise).astype(np.float32)
    assert 0 < np.abs(conf.astype(np.float64) - r["confidence"]).max() <= 0.5 * bound
    seeds, _ = O.pick_seeds(pair["src_keypts"], conf, 0.10, len(r["seeds"]))
    assert (seeds != r["seeds"]).sum() >= 1  # this pair: the noise swaps a near-tie in the ranking
    labels, trans, knn = _downstream(pair, sd, seeds)
    fig = PR.explain_near_tie(pair, labels, trans, conf, seeds, knn, sd, CPU, **HP)
    assert fig["seeds_moved"] == (seeds != r["seeds"]).sum() and fig["tol"] <= 0.5 * bound


def test_wrong_knn_row_is_rejected(ref):
    pair, sd, r = ref
    knn = r["knn_idx"].copy()
    f = r["normed"].astype(np.float64)
    d = 2.0 - 2.0 * (f[r["seeds"][0]] @ f.T)
    j = int(np.argmax(d))  # the point farthest from seed 0 in feature space, in place of its last neighbour
    assert j not in knn[0] and d[j] - d[knn[0]].max() > 2e-6
    knn[0, -1] = j
    with pytest.raises(AssertionError, match="kNN rows not the oracle's up to distance near-ties"):
        PR.explain_near_tie(pair, r["final_labels"], r["final_trans"], r["confidence"], r["seeds"], knn, sd, CPU,
                            **HP)


@pytest.mark.parametrize("pairs,cap", [(4, 1), (5, 1), (8, 2), (65, 5), (128, 8), (130, 9)])
def test_tally_cap(pairs, cap):
    assert PR.fallback_cap(pairs) == cap
    for extra in (0, 1):
        tally = PR.NearTieTally(f"tally {pairs}")
        for i in range(pairs):
            tally.add(1e-5 if i >= cap + extra else 2e-4, fallback=i < cap + extra)
        assert (tally.pairs, tally.fallbacks, tally.cap, tally.max_dist) == (pairs, cap + extra, cap, 2e-4)
        if extra:
            with pytest.raises(AssertionError,
                               match=f"{cap + 1} near-tie fallbacks exceed the cap {cap} of {pairs} pairs"):
                tally.finish()
        else:
            tally.finish()


def test_measured_cap_never_above_half():
    tally = PR.NearTieTally("measured cap", cap=3)
    for i in range(5):
        tally.add(0.0, fallback=False)
    with pytest.raises(AssertionError, match="cap 3 above half of 5 pairs"):
        tally.finish()
