"""CPU checks of tests/gc_reference.py, the yardstick of tests/test_gpu_gc.py: the
per-cell prefix minimiser of include/pdsc.h (f10) equals a brute force over all
2^n labellings, and every case the GPU tests compare exactly is free of
near-ties on the reference alone (the condition selects the seeds; it widens no
tolerance)."""
import numpy as np
import pytest

import gc_reference as G

LAMBDAS = (0.0, 0.1, 0.975, 1.0)


def _check_cell(K, lam):
    K = np.sort(np.asarray(K, np.float64))[::-1]  # ascending d2 = descending K
    m, e, gap = G.cell_minimise(K, lam)
    best, ms = G.brute_force(K, lam)
    assert abs(e - best) <= 1e-12 * max(1.0, abs(best)), (K, lam, e, best)
    assert gap >= 0.0
    L = np.zeros(len(K), np.int64)
    L[:m] = 1
    assert abs(G.labelling_energy(K, L, lam) - best) <= 1e-12 * max(1.0, abs(best))
    if gap > 1e-9:
        assert ms == [m], (K, lam, m, ms)
    else:
        assert m in ms  # a tie to rounding: any of the minimisers (exact ties: test_singleton_ties_go_to_the_lower_m)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_prefix_minimiser_equals_brute_force_random(lam):
    rng = np.random.RandomState(int(lam * 1000))
    for _ in range(40):
        n = int(rng.randint(1, 10))
        _check_cell(np.exp(-rng.rand(n) * rng.choice([0.3, 3.0, 30.0])), lam)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_prefix_minimiser_adversarial(lam):
    for n in (1, 2, 5, 9):
        for k in (0.0, 0.25, 0.5, 0.75, 1.0):  # equal residuals, K = 1/2 among them
            _check_cell(np.full(n, k), lam)
    _check_cell([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], lam)       # clean inliers and clean outliers
    _check_cell([0.51, 0.5, 0.49, 0.5, 0.5], lam)          # everything at the unary break-even
    _check_cell([0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.1], lam)  # one outlier among inliers
    _check_cell([0.9, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1], lam)  # one inlier among outliers
    _check_cell([1e-300, 1.0 - 1e-16, 0.5], lam)


def test_singleton_ties_go_to_the_lower_m():
    assert G.cell_minimise([0.99], 1.0)[0] == 0 and G.cell_minimise([0.99], 1.0)[2] == 0.0
    assert G.cell_minimise([0.99], 0.5)[0] == 1 and G.cell_minimise([0.01], 0.5)[0] == 0
    assert G.cell_minimise([0.5], 0.0)[0] == 0


def test_energy_margin_stands_clear_of_the_measured_envelope():
    env = G.measure_envelope(cells=40, trials=3, seed=1)
    print("one-ulp envelope (40 cells):", env)
    assert 0.0 < env <= 1.6e-16 * 4  # the file's figure (300 cells) with room for another draw
    assert G.ENERGY_MARGIN >= 1e5 * env


def test_grid_reference_shapes():
    for name in [*G.GRID_SHAPES, "flat_axis", "far_outlier"]:
        src, tgt, g = G.grid_inputs(name)
        ref = G.gc_grid(src, tgt, g)
        N = len(src)
        assert sorted(ref["order"]) == list(range(N)) and ref["cell_start"][0] == 0 and ref["cell_start"][-1] == N
        assert len(ref["cell_start"]) == ref["n_cells"] + 1 and ref["cell_of"].max() == ref["n_cells"] - 1
        for a, b in ((i, j) for i in range(0, N, 37) for j in range(0, N, 41)):
            assert (ref["cell_of"][a] == ref["cell_of"][b]) == (ref["key"][a] == ref["key"][b])
    assert G.gc_grid(*G.grid_inputs((1000, 1)))["n_cells"] == 1
    far = G.gc_grid(*G.grid_inputs("far_outlier"))
    sizes = np.diff(far["cell_start"])
    assert sizes.max() >= 50 and far["n_cells"] >= 2  # the outlier squeezes the others together


@pytest.mark.parametrize("name", sorted(G.LABEL_CASES))
@pytest.mark.parametrize("lam", G.LABEL_LAMBDAS)
def test_label_cases_are_tie_free(name, lam):
    grid, ref = G.label_reference(name, lam)
    print(name, lam, "cells", grid["n_cells"], "count", ref["count"], ref["diag"])
    assert G.label_tie_free(ref["diag"])
    if name.startswith("one_cell"):
        assert grid["n_cells"] == 1
    if lam <= 0.0005 and name != "identical_8" or name == "clustered_1000":
        assert 0 < ref["count"] < len(ref["labels"])  # the case exercises both labels


def test_label_cases_cover_the_split():
    sizes = {G.LABEL_CASES[k][0] for k in G.LABEL_CASES if k.startswith("one_cell")}
    for b in (G.WAVE_CELL, G.LDS_CELL):
        assert {b - 1, b, b + 1} <= sizes
    grid, _ = G.label_reference("clustered_1000", 0.1)
    n = np.diff(grid["cell_start"])
    assert n.min() == 1 and (n > G.WAVE_CELL).any() and ((n > 1) & (n <= G.WAVE_CELL)).any()


def test_stage_case_is_tie_free():
    ref = G.stage_reference()
    print(ref["diag"], ref["best"], ref["lo_runs"], ref["lo_steps"])
    assert G.tie_free(ref["diag"]) and ref["best"] >= 0 and (ref["count"] == -1).any()


@pytest.mark.parametrize("name", sorted(G.WHOLE_CASES))
@pytest.mark.parametrize("lo", [False, True])
def test_whole_cases_are_tie_free(name, lo):
    ref = G.whole_reference(name, lo)
    print(name, lo, ref["diag"], ref["best"], ref["score"], ref["n_inliers"], ref["lo_runs"], ref["lo_steps"])
    assert G.tie_free(ref["diag"]) and ref["best"] >= 0
    assert ref["score"] >= ref["best_minimal_score"]
    if lo:
        assert ref["lo_runs"] >= 1 and ref["lo_steps"] >= ref["lo_runs"]
    else:
        assert ref["lo_runs"] == 0 and ref["lo_steps"] == 0 and ref["n_cells"] == 0


def test_early_case_stops_after_round_0():
    e = G.EARLY
    src, tgt = G.solver_inputs(G.WHOLE_N, e["ratio"], e["data_seed"])
    ref = G.gc_ransac(src, tgt, G.EPS, G.WHOLE_LAMBDA, G=G.WHOLE_G, max_iteration=e["rounds"] * G.ROUND,
                      confidence=e["confidence"], seed=e["seed"], lo=True, rows=False)
    assert ref["iterations"] == G.ROUND and G.tie_free(ref["diag"]) and len(ref["diag"]["stop"]) == 1
