"""The PMC baseline on the GPU (include/pdsc.h f8, pointdsc_amd/csrc/clique.hip):
the consistency graph bit for bit against a numpy restatement of the
reference's loop (baseline_scripts/baseline_3DMatch.py:60-68), the maximum
clique against networkx, and baselines.PMC end to end.  The checkers share no
code with the library."""
import functools

import networkx as nx
import numpy as np
import pytest

from conftest import kabsch64
from pointdsc_amd.synthetic import synthetic_pair

pytestmark = pytest.mark.gpu

MODES = ("squared", "length")


# ------------------------------------------------------------------ checkers
def restated_diff(corr, mode):
    """|diff| [N,N] fp32 of baseline_3DMatch.py:66 -- np.sum of three fp32 squares
    is ((x + y) + z) -- and, for 'length', of the square roots of the two sums."""
    c = np.asarray(corr, np.float32)
    d = c[:, None, :] - c[None, :, :]
    q = d * d
    a = (q[..., 0] + q[..., 1]) + q[..., 2]
    b = (q[..., 3] + q[..., 4]) + q[..., 5]
    assert a.dtype == np.float32
    if mode == "length":
        a, b = np.sqrt(a), np.sqrt(b)
    return np.abs(a - b)


def restated_graph(corr, thr, mode):
    """bool [N,N]: the reference's compare in fp64 (numpy 1.x promotes the fp32
    scalar against the Python float), written out; no self loops."""
    e = restated_diff(corr, mode).astype(np.float64) < float(thr)
    np.fill_diagonal(e, False)
    return e


def reference_loop_graph(corr, thr):
    """The reference's double loop as written (squared mode), for a small N."""
    corr = np.asarray(corr, np.float32)
    n = len(corr)
    e = np.zeros((n, n), bool)
    for i in range(n):
        for j in range(i):
            diff = np.sum((corr[i][0:3] - corr[j][0:3]) ** 2) - np.sum((corr[i][3:] - corr[j][3:]) ** 2)
            if np.abs(diff).astype(np.float64) < thr:
                e[i, j] = e[j, i] = True
    return e


def to_bits(e):
    """bool [N,N] -> int64 [N, ceil(N/64)], bit j % 64 of word j // 64."""
    n = e.shape[0]
    W = (n + 63) // 64
    pad = np.zeros((n, W * 64), np.uint8)
    pad[:, :n] = e
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").astype(np.uint64).view(np.int64).reshape(n, W)


def from_bits(adj, n):
    b = np.unpackbits(np.ascontiguousarray(adj).view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
    return b[:, :n].astype(bool), b[:, n:]


def omega(e):
    return nx.max_weight_clique(nx.from_numpy_array(e), weight=None)[1]


def maximum_cliques(e):
    cl = list(nx.find_cliques(nx.from_numpy_array(e)))
    w = max(len(c) for c in cl)
    return [sorted(c) for c in cl if len(c) == w]


def rows(n, seed, dup=False):
    c = synthetic_pair(max(n, 8), seed)["corr_pos"][:n].copy()
    if dup and n >= 2:  # duplicated rows: diff exactly 0 against each other, equal rows of the graph
        c[n // 2:] = c[: n - n // 2]
    return c


# --------------------------------------------------------------------- graph
def run_graph(dev, corr, thr, mode):
    import torch
    from pointdsc_amd import kernels as K
    adj, deg = K.consistency_graph(torch.from_numpy(np.ascontiguousarray(corr, np.float32)).to(dev), thr, mode)
    return adj.cpu().numpy(), deg.cpu().numpy()


def check_graph(dev, corr, thr, mode):
    n = len(corr)
    want = restated_graph(corr, thr, mode)
    adj, deg = run_graph(dev, corr, thr, mode)
    assert adj.shape == (n, (n + 63) // 64) and adj.dtype == np.int64
    got, past = from_bits(adj, n)
    assert not past.any(), "bits past N"
    assert not got.diagonal().any(), "diagonal"
    assert np.array_equal(got, got.T), "symmetry"
    assert np.array_equal(adj, to_bits(want)), f"{(got != want).sum()} bits differ"
    assert deg.dtype == np.int32 and np.array_equal(deg, want.sum(1))
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 300])
def test_graph_bit_exact(gpu_device, n, mode):
    # the 3dmatch preset's threshold; in length mode also a wider one, so both sparse and dense words occur
    for thr in (0.10, 0.75) if mode == "length" else (0.10,):
        want = check_graph(gpu_device, rows(n, seed=n), thr, mode)
    if n >= 63:
        assert want.any() and not want[~np.eye(n, dtype=bool)].all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [2, 65, 129])
def test_graph_duplicated_rows(gpu_device, n, mode):
    c = rows(n, seed=5, dup=True)
    want = check_graph(gpu_device, c, 0.10, mode)
    h = n // 2
    assert all(want[i, i + h] for i in range(n - h - (n % 2)))  # |diff| = 0 < thr


def test_graph_follows_reference_loop(gpu_device):
    c = rows(65, seed=9)
    assert np.array_equal(restated_graph(c, 0.10, "squared"), reference_loop_graph(c, 0.10))
    check_graph(gpu_device, c, 0.10, "squared")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [65, 129])
def test_graph_diff_equal_to_fp32_threshold(gpu_device, n, mode):
    """Some |diff| equals float32(threshold) exactly.  For thr = v + 1e-9 with v an
    fp32 value, float32(thr) = v: an fp32 compare (v < v) leaves the edge out, the
    reference's fp64 compare (v < v + 1e-9) puts it in.  thr = v and v - 1e-9 are
    the other side: no edge either way."""
    v = 0.5625
    gap = 0.75 if mode == "squared" else 0.5625  # 0.75^2 = 0.5625; sqrt(0.5625^2) = 0.5625: all exact
    c = rows(n, seed=3)
    c[:8] = 0.0
    c[1:8:2, 0] = gap  # rows 1, 3, 5, 7 at x = gap, rows 0, 2, 4, 6 at the origin; targets coincide
    for thr in (v + 1e-9, v, v - 1e-9):
        assert np.float32(thr) == np.float32(v)
        d = restated_diff(c, mode)
        assert d[0, 1] == np.float32(thr) and (d[:8, :8] == np.float32(thr)).sum() == 32
        want = check_graph(gpu_device, c, thr, mode)
        f32 = d < np.float32(thr)
        np.fill_diagonal(f32, False)
        assert want[0, 1] == (thr > v)
        assert (want != f32).any() == (thr > v)  # where the two compares part ways


# -------------------------------------------------------------------- clique
def gnp(n, p, seed):
    return nx.to_numpy_array(nx.gnp_random_graph(n, p, seed=seed), dtype=bool, nodelist=range(n))


def planted(n, p, k, seed):
    e = gnp(n, p, seed)
    m = np.random.RandomState(seed).permutation(n)[:k]
    e[np.ix_(m, m)] = True
    np.fill_diagonal(e, False)
    return e


def two_cliques():
    e = np.zeros((20, 20), bool)
    e[2:9, 2:9] = True      # 7
    e[10:19, 10:19] = True  # 9
    np.fill_diagonal(e, False)
    return e


def matching_complement(n):
    e = np.ones((n, n), bool)
    np.fill_diagonal(e, False)
    for i in range(0, n, 2):
        e[i, i + 1] = e[i + 1, i] = False
    return e


GRAPHS = {
    "empty_70": lambda: np.zeros((70, 70), bool),
    "single_vertex": lambda: np.zeros((1, 1), bool),
    "K65": lambda: ~np.eye(65, dtype=bool),
    "two_cliques_7_9": two_cliques,
    "planted_9_in_G130_0.1": lambda: planted(130, 0.1, 9, 4),
    "G128_0.5": lambda: gnp(128, 0.5, 1),
    "G200_0.3": lambda: gnp(200, 0.3, 2),
    "matching_complement_64": lambda: matching_complement(64),
}
# the clique number where enumerating is hopeless: one vertex of each of the 32 non-adjacent pairs
KNOWN_OMEGA = {"matching_complement_64": 32}
UNIQUE = ("two_cliques_7_9", "planted_9_in_G130_0.1")


@functools.lru_cache(maxsize=None)
def graph_case(name):
    e = GRAPHS[name]()
    e.setflags(write=False)
    w = omega(e)
    assert w == KNOWN_OMEGA.get(name, w)
    return e, w


def run_clique(dev, e, **kw):
    import torch
    from pointdsc_amd import kernels as K
    members, labels, result = K.max_clique(torch.from_numpy(to_bits(e)).to(dev), **kw)
    return members.cpu().numpy(), labels.cpu().numpy(), K.CliqueInfo(result), result.cpu().numpy()


def assert_clique(e, members, labels, info):
    n = len(e)
    m = members[: info.size]
    assert info.size >= 1 and np.all(members[info.size:] == -1)
    assert np.all(np.diff(m) > 0) and m[0] >= 0 and m[-1] < n, m
    sub = e[np.ix_(m, m)]
    assert sub[~np.eye(len(m), dtype=bool)].all(), "members are not pairwise adjacent"
    want = np.zeros(n, np.float32)
    want[m] = 1
    assert labels.dtype == np.float32 and np.array_equal(labels, want)
    assert info.exact == int(info.roots_incomplete == 0)
    assert 1 <= info.heuristic_size <= info.size and info.nodes >= 0


@pytest.mark.parametrize("name", list(GRAPHS))
def test_max_clique(gpu_device, name):
    e, w = graph_case(name)
    members, labels, info, raw = run_clique(gpu_device, e)
    print(name, info)
    assert_clique(e, members, labels, info)
    assert info.exact == 1 and info.roots_incomplete == 0
    assert info.size == w
    if name in UNIQUE:
        best = maximum_cliques(e)
        assert len(best) == 1
        assert members[: info.size].tolist() == best[0]
    if not e.any():
        assert members[0] == 0  # (size, lower start vertex)
    m2, l2, _, raw2 = run_clique(gpu_device, e)
    assert np.array_equal(members, m2) and np.array_equal(labels, l2) and np.array_equal(raw, raw2)


@pytest.mark.parametrize("n,p,seed", [(60, 0.5, 0), (80, 0.5, 1), (80, 0.5, 3)])
def test_search_improves_on_the_lower_bound(gpu_device, n, p, seed):
    """Graphs on which the greedy lower bound (highest degree first, from every
    start) stops one short of the clique number, so the clique returned is one the
    search found and mapped back from its own vertex order."""
    e = gnp(n, p, seed)
    w = omega(e)
    members, labels, info, raw = run_clique(gpu_device, e)
    print(n, p, seed, info)
    assert_clique(e, members, labels, info)
    assert info.exact == 1 and info.size == w
    assert info.heuristic_size < info.size
    m2, l2, _, raw2 = run_clique(gpu_device, e)
    assert np.array_equal(members, m2) and np.array_equal(labels, l2) and np.array_equal(raw, raw2)


def test_max_clique_budget(gpu_device):
    e, w = graph_case("G200_0.3")
    members, labels, info, raw = run_clique(gpu_device, e, node_budget=1)
    print(info)
    assert_clique(e, members, labels, info)
    assert info.heuristic_size <= info.size <= w
    m2, l2, _, raw2 = run_clique(gpu_device, e, node_budget=1)
    assert np.array_equal(members, m2) and np.array_equal(labels, l2) and np.array_equal(raw, raw2)
    _, _, full, _ = run_clique(gpu_device, e)
    assert full.exact == 1 and full.size == w


def test_greedy_clique_is_the_lower_bound(gpu_device):
    e, w = graph_case("G128_0.5")
    members, labels, info, _ = run_clique(gpu_device, e, heuristic_only=True)
    assert info.exact == 0 and info.roots_incomplete == 0 and info.nodes == 0
    assert info.size == info.heuristic_size <= w
    m = members[: info.size]
    assert e[np.ix_(m, m)][~np.eye(len(m), dtype=bool)].all() and labels.sum() == info.size
    assert run_clique(gpu_device, e)[2].heuristic_size == info.size


def test_max_clique_two_words_per_lane(gpu_device):
    """N > 4096: a row is more than 64 words and every lane holds two.  Disjoint
    cliques laid across the word-64 boundary; the largest (40, vertices 4080 ..
    4119) is the unique maximum."""
    n = 4200
    e = np.zeros((n, n), bool)
    for lo, hi in ((4080, 4120), (10, 40), (4150, 4185)):
        e[lo:hi, lo:hi] = True
    np.fill_diagonal(e, False)
    members, labels, info, _ = run_clique(gpu_device, e)
    assert_clique(e, members, labels, info)
    assert info.exact == 1 and info.size == 40 and members[:40].tolist() == list(range(4080, 4120))


# ---------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def pair_case(seed, mode):
    p = synthetic_pair(256, seed)
    e = restated_graph(p["corr_pos"], 0.10, mode)
    return p, e, omega(e)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1])
def test_pmc_end_to_end(gpu_device, seed, mode):
    import torch
    from pointdsc_amd import PMC, kernels as K
    p, e, w = pair_case(seed, mode)
    corr, src, tgt = (torch.from_numpy(p[k][None]).to(gpu_device) for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    trans, labels, info = PMC(corr, src, tgt, inlier_threshold=0.10, mode=mode, return_info=True)
    print(seed, mode, info)
    assert trans.shape == (1, 4, 4) and trans.dtype == torch.float32
    assert labels.shape == (1, 256) and labels.dtype == torch.float32
    assert info.exact == 1 and info.size == w
    assert w == {("squared", 0): 45, ("squared", 1): 46, ("length", 0): 77, ("length", 1): 77}[(mode, seed)]
    lab = labels[0].cpu().numpy()
    m = np.nonzero(lab)[0]
    assert set(np.unique(lab)) <= {0.0, 1.0} and len(m) == w
    assert e[np.ix_(m, m)][~np.eye(w, dtype=bool)].all()
    assert torch.equal(trans, K.rigid_transform_3d(src, tgt, labels))
    t2, l2 = PMC(corr, src, tgt, inlier_threshold=0.10, mode=mode)
    assert torch.equal(t2, trans) and torch.equal(l2, labels)
    if mode == "length":
        assert np.array_equal(lab, p["gt_labels"])  # the planted inliers
        T64 = kabsch64(p["src_keypts"], p["tgt_keypts"], lab)
        assert np.abs(trans[0].cpu().numpy() - T64).max() <= 1e-4


@pytest.mark.parametrize("n", [1, 2])
def test_pmc_tiny(gpu_device, n):
    import torch
    from pointdsc_amd import PMC
    p = synthetic_pair(8, 0)
    corr, src, tgt = (torch.from_numpy(p[k][None, :n].copy()).to(gpu_device)
                      for k in ("corr_pos", "src_keypts", "tgt_keypts"))
    for mode in MODES:
        trans, labels, info = PMC(corr, src, tgt, inlier_threshold=1e6, mode=mode, return_info=True)
        assert trans.shape == (1, 4, 4) and labels.shape == (1, n)
        assert info.exact == 1 and info.size == n and labels.sum().item() == n  # every pair consistent
        assert torch.isfinite(trans).all()
        _, labels, info = PMC(corr, src, tgt, inlier_threshold=1e-30, mode=mode, return_info=True)
        assert info.size == 1 and labels[0].tolist() == [1.0] + [0.0] * (n - 1)
