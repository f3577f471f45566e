"""Every host-only workspace size query of the solver, descriptor and matching
stages, replayed against a recorded table
(tests/golden/workspace/workspace_table.npz) -- no GPU needed.

A caller allocates what `pdsc_*_workspace_bytes` reports and the launcher
carves exactly that much, so the numbers are ABI-visible: a slice added,
dropped, resized or re-aligned shows here as a differing row.  The shapes
straddle the 256-byte alignment, the 256-row chunks of the RANSAC and ICP
partials, the in-LDS limits and the range guards that make a query return 0
(those zeros are part of the table).

`python tests/test_workspace_table.py --write` records the table from the
built library; only a commit whose workspace layouts are MEANT to change
should do that.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "workspace", "workspace_table.npz")

NS = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 8192, 8193, 16384, 262144, 262145)
ICP = tuple(itertools.product((1, 256, 257, 1000), repeat=2))
NN2 = tuple(itertools.product((1, 64, 257), (1, 2, 130)))
GPF_G = (1, 10, 64, 65)
MAX_NN = (1, 30, 100)
PAIRS = ((1, 1), (2, 3), (8, 100), (64, 500), (3, 5000))  # (B, N) / (B, S) / (Ns, Nt) of the small forward-stage queries

# name -> the argument tuples it is tabulated at
QUERIES = {
    "pdsc_ransac_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_gc_grid_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_gc_label_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_gc_ransac_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_gpf_select_workspace_bytes": tuple(itertools.product(NS, GPF_G)),
    "pdsc_nn2_workspace_bytes": NN2 + tuple((n, n) for n in NS),
    "pdsc_icp_workspace_bytes": ICP + tuple((n, n) for n in NS),
    "pdsc_radius_knn_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_voxel_down_sample_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_estimate_normals_workspace_bytes": tuple(itertools.product(NS, MAX_NN)),
    "pdsc_compute_fpfh_workspace_bytes": tuple(itertools.product(NS, MAX_NN)),
    "pdsc_max_clique_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_tls_translation_workspace_bytes": tuple((n,) for n in NS),
    "pdsc_teaser_solve_workspace_bytes": tuple((n,) for n in NS),
    # the small sums of the forward's stand-alone stages
    "pdsc_mutual_nn_workspace_bytes": PAIRS,
    "pdsc_seed_hypotheses_workspace_bytes": PAIRS,
    "pdsc_spectral_matching_loss_workspace_bytes": PAIRS + ((0, 5), (5, 0)),
    "pdsc_spectral_matching_workspace_bytes": tuple((n,) for n in NS[:16]),
    "pdsc_seed_knn_workspace_bytes": tuple((b, n, max(1, n // 10)) for b, n in PAIRS),
}


def record():
    """name -> int64 [len(QUERIES[name])] from the loaded library."""
    sys.path.insert(0, os.path.dirname(HERE))
    from pointdsc_amd import _lib
    lib = _lib.load()
    return {name: np.array([getattr(lib, name)(*a) for a in args], np.int64) for name, args in QUERIES.items()}


def test_workspace_table_matches_recording():
    got = record()
    with np.load(FIXTURE, allow_pickle=False) as z:
        assert sorted(k[5:] for k in z.files if k.startswith("args:")) == sorted(QUERIES)
        for name, args in QUERIES.items():
            assert z["args:" + name].tolist() == [list(a) for a in args], name
            want = z["size:" + name]
            bad = np.flatnonzero(got[name] != want)
            rows = [(args[i], int(got[name][i]), int(want[i])) for i in bad[:5]]
            assert not len(bad), f"{name}: {len(bad)} shapes differ; (args, got, want): {rows}"


def test_workspace_table_reaches_the_guards():
    """The recording holds both zeros (a range guard) and sizes for every guarded query."""
    with np.load(FIXTURE, allow_pickle=False) as z:
        for name in ("pdsc_gc_grid_workspace_bytes", "pdsc_gc_label_workspace_bytes", "pdsc_gc_ransac_workspace_bytes",
                     "pdsc_gpf_select_workspace_bytes", "pdsc_nn2_workspace_bytes", "pdsc_max_clique_workspace_bytes",
                     "pdsc_tls_translation_workspace_bytes", "pdsc_teaser_solve_workspace_bytes"):
            size = z["size:" + name]
            assert (size == 0).any() and (size > 0).any(), name
        for name in QUERIES:
            assert (z["size:" + name] % 256 == 0).all(), name


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        table = record()
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        np.savez_compressed(FIXTURE, **{"size:" + k: v for k, v in table.items()},
                            **{"args:" + k: np.array(v, np.int64) for k, v in QUERIES.items()})
        print("wrote", FIXTURE, {k: int((v > 0).sum()) for k, v in table.items()})
    else:
        sys.exit("usage: test_workspace_table.py --write")
