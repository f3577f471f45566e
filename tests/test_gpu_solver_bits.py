"""RANSAC, the inlier refit and GC-RANSAC, bit for bit against a recording
(tests/golden/solver_bits/solver_bits.json).

The other GPU files hold these stages to fp64 references within tolerances.
This one holds them to themselves: every output byte of a fixed set of calls --
the fp64 and fp32 poses, the labels, the whole result struct and, with the
debug rows on, every hypothesis's sample, count, score and pose -- must equal
what an earlier build of the same sources produced.  That is the property a
refactor of the solver code relies on ("two builds, same bits"): both solvers
are fp64 without contraction in a fixed order with total orders on the
hypotheses, so nothing but a change of the arithmetic can move a bit.

The recording holds the result struct's bytes and a SHA-256 per output (the
debug rows of a 16385-hypothesis call are megabytes).  It is tied to the
toolchain: a different compiler may contract, reassociate or schedule libm
differently.  Only a commit that MEANS to change the solvers' numerics, or a
ROCm update, re-records it: `python tests/test_gpu_solver_bits.py --write` on
the GPU (PDSC_LIB_VARIANT selects the build to record from).

The cases are the smallest that reach every branch: row counts around the
256-row scoring chunk, hypothesis counts around the 256-hypothesis workgroup
and the 16384-hypothesis round (16385: a second round of one hypothesis), both
sample sizes, the edge checker off and on, the refit off and on, the
confidence stop off, on and stopping after the first round; the refit with
fewer than three rows and with fewer than three inliers; GC-RANSAC with one
cell holding every row at the sizes of its three cell paths (one wave up to 64
rows, LDS up to 1024, global scratch above), a 4^6 grid, the local
optimisation off and on.

Every call with a result struct also records ``fields``: the scalars its Python
wrapper hands out (the RansacResult / GcRansacResult / RegistrationResult
dataclasses, CliqueInfo, GncInfo, TeaserInfo), floats as hex -- what the
wrapper reads back from the struct must not move either.  The ICP, clique
(exact and greedy), GNC-TLS rotation and TEASER calls are there for that: one
call each on 64 rows.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ransac_reference as R  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "solver_bits", "solver_bits.json")
ROUND = R.ROUND

# (N, max_iteration, ransac_n, edge_similarity, refit, confidence): every value of every axis occurs
RANSAC_CASES = [
    (3, 1, 3, 0.0, 0, 1.0),
    (4, 255, 4, 0.9, 1, 1.0),
    (255, 256, 3, 0.9, 0, 1.0),
    (256, 257, 4, 0.0, 1, 1.0),
    (257, ROUND, 3, 0.0, 1, 1.0),
    (1000, ROUND + 1, 4, 0.9, 0, 1.0),
    (1000, ROUND + 1, 3, 0.0, 1, 0.999),
    ("early", 2 * ROUND, 3, 0.0, 0, 0.999),  # R.EARLY["dense"]: stops after round 0
]
# (N, pose): "true" the generating motion (every row an inlier), "far" a pose under which none is
REFIT_CASES = [(1, "true"), (2, "true"), (3, "true"), (257, "true"), (257, "far")]
# (N, G, max_iteration, confidence, local_optimization)
GC_CASES = [(N, 1, 2048, 1.0, lo) for N in (3, 64, 65, 1024, 1025) for lo in (0, 1)] + [
    (1000, 4, 2048, 1.0, 0), (1000, 4, 2048, 1.0, 1), (1000, 4, ROUND + 1, 1.0, 1), (1000, 4, ROUND + 1, 0.999, 0),
    (1000, 4, ROUND + 1, 0.999, 1)]


def _pair(N):
    if N == "early":
        n, ratio, _, data_seed, _ = R.EARLY["dense"]
        return R.make_case(data_seed, n, ratio)[:2]
    return R.stage_inputs(N)


def _bytes(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()


def _entry(outputs, struct, fields=None):
    """outputs: name -> device tensor; struct: the result struct's tensor (or None);
    fields: the object whose int / float attributes the wrapper read from the struct."""
    e = {k: hashlib.sha256(_bytes(v)).hexdigest() for k, v in outputs.items()}
    if struct is not None:
        e["struct"] = _bytes(struct).hex()
    if fields is not None:
        names = getattr(fields, "__slots__", None) or list(vars(fields))
        vals = {k: getattr(fields, k) for k in names}
        e["fields"] = {k: v.hex() if type(v) is float else v for k, v in vals.items() if type(v) in (int, float)}
    return e


def _struct(r):
    """The 160-byte result struct: r.transformation is a view of its first 16 doubles."""
    import torch
    return torch.as_strided(r.transformation, (20,), (1,), 0)


def run_ransac(dev, case):
    import torch
    from pointdsc_amd.ransac import registration_ransac_based_on_correspondence as ransac
    N, H, ns, es, refit, conf = case
    src, tgt = (torch.from_numpy(a).to(dev) for a in _pair(N))
    r = ransac(src, tgt, None, 0.1, ransac_n=ns, edge_similarity=es, max_iteration=H, confidence=conf, seed=7,
               refit=bool(refit), debug=True)
    debug = {"debug_" + k: v for k, v in r.debug.items()}
    return _entry(dict(trans=r.transformation, trans_f32=r.transformation_f32, labels=r.labels, **debug), _struct(r),
                  r)


def run_refit(dev, case):
    import torch
    from pointdsc_amd.matching import refit_inliers
    N, pose = case
    src, tgt, true, _ = R.make_case(2000 + N, N, 1.0)
    T = true.copy()
    if pose == "far":
        T[:3, 3] += 100.0
    out, o32, cnt, labels = refit_inliers(torch.from_numpy(T).to(dev), torch.from_numpy(src).to(dev),
                                          torch.from_numpy(tgt).to(dev), 0.1)
    return _entry(dict(trans=out, trans_f32=o32, count=cnt, labels=labels), None)


def run_gc(dev, case):
    import torch
    from pointdsc_amd.gc_ransac import gc_ransac
    N, G, H, conf, lo = case
    src, tgt = (torch.from_numpy(a).to(dev) for a in R.make_case(3000 + N, N, 0.3)[:2])
    r = gc_ransac(src, tgt, 0.1, 0.975, max_iteration=H, confidence=conf, seed=7, local_optimization=bool(lo),
                  neighborhood_size=G, debug=True)
    debug = {"debug_" + k: v for k, v in r.debug.items()}
    return _entry(dict(trans=r.transformation, trans_f32=r.transformation_f32, labels=r.labels, **debug), _struct(r),
                  r)


# the calls whose result struct only the wrapper's read-back pins: 64 rows each
INFO_CASES = [("icp",), ("clique", "exact"), ("clique", "greedy"), ("gnc",), ("teaser",)]


def run_info(dev, case):
    import torch
    from pointdsc_amd import kernels as K
    kind = case[0]
    src, tgt, true, _ = R.make_case(4000 + len(kind), 64, 1.0 if kind == "icp" else 0.6)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    if kind == "icp":
        from pointdsc_amd.icp import registration_icp
        init = true.copy()
        init[:3, 3] += 0.05
        r = registration_icp(s, t, 0.2, torch.from_numpy(init).to(dev), want_correspondences=True)
        return _entry(dict(trans=r.transformation, trans_f32=r.transformation_f32, correspondence=r.correspondence),
                      None, r)
    if kind == "clique":
        adj, degree = K.consistency_graph(torch.cat([s, t], 1), 0.05, "length")
        members, labels, result = K.max_clique(adj, heuristic_only=case[1] == "greedy")
        return _entry(dict(adj=adj, degree=degree, members=members, labels=labels), result, K.CliqueInfo(result))
    if kind == "gnc":
        a, b = (s[1:] - s[:-1]).double(), (t[1:] - t[:-1]).double()
        Rm, w, inl, info = K.gnc_tls_rotation(a, b, 0.05)
        return _entry(dict(R=Rm, weights=w, inliers=inl), info, K.GncInfo(info))
    trans, t32, labels, result = K.teaser_solve(s, t, 0.05)
    return _entry(dict(trans=trans, trans_f32=t32, labels=labels), result, K.TeaserInfo(result))


GROUPS = {"ransac": (RANSAC_CASES, run_ransac), "refit": (REFIT_CASES, run_refit), "gc": (GC_CASES, run_gc),
          "info": (INFO_CASES, run_info)}


def _key(group, case):
    return group + ":" + ",".join(str(v) for v in case)


ALL = [(g, c) for g, (cases, _) in GROUPS.items() for c in cases]


@pytest.fixture(scope="module")
def recording():
    with open(FIXTURE) as f:
        return json.load(f)


def test_recording_lists_these_cases(recording):
    assert sorted(recording) == sorted(_key(g, c) for g, c in ALL)


@pytest.mark.gpu
@pytest.mark.parametrize("group,case", ALL, ids=[_key(g, c) for g, c in ALL])
def test_solver_bits(gpu_device, recording, group, case):
    got, want = GROUPS[group][1](gpu_device, case), recording[_key(group, case)]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    print(_key(group, case), "differing outputs:", bad or "none")
    assert not bad, f"{_key(group, case)}: {bad} differ from the recording"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        import torch
        dev = torch.device("cuda:0")
        table = {_key(g, c): GROUPS[g][1](dev, c) for g, c in ALL}
        path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path, len(table), "cases")
    else:
        sys.exit("usage: test_gpu_solver_bits.py --write [PATH]")
