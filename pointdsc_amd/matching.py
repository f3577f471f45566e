"""The fork's correspondence filters (algorithms/matching.py of
AmnonDrory/PointDSC) on the gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f7):
second nearest neighbours in feature space, the mutual / best-buddy filter
(MFR), the 1st / 2nd distance ratio and the Grid-Prioritized Filter (GPF).  The
functions keep the reference's names, argument orders and int64 index tensors;
tensors live on the device and the choices the reference leaves open are fixed
as include/pdsc.h states them (ties to the lower index, the unstable argsort,
max == min in the normalisation).

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from time import time

import torch

from . import _lib
from ._call import _p, _workspace, call, query
from .kernels import _dev


def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (there is no CPU fallback)")
    return t.to(torch.int32).contiguous()


def _feats(F0, F1):
    F0, F1 = _dev(F0, "feats0"), _dev(F1, "feats1")
    if F0.dim() != 2 or F1.dim() != 2 or F0.shape[1] != F1.shape[1]:
        raise ValueError(f"feats0 {tuple(F0.shape)} / feats1 {tuple(F1.shape)} must be [n,D] with one D")
    return F0, F1


def nn2(F0: torch.Tensor, F1: torch.Tensor, split: int | None = None):
    """pdsc_nn2: (nn1 [N0], nn2 [N0], rev [N1]) int32 device tensors.  split: the
    column split per row stripe through pdsc_nn2_split (tests; the result does
    not depend on it)."""
    F0, F1 = _feats(F0, F1)
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    ws = ("pdsc_nn2_workspace_bytes", n0, n1)
    a = torch.empty(n0, dtype=torch.int32, device=dev)
    b = torch.empty(n0, dtype=torch.int32, device=dev)
    r = torch.empty(n1, dtype=torch.int32, device=dev)
    if split is None:
        call("pdsc_nn2", F0, F1, n0, n1, d, a, b, r, device=dev, ws=ws)
    else:
        call("pdsc_nn2_split", F0, F1, n0, n1, d, int(split), a, b, r, device=dev, ws=ws)
    return a, b, r


def match_ratio(F0, F1, idx1, idx1_2nd, rev=None):
    """pdsc_match_ratio: (feat_dist [N0], is_bb [N0] int32, norm [N0], num_bb
    device int32 [1]); with rev None only feat_dist (the others None)."""
    F0, F1 = _feats(F0, F1)
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    dev = F0.device
    a, b = _i32(idx1, "corres_idx1"), _i32(idx1_2nd, "idx1_2nd")
    if a.shape != (n0,) or b.shape != (n0,):
        raise ValueError("one first and one second neighbour per row of feats0")
    fd = torch.empty(n0, dtype=torch.float32, device=dev)
    is_bb = norm = num = None
    if rev is not None:
        rev = _i32(rev, "rev")
        if rev.shape != (n1,):
            raise ValueError("rev must have one entry per row of feats1")
        is_bb = torch.empty(n0, dtype=torch.int32, device=dev)
        norm = torch.empty(n0, dtype=torch.float32, device=dev)
        num = torch.empty(1, dtype=torch.int32, device=dev)
    call("pdsc_match_ratio", F0, F1, n0, n1, d, a, b, rev, is_bb, fd, norm, num, device=dev)
    return fd, is_bb, norm, num


def gpf_select(xyz0, norm, num_bb, grid_wid: int, factor: float, debug: bool = False):
    """pdsc_gpf_select: (kept rows int32 [count] ascending, their norm, debug
    dict or None).  Reads the count back (one synchronisation)."""
    xyz0, norm = _dev(xyz0, "xyz0"), _dev(norm, "norm_feat_dist")
    n0, g = xyz0.shape[0], int(grid_wid)
    dev = xyz0.device
    kept = torch.empty(n0, dtype=torch.int32, device=dev)
    kn = torch.empty(n0, dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    dbg = dstruct = None
    if debug and 1 <= g <= 64:
        dbg = dict(cell=torch.empty(n0, dtype=torch.int32, device=dev),
                   max_per_quad=torch.empty(g * g, dtype=torch.int32, device=dev),
                   per_quad=torch.empty(g * g, dtype=torch.float64, device=dev),
                   height=torch.empty(1, dtype=torch.float64, device=dev))
        dstruct = _lib.PdscGpfDebug(*(_p(dbg[k]) for k in ("cell", "max_per_quad", "per_quad", "height")))
    call("pdsc_gpf_select", xyz0, norm, _i32(num_bb, "num_bb"), n0, g, float(factor), kept, cnt, kn, dstruct,
         device=dev, ws=("pdsc_gpf_select_workspace_bytes", n0, g))
    n = int(cnt.item())
    return kept[:n], kn[:n], dbg


def refit_inliers(T, src, tgt, radius: float):
    """pdsc_refit_inliers (FR.py:101-114): (trans fp64 [4,4], trans fp32 [4,4],
    count device int32 [1], labels [N]) for the pose T over the pairs src[i],
    tgt[i]; fewer than 3 inliers: T itself."""
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    if src.shape != tgt.shape or src.dim() != 2 or src.shape[1] != 3:
        raise ValueError(f"src {tuple(src.shape)} / tgt {tuple(tgt.shape)} must both be [n,3]")
    dev = src.device
    T = _dev(T.to(dev), "T", torch.float64).reshape(16)
    out = torch.empty((4, 4), dtype=torch.float64, device=dev)
    o32 = torch.empty((4, 4), dtype=torch.float32, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    labels = torch.empty(src.shape[0], dtype=torch.float32, device=dev)
    call("pdsc_refit_inliers", T, src, tgt, src.shape[0], float(radius), out, o32, cnt, labels, device=dev)
    return out, o32, cnt, labels


# ------------------------------------------------------- the reference's names
def find_nn(F0, F1, return_2nd=False):
    """matching.py:22-65: (corres_idx0 = arange(N0), corres_idx1, idx1_2nd or
    None), int64 device tensors.  A single target row (N1 = 1) is every row's
    neighbour and needs no kernel; a second neighbour, find_2nn and the mutual
    filters need N1 >= 2 (pdsc_nn2)."""
    F0, F1 = _feats(F0, F1)
    if F1.shape[0] == 1 and not return_2nd:
        idx0 = torch.arange(F0.shape[0], dtype=torch.int64, device=F0.device)
        return idx0, torch.zeros_like(idx0), None
    a, b, _ = nn2(F0, F1)
    idx0 = torch.arange(a.shape[0], dtype=torch.int64, device=a.device)
    return idx0, a.long(), (b.long() if return_2nd else None)


def _find_2nn(F0, F1):
    """find_2nn plus rev (the reverse nearest neighbours the filters need)."""
    F0, F1 = _feats(F0, F1)
    dev = F0.device
    n0, n1, d = F0.shape[0], F1.shape[0], F0.shape[1]
    nb = query("pdsc_mutual_nn_workspace_bytes", n0, n1)
    ws = _workspace(nb, dev)  # allocated outside the timed span
    s = torch.empty(n0, dtype=torch.int32, device=dev)
    t = torch.empty(n1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    t0 = time()  # the first neighbours alone: what a pipeline without second neighbours pays
    call("pdsc_mutual_nn", F0, F1, n0, n1, d, s, t, device=dev, ws=(ws, nb))
    torch.cuda.synchronize(dev)
    t1 = time()
    a, b, rev = nn2(F0, F1)
    torch.cuda.synchronize(dev)
    t2 = time()
    idx0 = torch.arange(n0, dtype=torch.int64, device=dev)
    return idx0, a.long(), b.long(), (t2 - t1) - (t1 - t0), rev


def find_2nn(fcgf_feats0, fcgf_feats1):
    """matching.py:6-19: (corres_idx0, corres_idx1, idx1_2nd, the additional time
    of finding the second neighbours).  The time is that of pdsc_nn2 minus that
    of a first-neighbour search (pdsc_mutual_nn), each with the stream
    synchronised around it."""
    return _find_2nn(fcgf_feats0, fcgf_feats1)[:4]


def _mutual_mask(feats0, feats1, corres_idx0, corres_idx1, rev=None):
    if rev is None:
        rev = nn2(feats0, feats1)[2]
    return rev.long()[corres_idx1] == corres_idx0


def nn_to_mutual(feats0, feats1, corres_idx0, corres_idx1, idx1_2nd=None, force_return_2nd=False, _rev=None):
    """matching.py:225-242: the pairs (i, j) with i the nearest row of feats0 to
    row j of feats1 too, in ascending i (the order torch's coalesce gives the
    reference)."""
    m = _mutual_mask(feats0, feats1, corres_idx0, corres_idx1, _rev)
    i0, i1 = corres_idx0[m], corres_idx1[m]
    if idx1_2nd is not None:
        return i0, i1, idx1_2nd[i0]  # as the reference: corres_idx0 is the full range
    if force_return_2nd:
        return i0, i1, None
    return i0, i1


def mark_best_buddies(fcgf_feats0, fcgf_feats1, corres_idx0, corres_idx1):
    """matching.py:210-223: (is_bb bool device tensor, num_bb int)."""
    m = _mutual_mask(fcgf_feats0, fcgf_feats1, corres_idx0, corres_idx1)
    return m, int(m.sum().item())


def calc_distance_ratio_in_feature_space(fcgf_feats0, fcgf_feats1, corres_idx0, corres_idx1, idx1_2nd):
    """matching.py:89-98: distance to the first over distance to the second
    neighbour (+ 1e-6), fp32 device tensor."""
    f0 = _dev(fcgf_feats0, "feats0")[corres_idx0]
    return match_ratio(f0, fcgf_feats1, corres_idx1, idx1_2nd)[0]


def Grid_Prioritized_Filter(fcgf_feats0, fcgf_feats1, corres_idx0, corres_idx1, idx1_2nd, xyz0, args, BB_first=False,
                            _rev=None):
    """matching.py:100-208: (corres_idx0, corres_idx1, idx1_2nd of the kept pairs,
    the three inputs, norm_feat_dist of the kept pairs).  corres_idx0 must be the
    full range 0 .. N0-1, as the reference assumes.

    BB_first=False (FR's form): every pair is a candidate, best buddies first,
    the total is GPF_factor * num_bb.  BB_first=True (TEASER's form, :112-116):
    only the mutual pairs are candidates; all of them are returned (with None for
    norm_feat_dist) when args.GPF_max_matches >= their number -- one host read, as
    in the reference -- else the grid keeps GPF_max_matches of them, ranked by the
    distance ratio normalised over the mutual pairs, without the best-buddy offset."""
    n0 = fcgf_feats0.shape[0]
    if corres_idx0.shape[0] != n0 or not torch.equal(corres_idx0, torch.arange(n0, device=corres_idx0.device,
                                                                               dtype=corres_idx0.dtype)):
        raise ValueError("corres_idx0 must be the full range 0 .. N0-1 of feats0's rows")
    rev = _rev if _rev is not None else nn2(fcgf_feats0, fcgf_feats1)[2]
    if BB_first:
        total = int(args.GPF_max_matches)
        i0, i1, i2 = nn_to_mutual(fcgf_feats0, fcgf_feats1, corres_idx0, corres_idx1, idx1_2nd, force_return_2nd=True,
                                  _rev=rev)
        if total >= i0.shape[0]:
            return i0, i1, i2, corres_idx0, corres_idx1, idx1_2nd, None
        fd = match_ratio(_dev(fcgf_feats0, "feats0")[i0], fcgf_feats1, i1, i2)[0]
        m, M = fd.min(), fd.max()
        norm = torch.where(M > m, (fd - m) / (M - m), torch.zeros_like(fd))  # max == min: 0, as pdsc_match_ratio
        num = torch.full((1,), total, dtype=torch.int32, device=fd.device)
        kept, kept_norm, _ = gpf_select(_dev(xyz0, "xyz0")[i0], norm, num, args.GPF_grid_wid, 1.0)
        k = kept.long()
        return i0[k], i1[k], i2[k], corres_idx0, corres_idx1, idx1_2nd, kept_norm
    _, _, norm, num_bb = match_ratio(fcgf_feats0, fcgf_feats1, corres_idx1, idx1_2nd, rev)
    kept, kept_norm, _ = gpf_select(_dev(xyz0, "xyz0")[corres_idx0], norm, num_bb, args.GPF_grid_wid, args.GPF_factor)
    k = kept.long()
    return (corres_idx0[k], corres_idx1[k], idx1_2nd[k] if idx1_2nd is not None else None, corres_idx0, corres_idx1,
            idx1_2nd, kept_norm)


def measure_inlier_ratio(corres_idx0, corres_idx1, pcd0, pcd1, T_gt, voxel_size):
    """matching.py:244-252 with [n,3] device tensors for the point clouds: the
    share of pairs with |T_gt p0 - p1|^2 < (2 voxel_size)^2, in fp64."""
    if corres_idx0.numel() == 0:
        return float("nan")  # the reference divides 0 by 0
    T = torch.as_tensor(T_gt, dtype=torch.float64).to(pcd0.device)
    p0 = pcd0.double()[corres_idx0] @ T[:3, :3].T + T[:3, 3]
    d2 = ((p0 - pcd1.double()[corres_idx1]) ** 2).sum(1)
    return float((d2 < (2 * voxel_size) ** 2).sum().item()) / d2.shape[0]
