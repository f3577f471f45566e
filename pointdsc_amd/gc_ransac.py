"""GC-RANSAC on the GPU: the fork's ``--algo GC`` (algorithms/GC_RANSAC.py:8-50
from algorithms/FR.py:70-87) and the ``GCRANSAC`` baseline
(baseline_scripts/baseline_3DMatch.py:101-123) of AmnonDrory/PointDSC, on the
gfx950 kernels of ``libpdsc.so`` (include/pdsc.h, f10): the grid neighbourhood,
the graph-cut labelling -- exact per grid cell, one sort and one prefix sum --
and the solver around them (f6's sampler, Kabsch and scoring order).

The reference calls the x86 library ``pygcransac``, which is not a dependency
and whose source is not in the reference tree: the algorithm is restated from
the paper (Barath & Matas, CVPR 2018) in include/pdsc.h, which is the contract;
parity with the library itself is unpinned.  Left out: SPRT and edge-length
pre-emption, PROSAC, the FLANN neighbourhood; the local optimisation runs at
round granularity and refits by least squares over all labelled rows.

There is no CPU path: tensors must be HIP device tensors.
"""
from __future__ import annotations

from dataclasses import dataclass
from time import time

import torch

from . import _lib
from ._call import _p, call, read_struct, struct_buffer, trans_view
from .kernels import _dev

NEIGHBORHOOD_SIZE = 20  # GC_RANSAC.py:21


@dataclass
class GcRansacResult:
    """``transformation`` fp64 [4,4] (device): the least-squares fit over the
    inliers of the best model, its fp32 copy, ``labels`` [N] 0/1 and ``n_inliers``
    of that model, its MSAC ``score``; ``iterations`` hypotheses were drawn,
    ``best`` is the minimal hypothesis the result descends from (-1: none valid),
    ``lo_runs`` local optimisations ran ``lo_steps`` labelling steps in all over a
    grid of ``n_cells`` occupied cells.  ``debug``: dict of per-hypothesis
    ``samples`` [H,3], ``count`` [H], ``score`` [H], ``trans`` [H,4,4] on request."""
    transformation: torch.Tensor
    transformation_f32: torch.Tensor
    labels: torch.Tensor
    n_inliers: int
    score: float
    iterations: int
    best: int
    lo_runs: int
    lo_steps: int
    n_cells: int
    debug: dict | None = None


def gc_ransac_round() -> int:
    """Hypotheses per round (the granularity of the local optimisation and of the stop)."""
    return int(_lib.load().pdsc_gc_ransac_round())


def gc_cell_bounds():
    """(rows of a cell one wavefront labels, rows of a cell labelled in LDS)."""
    L = _lib.load()
    return int(L.pdsc_gc_cell_bound(0)), int(L.pdsc_gc_cell_bound(1))


def _pairs(src, tgt):
    src, tgt = _dev(src, "src"), _dev(tgt, "tgt")
    if src.dim() != 2 or src.shape[1] != 3 or tgt.shape != src.shape:
        raise ValueError(f"src {tuple(src.shape)} / tgt {tuple(tgt.shape)} must both be [N,3]")
    return src, tgt


def gc_grid(src: torch.Tensor, tgt: torch.Tensor, neighborhood_size: int = NEIGHBORHOOD_SIZE):
    """The grid neighbourhood of the correspondences (src[i], tgt[i]): ``order`` [N]
    (rows by (cell key, row)), ``cell_start`` [N+1] (the first n_cells + 1 entries
    are meaningful), ``cell_of`` [N] and ``n_cells`` [1], int32 device tensors.
    Two rows are neighbours iff they are in the same cell."""
    src, tgt = _pairs(src, tgt)
    n, dev = src.shape[0], src.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    cell_start = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    cell_of = torch.empty(n, dtype=torch.int32, device=dev)
    n_cells = torch.zeros(1, dtype=torch.int32, device=dev)
    call("pdsc_gc_grid", src, tgt, n, int(neighborhood_size), order, cell_start, cell_of, n_cells, device=dev,
         ws=("pdsc_gc_grid_workspace_bytes", n))
    return order, cell_start, cell_of, n_cells


def gc_label(pose: torch.Tensor, src: torch.Tensor, tgt: torch.Tensor, grid, threshold: float,
             spatial_coherence_weight: float, debug: bool = False):
    """The minimum of GC-RANSAC's energy under ``pose`` (fp64 [4,4] device tensor)
    over the grid of ``gc_grid``: ``(labels [N] 0/1 float, count [1] int32)``, with
    ``debug=True`` also a dict of ``d2`` [N] and per cell (capacity N) ``m_star``,
    ``energy``, ``energy_gap``."""
    src, tgt = _pairs(src, tgt)
    pose = _dev(pose, "pose", torch.float64)
    if pose.shape != (4, 4):
        raise ValueError(f"pose {tuple(pose.shape)} must be [4,4]")
    order, cell_start, _, n_cells = grid
    n, dev = src.shape[0], src.device
    if order.shape != (n,) or cell_start.shape != (n + 1,):
        raise ValueError("grid does not belong to these rows")
    labels = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    dbg = dstruct = None
    if debug:
        dbg = dict(d2=torch.zeros(n, dtype=torch.float64, device=dev),
                   m_star=torch.zeros(n, dtype=torch.int32, device=dev),
                   energy=torch.zeros(n, dtype=torch.float64, device=dev),
                   energy_gap=torch.zeros(n, dtype=torch.float64, device=dev))
        dstruct = _lib.PdscGcLabelDebug(*(_p(dbg[k]) for k in ("d2", "m_star", "energy", "energy_gap")))
    call("pdsc_gc_label", pose, src, tgt, n, order, cell_start, n_cells, float(threshold),
         float(spatial_coherence_weight), labels, count, dstruct, device=dev, ws=("pdsc_gc_label_workspace_bytes", n))
    return (labels, count, dbg) if debug else (labels, count)


def gc_ransac(src: torch.Tensor, tgt: torch.Tensor, threshold: float, spatial_coherence_weight: float = 0.975,
              max_iteration: int = 10000, confidence: float = 0.99, seed: int = 0, local_optimization: bool = True,
              neighborhood_size: int = NEIGHBORHOOD_SIZE, debug: bool = False) -> GcRansacResult:
    """pygcransac.findRigidTransform(src, tgt, threshold, conf, spatial_coherence_weight,
    max_iters, neighborhood=0, neighborhood_size) restated (include/pdsc.h, f10) on
    the current torch stream; src, tgt [N,3] fp32 device tensors, row i with row i.
    The keyword defaults are the library's.  Two calls with the same ``seed`` are
    bitwise equal."""
    src, tgt = _pairs(src, tgt)
    n, dev, H = src.shape[0], src.device, int(max_iteration)
    res = struct_buffer(_lib.PdscGcRansacResult, dev)
    t32 = torch.empty((4, 4), dtype=torch.float32, device=dev)
    labels = torch.empty(n, dtype=torch.float32, device=dev)
    dbg = dstruct = None
    if debug and H >= 1:
        dbg = dict(samples=torch.zeros((H, 3), dtype=torch.int32, device=dev),
                   count=torch.zeros(H, dtype=torch.int32, device=dev),
                   score=torch.zeros(H, dtype=torch.float64, device=dev),
                   trans=torch.zeros((H, 4, 4), dtype=torch.float64, device=dev))
        dstruct = _lib.PdscGcRansacDebug(*(_p(dbg[k]) for k in ("samples", "count", "score", "trans")))
    call("pdsc_gc_ransac", src, tgt, n, float(threshold), float(spatial_coherence_weight), int(neighborhood_size), H,
         float(confidence), int(seed) & (2 ** 64 - 1), 1 if local_optimization else 0, t32, labels, res, dstruct,
         device=dev, ws=("pdsc_gc_ransac_workspace_bytes", n))
    r = read_struct(res, _lib.PdscGcRansacResult)
    return GcRansacResult(trans_view(res), t32, labels, r.n_inliers, r.score, r.iterations, r.best, r.lo_runs,
                          r.lo_steps, r.n_cells, dbg)


def GC_RANSAC(A, B, distance_threshold, num_iterations, args, match_quality, seed=0):
    """algorithms/GC_RANSAC.py:8-50.  A, B [N,3] fp32 device tensors (row i with row
    i); ``args`` carries ``spatial_coherence_weight``, ``GC_conf``, ``GC_LO``,
    ``prosac``, ``use_edge_len`` and ``use_sprt``.  Returns the reference's
    ``(pose_T.T, elapsed_time)``: pygcransac returns the transposed pose and the
    reference transposes it back, so the first item is the source -> target [4,4]
    (device fp64 here).  ``prosac`` and ``use_edge_len`` are not implemented;
    ``use_sprt`` only saves CPU time in the library and is ignored;
    ``match_quality`` feeds PROSAC alone.  Fewer than 3 rows: the identity (the
    library returns no pose)."""
    if getattr(args, "prosac", False):
        raise NotImplementedError("GC-RANSAC: the PROSAC sampler (args.prosac) is not implemented")
    if getattr(args, "use_edge_len", False):
        raise NotImplementedError("GC-RANSAC: edge-length pre-emption (args.use_edge_len) is not implemented")
    A, B = _pairs(A, B)
    dev = A.device
    torch.cuda.synchronize(dev)
    start = time()
    if A.shape[0] < 3:
        T = torch.eye(4, dtype=torch.float64, device=dev)
    else:
        T = gc_ransac(A, B, distance_threshold, args.spatial_coherence_weight, num_iterations, args.GC_conf, seed,
                      bool(args.GC_LO)).transformation
    torch.cuda.synchronize(dev)
    return T, time() - start
