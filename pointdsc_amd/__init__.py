"""pointdsc_amd -- MI355X-native (gfx950) PointDSC spatial-consistency + NSM hot path.

``pointdsc_amd.PointDSC.PointDSC`` is the drop-in for the reference's
``models.PointDSC.PointDSC``; ``pointdsc_amd.kernels`` exposes each hot-path op;
``pointdsc_amd.icp`` refines a pose by point-to-point ICP (the drivers' "+ICP"
row); ``pointdsc_amd.ransac`` is RANSAC on correspondences (the drivers' RANSAC
baseline and ``--solver RANSAC``); ``pointdsc_amd.matching`` / ``pointdsc_amd.fr``
are the fork's correspondence filters (MFR, GPF) and its filtered RANSAC ``FR``;
``pointdsc_amd.baselines`` holds the baselines ``SM``, ``RANSAC`` and ``PMC``
(consistency graph + maximum clique); ``pointdsc_amd.teaser`` is the fork's
``TEASER`` (graph, clique, GNC-TLS rotation, TLS translation);
``pointdsc_amd.gc_ransac`` is its ``GC`` (GC-RANSAC on the grid neighbourhood, the
exact per-cell graph cut; ``GCRANSAC`` is the baseline); ``pointdsc_amd.multiway``
is multiway registration around the forward (information matrix, multi-scale ICP,
pose-graph optimisation with loop-closure pruning, ATE); the C ABI is ``include/pdsc.h`` /
``pointdsc_amd/libpdsc.so``.
"""
__version__ = "0.1.0"

_ICP = ("icp_refine", "registration_icp")
_RANSAC = ("registration_ransac_based_on_correspondence", "ransac_solver")
_MATCHING = ("find_nn", "find_2nn", "nn_to_mutual", "mark_best_buddies", "calc_distance_ratio_in_feature_space",
             "Grid_Prioritized_Filter", "measure_inlier_ratio", "refit_inliers")
_FR = ("FR",)
_PMC = ("PMC",)
_TEASER = ("TEASER",)
_GC = ("GC_RANSAC", "gc_grid", "gc_label")  # the solver itself: pointdsc_amd.gc_ransac.gc_ransac (the module's name)
_GCRANSAC = ("GCRANSAC",)
__all__ = [*_ICP, *_RANSAC, *_MATCHING, *_FR, *_PMC, *_TEASER, *_GC, *_GCRANSAC]


def __getattr__(name):  # the ICP / RANSAC / FR / PMC / TEASER / GC entry points, without importing torch on `import pointdsc_amd`
    if name in _TEASER:
        from . import teaser
        return getattr(teaser, name)
    if name in _GC:
        from . import gc_ransac
        return getattr(gc_ransac, name)
    if name in _PMC or name in _GCRANSAC:
        from . import baselines
        return getattr(baselines, name)
    if name in _MATCHING:
        from . import matching
        return getattr(matching, name)
    if name in _FR:
        from . import fr
        return getattr(fr, name)
    if name in _ICP:
        from . import icp
        return getattr(icp, name)
    if name in _RANSAC:
        from . import ransac
        return getattr(ransac, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
