"""pointdsc_amd -- MI355X-native (gfx950) PointDSC spatial-consistency + NSM hot path.

``pointdsc_amd.PointDSC.PointDSC`` is the drop-in for the reference's
``models.PointDSC.PointDSC``; ``pointdsc_amd.kernels`` exposes each hot-path op;
``pointdsc_amd.icp`` refines a pose by point-to-point ICP (the drivers' "+ICP"
row); the C ABI is ``include/pdsc.h`` / ``pointdsc_amd/libpdsc.so``.
"""
__version__ = "0.1.0"

__all__ = ["icp_refine", "registration_icp"]


def __getattr__(name):  # the ICP entry points, without importing torch on `import pointdsc_amd`
    if name in __all__:
        from . import icp
        return getattr(icp, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
