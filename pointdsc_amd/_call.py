"""The one call path from torch tensors to the C ABI of ``libpdsc.so``.

Every ABI function that takes a workspace ends in ``(void *ws, size_t ws_bytes,
pdsc_stream_t stream)`` and every other device entry point in ``stream``
(include/pdsc.h; tests/test_lib.py holds both to the header), so one helper can
append them: ``call`` resolves the function, turns tensors into pointers,
queries and allocates the workspace, passes torch's current stream and raises
through ``_lib.check``.  Result structs the kernels write into device memory
are allocated by ``struct_buffer`` and read back by ``read_struct``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def query(name: str, *args, required: bool = False) -> int:
    """A ``*_workspace_bytes`` (or other size) query.  required: 0 means the
    configuration is unsupported and pdsc_last_error says why."""
    L = _lib.load()
    n = getattr(L, name)(*args)
    if required and n == 0:
        raise RuntimeError(f"unsupported configuration: {L.pdsc_last_error().decode()}")
    return n


def call(name: str, *args, device, ws=None, stream=None):
    """``name(*args[, ws pointer, ws bytes][, stream])`` on the loaded library.

    args: tensors become their device pointers and None NULL; a ctypes struct
    goes by reference where the prototype takes a pointer to it.
    ws: ``(query_name, *query_args)`` -- the size query is called and a uint8
    workspace allocated on ``device`` -- or a caller-kept ``(tensor, nbytes)``.
    device: whose current stream the call runs on; None for the host-only entry
    points, which take no stream.  stream: a torch stream instead of the current."""
    L = _lib.load()
    a = [ctypes.c_void_p(x.data_ptr()) if isinstance(x, torch.Tensor) else x for x in args]
    if ws is not None:
        buf, nb = ws[0], ws[1]
        if not isinstance(buf, torch.Tensor):
            nb = getattr(L, buf)(*ws[1:])
            buf = _workspace(nb, device)
        a += (ctypes.c_void_p(buf.data_ptr()), nb)
    if stream is not None:
        a.append(ctypes.c_void_p(stream.cuda_stream))
    elif device is not None:
        a.append(_stream(device))
    _lib.check(getattr(L, name)(*a), name)


def struct_buffer(struct_type, device) -> torch.Tensor:
    """Device memory for one ``struct_type`` the kernels write: uint8 [sizeof]."""
    return torch.empty(ctypes.sizeof(struct_type), dtype=torch.uint8, device=device)


def read_struct(t: torch.Tensor, struct_type):
    """The struct a ``struct_buffer`` holds, on the host (one synchronising copy)."""
    return struct_type.from_buffer_copy(t.cpu().numpy().tobytes())


def trans_view(buf: torch.Tensor) -> torch.Tensor:
    """The leading ``double trans[16]`` of a result struct as a device fp64 [4,4] view."""
    return buf[:ctypes.sizeof(ctypes.c_double * 16)].view(torch.float64).view(4, 4)
