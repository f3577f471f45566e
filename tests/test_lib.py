"""libpdsc.so loads and exports the C ABI of include/pdsc.h; host-side logic
(argument checks, parameter order, workspace queries) -- no GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pointdsc_amd import _lib
from pointdsc_amd.synthetic import state_dict_keys


def header_functions():
    src = open(os.path.join(ROOT, "include", "pdsc.h")).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(pdsc_[a-z_0-9]+)\s*\(", src, re.M)))


def test_library_exports_every_header_symbol():
    lib = _lib.load()
    names = header_functions()
    assert len(names) >= 20, names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/pdsc.h but not exported"
    assert set(names) == set(_lib.EXPORTS)


# ------------------------------------------------- include/pdsc.h against _lib.py
P = ctypes.POINTER
# C type -> ctypes.  Scalars (function parameters, return types and struct fields):
SCALARS = {
    "int32_t": ctypes.c_int32,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "size_t": ctypes.c_size_t,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "pdsc_stream_t": ctypes.c_void_p,
}
# Pointers: `const char *` -> c_char_p, `const pdsc_config *` -> CFG, a pointer to
# pdsc_X_debug -> POINTER(PdscXDebug) or c_void_p, every other data pointer ->
# c_void_p, but for the host pointers ctypes fills or reads in place:
HOST_POINTERS = {
    ("pdsc_pack_weights", "params_host_array"): P(ctypes.c_void_p),
    ("pdsc_attention_layout", "Npad"): P(ctypes.c_int32),
    ("pdsc_attention_layout", "nsplit"): P(ctypes.c_int32),
    ("pdsc_encoder_plan", "fused"): P(ctypes.c_int32),
    ("pdsc_encoder_plan_vfold", "vfold"): P(ctypes.c_int32),
    ("pdsc_launch_plan", "out"): P(ctypes.c_int32),
    ("pdsc_packed_block", "offsets"): P(ctypes.c_size_t),
    ("pdsc_attention_timing", "start_events"): P(ctypes.c_void_p),
    ("pdsc_attention_timing", "stop_events"): P(ctypes.c_void_p),
    ("pdsc_attention_timing", "count"): P(ctypes.c_int32),
    ("pdsc_forward_timing", "events"): P(ctypes.c_void_p),
    ("pdsc_forward_timing", "count"): P(ctypes.c_int32),
    ("pdsc_forward_testing_ragged", "counts"): P(ctypes.c_int32),
    ("pdsc_ply_read_xyz", "n_points"): P(ctypes.c_int64),
    ("pdsc_range_status", "flags"): P(ctypes.c_int32),
}


def _struct_class(c_name):
    """pdsc_gc_ransac_result -> _lib.PdscGcRansacResult (None if _lib has no mirror)."""
    return getattr(_lib, "".join(w.capitalize() for w in c_name.split("_")), None)


def _declarator(text):
    """'const float *const *tensors' / 'size_t offsets[5]' -> (base type, pointer depth, name, array length)."""
    m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(\d+)\])?", text.strip(), re.S)
    assert m, text
    kind = m.group(1).replace("const", " ")
    return " ".join(kind.replace("*", " ").split()), kind.count("*"), m.group(2), int(m.group(3)) if m.group(3) else None


def parse_header():
    """include/pdsc.h -> (structs {name: [(field, base, depth, array length)]},
    functions {name: (return declarator, [parameter declarators])}).  Every
    statement of the header is a typedef, an enum or a prototype: anything else
    fails here, so no declaration is skipped silently."""
    src = open(os.path.join(ROOT, "include", "pdsc.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    src = src.replace('extern "C" {', "")
    structs = {}

    def take_struct(m):
        assert m.group(1) == m.group(3), m.group(0)
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            first, *rest = decl.split(",")
            base, depth, name, arr = _declarator(first)
            fields.append((name, base, depth, arr))
            for r in rest:  # `double fitness, inlier_rmse;`
                _, d2, n2, a2 = _declarator("x " + r)
                fields.append((n2, base, d2, a2))
        structs[m.group(1)] = fields
        return ""

    src = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^}]*)\}\s*(\w+)\s*;", take_struct, src)
    src = re.sub(r"enum\s+\w+\s*\{[^}]*\}\s*;", "", src)
    src = re.sub(r"typedef\s+void\s*\*\s*pdsc_stream_t\s*;", "", src)
    functions = {}
    for stmt in filter(None, (s.strip() for s in src.split(";"))):
        if stmt == "}":  # closes extern "C"
            continue
        m = re.fullmatch(r"(.*?\bpdsc_\w+)\s*\((.*)\)", stmt, re.S)
        assert m, f"include/pdsc.h: not a prototype: {stmt!r}"
        ret = _declarator(m.group(1))
        params = [] if m.group(2).strip() == "void" else [_declarator(p) for p in m.group(2).split(",")]
        assert ret[2] not in functions, ret[2]
        functions[ret[2]] = (ret, params)
    return structs, functions


def _scalar_or_pointer(base, depth):
    if depth == 0:
        return SCALARS[base]
    return ctypes.c_char_p if (base, depth) == ("char", 1) else ctypes.c_void_p


def expected_parameter(fn, base, depth, name, arr):
    """The ctypes types _PROTOS may give this parameter (see the table above)."""
    if arr is not None:
        depth += 1  # an array parameter is a pointer
    if (fn, name) in HOST_POINTERS:
        want = HOST_POINTERS[(fn, name)]
        assert depth >= 1 and (base in ("void", "float") or want == P(SCALARS[base])), (fn, name, base)
        return (want,)
    if (base, depth) == ("pdsc_config", 1):
        return (_lib.CFG,)
    if depth == 1 and re.fullmatch(r"pdsc_\w+_debug", base):
        return (P(_struct_class(base)), ctypes.c_void_p)
    return (_scalar_or_pointer(base, depth),)


def test_prototypes_match_header():
    """_lib._PROTOS against include/pdsc.h: the return type and the ordered
    parameter types of every function (only the names were compared before: a
    swapped c_int32 / c_double loaded and ran).  Needs no library and no GPU."""
    _, functions = parse_header()
    assert sorted(functions) == header_functions() and set(functions) == set(_lib._PROTOS)
    assert not [k for k in HOST_POINTERS if k[0] not in functions
                or k[1] not in [p[2] for p in functions[k[0]][1]]], "HOST_POINTERS names a parameter the header lacks"
    bad = []
    for fn, ((rbase, rdepth, _, _), params) in functions.items():
        res, args = _lib._PROTOS[fn]
        if res != _scalar_or_pointer(rbase, rdepth):
            bad.append(f"{fn}: returns {res.__name__}, the header says {rbase}{'*' * rdepth}")
        if len(args) != len(params):
            bad.append(f"{fn}: {len(args)} arguments, the header has {len(params)}")
            continue
        for i, (got, (base, depth, name, arr)) in enumerate(zip(args, params)):
            if got not in expected_parameter(fn, base, depth, name, arr):
                bad.append(f"{fn}: argument {i} ({name}) is {got.__name__}, the header says {base}{'*' * depth}")
    assert not bad, "\n".join(bad)


def test_workspace_functions_end_in_ws_bytes_stream():
    """What _call.call relies on: a function that takes a workspace ends in (void
    *workspace, size_t workspace_bytes, pdsc_stream_t stream), and every
    *_workspace_bytes query has such a function."""
    _, functions = parse_header()
    users = {fn: p for fn, (_, p) in functions.items() if any(q[2] == "workspace" for q in p)}
    for fn, p in users.items():
        assert [(b, d) for b, d, _, _ in p[-3:]] == [("void", 1), ("size_t", 0), ("pdsc_stream_t", 0)], fn
        assert [n for _, _, n, _ in p[-3:-1]] == ["workspace", "workspace_bytes"], fn
    queries = [fn for fn in functions if fn.endswith("_workspace_bytes")]
    assert len(queries) >= 20 and len(users) >= len(queries)
    for q in queries:
        stem = q[:-len("_workspace_bytes")]
        assert any(fn.startswith(stem) for fn in users), q


def test_structs_match_header():
    """Every typedef struct of include/pdsc.h has a ctypes.Structure in _lib with
    the same field names, order, types and array lengths, and the size and
    offsets the C compiler gives the header's declaration (natural alignment)."""
    structs, _ = parse_header()
    assert len(structs) >= 12
    for c_name, fields in structs.items():
        cls = _struct_class(c_name)
        assert cls is not None and issubclass(cls, ctypes.Structure), f"no ctypes mirror of {c_name}"
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], c_name
        offset = align = 0
        for (name, got), (_, base, depth, arr) in zip(cls._fields_, fields):
            want = _scalar_or_pointer(base, depth)
            size = al = ctypes.sizeof(want)
            if arr is not None:
                want, size = want * arr, size * arr
            assert got == want, f"{c_name}.{name} is {got.__name__}, the header says {base}{'*' * depth}[{arr}]"
            offset = -(-offset // al) * al
            assert getattr(cls, name).offset == offset, f"{c_name}.{name}"
            offset, align = offset + size, max(align, al)
        assert ctypes.sizeof(cls) == -(-offset // align) * align, c_name
    sizes = {n: ctypes.sizeof(_struct_class(n)) for n in structs}
    assert (sizes["pdsc_clique_result"], sizes["pdsc_gnc_info"], sizes["pdsc_icp_result"]) == (24, 24, 152)
    assert sizes["pdsc_ransac_result"] == sizes["pdsc_gc_ransac_result"] == sizes["pdsc_teaser_result"] == 160


def test_version():
    assert b"gfx950" in _lib.load().pdsc_version()


@pytest.mark.parametrize("L", [1, 2, 12])
def test_param_order_matches_reference_state_dict(L):
    lib = _lib.load()
    cfg = _lib.make_config(num_layers=L)
    names = [lib.pdsc_param_name(ctypes.byref(cfg), i).decode() for i in range(lib.pdsc_param_count(ctypes.byref(cfg)))]
    ref = [k for k in state_dict_keys(L) if not k.endswith("num_batches_tracked")]
    assert names == ref


def test_refine_threshold_rule():
    # models/PointDSC.py:415-418
    assert abs(_lib.make_config(inlier_threshold=0.10).refine_threshold - 0.10) < 1e-7
    assert abs(_lib.make_config(inlier_threshold=0.6).refine_threshold - 1.2) < 1e-7


def test_workspace_queries():
    lib = _lib.load()
    cfg = _lib.make_config()
    for B, N in [(1, 1000), (4, 5000), (1, 30)]:
        assert lib.pdsc_forward_workspace_bytes(ctypes.byref(cfg), B, N) > 4 * B * N * N
        assert lib.pdsc_encoder_workspace_bytes(ctypes.byref(cfg), B, N) > 0
    assert lib.pdsc_forward_workspace_bytes(ctypes.byref(cfg), 1, 5) == 0  # int(5*0.1) = 0 seeds
    bad = _lib.make_config(num_channels=64)
    assert lib.pdsc_forward_workspace_bytes(ctypes.byref(bad), 1, 1000) == 0
    assert b"num_channels" in lib.pdsc_last_error()


def test_argument_errors_without_device():
    lib = _lib.load()
    assert lib.pdsc_compat_f32(None, None, 1, 10, None, None, None) == 1
    assert b"null" in lib.pdsc_last_error()
    cfg = _lib.make_config()
    rc = lib.pdsc_forward_testing(ctypes.byref(cfg), None, None, None, None, 1, 1000, None, None, None,
                                  None, None, 0, None)
    assert rc == 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_module_state_dict_keys_match_reference():
    import torch
    from pointdsc_amd.PointDSC import PointDSC
    m = PointDSC(num_layers=12)
    assert list(m.state_dict().keys()) == state_dict_keys(12)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in
          __import__("pointdsc_amd.synthetic", fromlist=["x"]).trained_state_dict("3dmatch", 12).items()}
    m.load_state_dict(sd, strict=True)


def test_module_refuses_cpu_and_training():
    import torch
    from pointdsc_amd.PointDSC import PointDSC
    m = PointDSC(num_layers=2)
    data = {"corr_pos": torch.zeros(1, 50, 6), "src_keypts": torch.zeros(1, 50, 3),
            "tgt_keypts": torch.zeros(1, 50, 3)}
    with pytest.raises(NotImplementedError):
        m(data)
    data["testing"] = True
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(data)


def test_query_functions_reject_bad_precision():
    lib = _lib.load()
    a, b = ctypes.c_int32(), ctypes.c_int32()
    assert lib.pdsc_attention_layout(4, 1000, 0, ctypes.byref(a), ctypes.byref(b)) == 0
    assert lib.pdsc_encoder_plan(4, 1000, 1, ctypes.byref(a)) == 0
    assert lib.pdsc_attention_layout(4, 1000, 7, ctypes.byref(a), ctypes.byref(b)) == 1
    assert b"precision" in lib.pdsc_last_error()
    assert lib.pdsc_encoder_plan(4, 1000, -1, ctypes.byref(a)) == 1


def test_ragged_counts_validated_on_host():
    """pdsc_forward_testing_ragged rejects counts that would change a pair's k
    (min(k, count - 1) must equal the batch's) or leave it without seeds, before
    touching any buffer (dummy non-null pointers: nothing is dereferenced)."""
    lib = _lib.load()
    cfg = _lib.make_config()
    dummy = ctypes.c_void_p(16)
    for counts in ([1000, 40], [1000, 1001], [1000, 0]):
        arr = (ctypes.c_int32 * 2)(*counts)
        rc = lib.pdsc_forward_testing_ragged(ctypes.byref(cfg), dummy, dummy, dummy, dummy, 2, 1000, arr, dummy,
                                             dummy, None, dummy, 1, None)
        assert rc == 1 and b"counts[1]" in lib.pdsc_last_error(), counts
    rc = lib.pdsc_forward_testing_ragged(ctypes.byref(cfg), dummy, dummy, dummy, dummy, 2, 1000, None, dummy,
                                         dummy, None, dummy, 1, None)
    assert rc == 1


def test_flat_weight_views_track_edits():
    """PointDSC re-homes the packed parameters/buffers as views of one flat
    buffer (PointDSC._flatten; on the device in a forward, on the CPU here):
    state_dict keys, values and requires_grad are unchanged, and every kind of
    in-place edit -- an optimizer-style update under no_grad, load_state_dict's
    copy_, a running statistic -- bumps the ONE version counter the per-forward
    change check reads; replacing a Parameter bumps the registration epoch."""
    import torch
    import torch.nn as nn
    from pointdsc_amd import PointDSC as mod
    m = mod.PointDSC(num_layers=3)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    grads = {k: p.requires_grad for k, p in m.named_parameters()}
    tensors = m._packable(m.pdsc_config())
    flat = m._flatten(tensors, device_only=False)
    assert flat is not None and flat.numel() == sum(t.numel() for t in tensors.values())
    after = m.state_dict()
    assert list(after) == list(before)
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert {k: p.requires_grad for k, p in m.named_parameters()} == grads
    views = m._packable(m.pdsc_config())
    assert all(t.data_ptr() >= flat.data_ptr() for t in views.values())
    v = flat._version
    with torch.no_grad():
        m.encoder.layer0.weight.mul_(2)
    assert flat._version != v
    v = flat._version
    m.encoder.blocks["PointCN_layer_1"][1].running_var.add_(1)
    assert flat._version != v
    v = flat._version
    m.load_state_dict(before)
    assert flat._version != v and torch.equal(m.state_dict()["encoder.layer0.weight"], before["encoder.layer0.weight"])
    e = mod._REGISTRATION_EPOCH[0]
    m.classification[4].bias = nn.Parameter(torch.zeros(1))
    assert mod._REGISTRATION_EPOCH[0] != e


def test_flatten_keeps_parameter_objects_and_inference_mode():
    """the flat buffer keeps every Parameter / buffer OBJECT (an
    optimizer built before the first forward still updates the model, and its
    steps bump the flat version), it is built outside inference mode (a first
    forward under torch.inference_mode() leaves ordinary tensors: later in-place
    edits and load_state_dict outside it work), and a registration in another
    module does not count as a change of this model's tensors."""
    import torch
    import torch.nn as nn
    from pointdsc_amd import PointDSC as mod
    m = mod.PointDSC(num_layers=2)
    ids = {k: id(v) for k, v in m.named_parameters()}
    bufs = {k: id(v) for k, v in m.named_buffers()}
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    w0 = m.encoder.layer0.weight
    w0.grad = torch.ones_like(w0)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    cfg = m.pdsc_config()
    with torch.inference_mode():
        flat = m._flatten(m._packable(cfg), device_only=False)
        _ = flat._version  # readable: not an inference tensor
    assert flat is not None and not flat.is_inference()
    assert {k: id(v) for k, v in m.named_parameters()} == ids
    assert {k: id(v) for k, v in m.named_buffers()} == bufs
    assert m.encoder.layer0.weight is w0 and torch.equal(w0.grad, torch.ones_like(w0))
    assert all(not v.is_inference() for v in m.state_dict().values())
    assert all(torch.equal(m.state_dict()[k], before[k]) for k in before)
    assert flat.data_ptr() <= w0.data_ptr() < flat.data_ptr() + flat.numel() * 4
    v = flat._version
    opt.step()  # the optimizer's own Parameter references
    assert flat._version != v
    assert torch.allclose(m.encoder.layer0.weight, before["encoder.layer0.weight"] - 0.5)
    v = flat._version
    m.load_state_dict(before)  # outside inference mode, after the flatten
    assert flat._version != v and torch.equal(m.encoder.layer0.weight, before["encoder.layer0.weight"])
    # identity check after an unrelated registration (what packed_weights does on an epoch bump)
    st = {"flat": flat, "tensors": m._packable(cfg)}
    nn.Linear(2, 2)
    assert m._same_tensors(st, cfg)
    m.encoder.layer0.bias = nn.Parameter(torch.zeros_like(m.encoder.layer0.bias))
    assert not m._same_tensors(st, cfg)
