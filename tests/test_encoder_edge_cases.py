"""The encoder's edge-shape cases on the reference alone -- no GPU needed
(DESIGN.md §7 "Encoder plans: edge-shape bars").

1. The bars of test_gpu_encoder_edges.py reject wrong kernels: the fp64 restatement
   with each of seven defects built in (plain torch, CPU) lands outside the case's
   bar on the logits AND on the features at every shape where the defect is not a
   no-op.  The defects, per attention layer of a pair of n correspondences:
     1-3  the softmax runs over keys padded to the next multiple of 32 / 128 / 256,
          with logit 0 and V = 0 on the pad (no-ops at n % 32 / 128 / 256 == 0);
     4    the partial last key tile is dropped (a no-op at n % 32 == 0; below 32
          keys none is left and the message is 0);
     5    dead rows are averaged over the count padded to 128 instead of n (none of
          the shapes is a multiple of 128).  The encoder's M has a unit diagonal, so
          no row of it is all zero: a dead row here is one with no compatible partner
          (M_ij = 0 for every j != i: every logit but its own is 0), and the defect
          is defect 2 on those rows alone;
     6    a ragged pair's zero-padded rows take part as keys (the ragged batch only;
          a no-op for the pair that fills the stride);
     7    1/sqrt(128) is dropped in the last layer only.
2. The case table's own preconditions: every pair has a non-zero off-diagonal M
   entry and a dead row, and the expected plan rows are self-consistent.
3. The knob table reaches every form of plan_encoder, and the library's host-only
   queries answer what tests/golden/encoder_edges/plans.json records.
"""
import numpy as np
import pytest
import torch

import encoder_edge_cases as C
from conftest import ENVELOPE, FEAT_FLOOR, LOGIT_FLOOR

CPU = torch.device("cpu")
DEFECTS = (1, 2, 3, 4, 5, 6, 7)
PAD = {1: 32, 2: 128, 3: 256}


def _round_up(n, m):
    return (n + m - 1) // m * m


def _attention(q, k, v, M, n, defect, last):
    """softmax_j(M_ij q_i.k_j / sqrt(128)) v_j over the pair's n keys, with `defect`."""
    scale = 1.0 if defect == 7 and last else 1.0 / 128 ** 0.5
    lg = M * (q @ k.T) * scale
    if defect in PAD:
        pad = _round_up(n, PAD[defect]) - n
        lg = torch.cat([lg, lg.new_zeros(len(lg), pad)], 1)
        v = torch.cat([v, v.new_zeros(pad, v.shape[1])], 0)
    if defect == 4:
        keep = n // 32 * 32
        if keep == 0:
            return torch.zeros_like(v)
        lg, v = lg[:, :keep], v[:keep]
    msg = torch.softmax(lg, -1) @ v
    if defect == 5:
        dead = _dead_rows(M)
        msg[dead] = _attention(q[dead], k, v, M[dead], n, 2, last)
    return msg


def _dead_rows(M):
    """Rows with no compatible partner: M_ij = 0 for every j != i."""
    return ((M != 0).sum(1) - (torch.diagonal(M) != 0).long()) == 0


def encoder_defect(g, sd, defect=None, stride=None):
    """conftest.encoder_torch's fp64 formula on the CPU with one defect built in.
    stride (defect 6): the pair zero-padded to `stride` rows, every row a key."""
    from oracle import pdsc_oracle as O
    n = len(g["corr_pos"])
    corr, src, tgt = g["corr_pos"], g["src_keypts"], g["tgt_keypts"]
    if defect == 6:
        corr, src, tgt = (np.concatenate([a, np.zeros((stride - n, a.shape[1]), a.dtype)]) for a in (corr, src, tgt))
    rows = len(corr)
    W = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items() if np.asarray(v).dtype != np.int64}
    conv = lambda x, nm: x @ W[nm + ".weight"][:, :, 0].T + W[nm + ".bias"]  # noqa: E731

    def bn(x, nm):
        a = W[nm + ".weight"] / torch.sqrt(W[nm + ".running_var"] + 1e-5)
        return x * a + (W[nm + ".bias"] - W[nm + ".running_mean"] * a)

    M = torch.from_numpy(O.compat(src, tgt, float(np.float32(g["sigma_d"])))).double()
    f = conv(torch.from_numpy(np.ascontiguousarray(corr)).double(), "encoder.layer0")
    L = int(g["num_layers"])
    for i in range(L):
        p = f"encoder.blocks.PointCN_layer_{i}"
        f = torch.relu(bn(conv(f, p + ".0"), p + ".1"))
        p = f"encoder.blocks.NonLocal_layer_{i}"
        q, k, v = (conv(f, f"{p}.projection_{c}") for c in "qkv")
        h = _attention(q, k, v, M, rows, defect, i == L - 1)
        h = torch.relu(bn(conv(h, p + ".fc_message.0"), p + ".fc_message.1"))
        h = torch.relu(bn(conv(h, p + ".fc_message.3"), p + ".fc_message.4"))
        f = f + conv(h, p + ".fc_message.6")
    h = torch.relu(conv(f, "classification.0"))
    h = torch.relu(conv(h, "classification.2"))
    return f[:n].numpy(), conv(h, "classification.4")[:n, 0].numpy()


def _noop(defect, n, ragged_stride):
    if defect in PAD:
        return n % PAD[defect] == 0
    if defect == 4:
        return n % 32 == 0
    if defect == 6:
        return ragged_stride is None or n == ragged_stride
    return False


_PAIRS = {}


def _pairs():
    if not _PAIRS:
        for key, i, g in C.all_pairs():
            _PAIRS.setdefault(key, []).append((i, g))
    return _PAIRS


KEYS = [C.shape_key(B, N) for B, N in C.SHAPES] + [C.RAGGED_KEY]


@pytest.mark.parametrize("key", KEYS)
def test_defects_land_outside_the_bar(key):
    sd = C.state_dict()
    stride = max(C.RAGGED) if key == C.RAGGED_KEY else None
    for i, g in _pairs()[key]:
        n = len(g["corr_pos"])
        r = C.reference(g, CPU, want_M=False)
        tol_f, tol_c = ENVELOPE * r["e_f"] + FEAT_FLOOR, ENVELOPE * r["e_c"] + LOGIT_FLOOR
        f0, c0 = encoder_defect(g, sd)  # the defect-free restatement is conftest's
        assert np.abs(f0 - r["f64"]).max() <= 1e-12 * r["mx"] and np.abs(c0 - r["c64"]).max() <= 1e-11
        for d in DEFECTS:
            if _noop(d, n, stride):
                continue
            f, c = encoder_defect(g, sd, d, stride)
            err_f, err_c = np.abs(f - r["f64"]).max() / r["mx"], np.abs(c - r["c64"]).max()
            # (a NaN compares false with any bound: it must count as outside)
            assert not err_f <= tol_f, (key, i, d, "features", err_f, tol_f)
            assert not err_c <= tol_c, (key, i, d, "logits", err_c, tol_c)


@pytest.mark.parametrize("key", KEYS)
def test_case_preconditions(key):
    """Every pair has a non-zero off-diagonal M entry (the attention is not uniform)
    and a dead row (no compatible partner: every logit but its own is 0, and the
    softmax is all but the mean over exactly n keys)."""
    from oracle import pdsc_oracle as O
    for i, g in _pairs()[key]:
        M = O.compat(g["src_keypts"], g["tgt_keypts"], 0.10)
        off = M - np.diag(np.diagonal(M))
        assert (off != 0).any(), (key, i)
        assert (off == 0).all(1).any(), (key, i)
        assert np.isfinite(g["corr_pos"]).all()


def test_attention_case_preconditions():
    """The standalone attention's M (kernels.compat on a synthetic pair) restated on
    the CPU: from N = 31 up it has non-zero off-diagonal entries and dead rows."""
    from oracle import pdsc_oracle as O
    for B, N in C.ATT_SHAPES:
        b = C.batch(B, max(N, 2))
        for i in range(B):
            M = O.compat(b["src_keypts"][i, :N], b["tgt_keypts"][i, :N], 0.10)
            if N >= 31:
                off = M - np.diag(np.diagonal(M))
                assert (off != 0).any() and (off == 0).all(1).any(), (B, N, i)


def test_plan_rows_self_consistent():
    rec = C.recorded_plans()
    assert sorted(rec) == sorted(C.KNOB_SETS)
    keys = [k for k, _, _ in C.plan_shapes()]
    for sid, rows in rec.items():
        assert list(rows) == keys, sid
        for key, B, N in C.plan_shapes():
            q = dict(zip(C.QUERY_FIELDS, rows[key]))
            assert q["Npad"] == _round_up(N, 128) and 1 <= q["nsplit"] <= max(1, _round_up(N, 32) // 64), (sid, key)
            assert q["kind"] in (0, 1, 2) and (q["pw2"] == 1) == (q["pw_tile"] == 0), (sid, key)
            if q["pw2"]:
                assert not any(q[f] for f in ("pw_mid8", "pw_first_qkv3", "pw_mid_qkv3", "pw_prefetch")), (sid, key)
            if q["kind"] == 1:
                assert q["pw2"] == 1, (sid, key)
            assert q["pw_mid_qkv3"] <= q["pw_mid8"] and q["pw_prefetch"] <= q["pw_mid8"], (sid, key)


@pytest.mark.parametrize("sid", list(C.KNOB_SETS))
def test_set_plans(sid):
    """Under the set's knobs (a fresh process) the library's host-only queries answer
    the recording, and plan_form -- plan_encoder's rules restated, which names what the
    queries cannot show -- agrees with them in every field they do show: a knob that is
    misspelt or no longer read, or a changed plan rule, fails here and cannot turn a
    set silently into a second copy of `default`."""
    precision, knobs = C.KNOB_SETS[sid]
    got, want = C.plan_queries_of(sid), C.recorded_plans()[sid]
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    for key, B, N in C.plan_shapes():
        form = C.plan_form(B, N, precision, knobs, ragged=key == C.RAGGED_KEY)
        assert C.form_as_queries(form) == want[key], (sid, key, form)


def _forms(entry):
    """(set, shape) -> plan_form of one entry point: the forwards', the standalone
    encoder's (dense_m_caller) or the standalone attention's (no fused plan)."""
    kw = {"forward": {}, "encoder": dict(dense_m_caller=True), "attention": dict(dense_m_caller=True, allow_fused=False)}
    out = {}
    for sid, (precision, knobs) in C.KNOB_SETS.items():
        if entry == "attention":
            if sid not in C.ATT_SETS:
                continue
            shapes = [(C.shape_key(B, N), B, N) for B, N in C.ATT_SHAPES]
            for pr in ("h3", "f32") if sid == "default" else ("h3",):
                out.update({(sid + ":" + pr, key): C.plan_form(B, N, pr, knobs, **kw[entry]) for key, B, N in shapes})
            continue
        for key, B, N in C.plan_shapes():
            if key == C.RAGGED_KEY and entry != "forward":
                continue
            out[(sid, key)] = C.plan_form(B, N, precision, knobs, ragged=key == C.RAGGED_KEY, **kw[entry])
    return out


def test_table_reaches_every_form():
    """The table as a whole reaches every attention kernel and pointwise chain of
    plan_encoder.  kind 1 / 2 / 0, vfold, the split count and the chain's form are the
    library's own answers (test_set_plans); which of the kind-0 kernels runs (ATT_F32
    by the precision; ATT_H3 by its waves and early loop; ATT_H3_WS), the precombine,
    stream-K against the split grid and M's layout are plan_form's restatement, which
    the queries support only through the split counts they share."""
    fwd, enc, att = _forms("forward"), _forms("encoder"), _forms("attention")
    kinds = lambda fs: {f["kind"] for f in fs.values()}  # noqa: E731
    assert kinds(fwd) == {"ATT_FUSED", "ATT_F32", "ATT_H3", "ATT_H3_WS", "ATT_W64", "ATT_W64_SK"}
    assert kinds(enc) == {"ATT_FUSED", "ATT_F32", "ATT_H3", "ATT_H3_WS"}  # dense M: never attention_w64
    assert kinds(att) == {"ATT_F32", "ATT_H3", "ATT_H3_WS"}
    for fs in (fwd, enc, att):
        h3 = {(f["nw"], f["early"]) for f in fs.values() if f["kind"] == "ATT_H3"}
        assert h3 == {(nw, e) for nw in (1, 2, 4) for e in (False, True)}
    for fs in (fwd, enc):
        assert {f["precombine"] for f in fs.values()} == {False, True}
        assert {f["vfold"] for f in fs.values()} == {False, True}
        assert {f["pw2"] for f in fs.values()} == {False, True}
        assert {f["pw_tile"] for f in fs.values()} == {0, 32, 64}
        assert {f["pw_mid8"] for f in fs.values() if not f["pw2"]} == {False, True}
        assert {f["pw_first_qkv3"] for f in fs.values() if not f["pw2"]} == {False, True}
        assert {f["pw_prefetch"] for f in fs.values() if not f["pw2"]} == {False, True}
    # the fused kernels on packed and on dense M; attention_w64 folded (zero-padded V') and not
    assert {f["dense_m"] for f in fwd.values() if f["kind"] == "ATT_FUSED"} == {False, True}
    assert {f["vfold"] for f in fwd.values() if f["kind"] == "ATT_W64"} == {False, True}
    # the sets reach what they are named after
    assert all(f["kind"] == "ATT_FUSED" for (s, _), f in fwd.items() if s.startswith("fused"))
    assert all(f["kind"] in ("ATT_W64", "ATT_W64_SK") for (s, _), f in fwd.items() if s.startswith("w64"))
    assert {k for (s, k), f in fwd.items() if f["kind"] == "ATT_W64_SK"} == {"1x513", "3x257", "3x513"}
    assert {k for (s, k), f in fwd.items() if s == "default" and f["kind"] == "ATT_H3_WS"} == {"3x513", "1x993"}
    assert all(f["nw"] == int(s[2]) for (s, _), f in fwd.items() if s in ("nw1", "nw2", "nw4"))
    assert {k for (s, k), f in fwd.items() if f["precombine"]} == {"1x993"}
    # a last key tile of one key, and N below one tile, under every set
    assert {"1x10", "3x31", "1x33", "3x65", "1x129", "3x257", "3x513", "1x993"} <= {k for _, k in fwd}
