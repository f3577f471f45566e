"""The pointwise chain's and the tail's launch plan, as the host-only query
pdsc_launch_plan reports it, against a Python restatement of the rules -- no
GPU needed.

The restatement (expected_row) is written from the launchers' rules as they
stood when each launcher still decided for itself: a change of which kernel
runs at a shape shows here as a differing row.  The grid is test_plan_table's
B x N x precision (plus 40 pairs: 40 x 1000 is the 320-workgroup bound itself),
under the default knobs and under each knob setting of VARIANTS (one fresh
process per setting: the library reads its knobs once).  It straddles every
threshold of the rules; test_grid_reaches_every_form asserts that each
decision takes each of its values somewhere on it.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

BS = (1, 2, 3, 4, 5, 8, 16, 17, 32, 40, 64, 65, 128)
NS = (2, 100, 500, 512, 513, 700, 777, 1000, 1024, 1025, 1500, 1536, 1537, 2000, 2048, 2049, 3000, 5000, 9000,
      12000, 32767)
PRECISIONS = (0, 1)  # enum pdsc_precision: H3, F32
VARIANTS = ("", "PDSC_PW2=0", "PDSC_PW2=2", "PDSC_PW_WAVES=4", "PDSC_PW_QKV_SPLIT=0", "PDSC_PW_SMALL_LIMIT=0",
            "PDSC_SEED_BLOCKS=0", "PDSC_LM_RPT=4", "PDSC_SEED_SELECT=0", "PDSC_SEED_SELECT=1", "PDSC_SEED_SORT=1",
            "PDSC_SEED_WPB=2", "PDSC_KABSCH_FUSED=0", "PDSC_TAIL_FUSED=0")
# pdsc_launch_plan's row (include/pdsc.h)
COLUMNS = ("pw2", "pw_tile", "pw_mid8", "pw_first_qkv3", "pw_mid_qkv3", "pw_prefetch", "seed_rows", "nms_rpt",
           "seed_rank", "seed_wpb", "knn_bitonic", "kabsch_fused", "tail_fused")
RANK_COMPARE, RANK_SORT, RANK_SELECT, RANK_SELECT_SPLIT = range(4)
RATIO = 0.1  # make_config's default (a double, as here)
NO_PLAN = -1  # a row of these: the call has no seeds (int(N * ratio) = 0), pdsc_launch_plan returns an error


def expected_row(B, N, f32, knob):
    """The row for B pairs of N correspondences under the knob setting {name: int}."""
    S = int(N * RATIO)
    if S < 1:
        return [NO_PLAN] * len(COLUMNS)
    # the pointwise chain: register-chained from 320 workgroups of 128 points on, never in exact fp32
    Npad = (N + 127) // 128 * 128
    pw2_mode = knob.get("PDSC_PW2", 1)
    pw2 = not f32 and pw2_mode != 0 and (pw2_mode == 2 or B * (Npad // 128) >= 320)
    if pw2:
        chain = [1, 0, 0, 0, 0, 0]
    else:
        # 32-point tiles below 512 64-point tiles; 8 waves up to 256 32-point tiles; Q / K / V in three
        # workgroups per tile while 3 x the 32-point tiles stay within 256 (pw_first: on its 32-point tiles)
        small = B * (Npad // 64) < knob.get("PDSC_PW_SMALL_LIMIT", 512)
        mid8 = not f32 and knob.get("PDSC_PW_WAVES", 8) != 4 and B * (Npad // 32) <= 256
        qkv3 = knob.get("PDSC_PW_QKV_SPLIT", 1) != 0 and 3 * B * (Npad // 32) <= 256
        chain = [0, 32 if small else 64, mid8, not f32 and small and qkv3, mid8 and qkv3, mid8]
    # the tail
    sort = knob.get("PDSC_SEED_SORT", 0) == 1
    rows16 = B * ((N + 63) // 64) < knob.get("PDSC_SEED_BLOCKS", 1024)
    rpt = knob.get("PDSC_LM_RPT", 0) or (2 if B > 1 and rows16 else 1)
    nms = 0 if sort and N <= 5120 else rpt
    sel_mode = knob.get("PDSC_SEED_SELECT", 2)
    sel_lds = ((N + 1) & ~1) * 4 + 2048 * 12  # keys + candidates: the 64 KiB LDS cap
    select = sel_mode != 0 and sel_lds <= 64 * 1024 and (sel_mode == 1 or float(B) * N * N >= 1e8)
    if select and not sort:
        rank = RANK_SELECT_SPLIT if S > 256 and N >= 3 else RANK_SELECT
    else:
        rank = RANK_SORT if sort and N <= 8192 else RANK_COMPARE
    wpb = knob.get("PDSC_SEED_WPB", 0) or (1 if B * ((S + 3) // 4) < 512 else 4)
    kabsch = knob.get("PDSC_KABSCH_FUSED", 1) != 0 and B * S <= 1024
    tail = knob.get("PDSC_TAIL_FUSED", 1) != 0
    return [int(v) for v in chain + [16 if rows16 else 64, nms, rank, wpb, 1, kabsch, tail]]


def expected(variant):
    knob = dict([(variant.split("=")[0], int(variant.split("=")[1]))] if variant else [])
    return np.array([[[expected_row(B, N, bool(p), knob) for p in PRECISIONS] for N in NS] for B in BS], np.int64)


def record():
    """[len(BS)][len(NS)][len(PRECISIONS)][len(COLUMNS)] int64 from the loaded library (this process's knobs)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from pointdsc_amd import _lib
    lib = _lib.load()
    out = np.zeros((len(BS), len(NS), len(PRECISIONS), len(COLUMNS)), np.int64)
    row = (ctypes.c_int32 * len(COLUMNS))()
    for p, prec in enumerate(PRECISIONS):
        cfg = _lib.make_config(precision="f32" if prec else "h3")
        assert cfg.ratio == RATIO
        for i, B in enumerate(BS):
            for j, N in enumerate(NS):
                assert lib.pdsc_launch_plan(ctypes.byref(cfg), B, N, row, len(COLUMNS) - 1) != 0  # too short a row
                rc = lib.pdsc_launch_plan(ctypes.byref(cfg), B, N, row, len(COLUMNS))
                out[i, j, p] = list(row) if rc == 0 else NO_PLAN
    return out


def record_variant(variant, path):
    """record() in a fresh process with the variant's knob set, through a file."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDSC_") or k == "PDSC_LIB_VARIANT"}
    if variant:
        k, v = variant.split("=")
        env[k] = v
    subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env=env, check=True, timeout=120)
    return np.load(path)


def test_launch_plan_matches_the_rules(tmp_path):
    for v, variant in enumerate(VARIANTS):
        got, want = record_variant(variant, str(tmp_path / f"v{v}.npy")), expected(variant)
        bad = np.argwhere((got != want).any(-1))
        rows = [(BS[i], NS[j], PRECISIONS[p], got[i, j, p].tolist(), want[i, j, p].tolist()) for i, j, p in bad[:5]]
        assert not len(bad), f"{variant or 'default knobs'}: {len(bad)} rows differ; (B, N, precision, got, want): {rows}"


def test_grid_reaches_every_form():
    """Each decision takes each of its values on the grid: under the default knobs
    every value a rule picks by shape, over all the settings the knob-only ones too."""
    def values(tables):
        rows = np.concatenate([t.reshape(-1, len(COLUMNS)) for t in tables])
        rows = rows[rows[:, 0] != NO_PLAN]
        return {c: set(rows[:, i].tolist()) for i, c in enumerate(COLUMNS)}
    default = values([expected("")])
    assert default == {"pw2": {0, 1}, "pw_tile": {0, 32, 64}, "pw_mid8": {0, 1}, "pw_first_qkv3": {0, 1},
                       "pw_mid_qkv3": {0, 1}, "pw_prefetch": {0, 1}, "seed_rows": {16, 64}, "nms_rpt": {1, 2},
                       "seed_rank": {RANK_COMPARE, RANK_SELECT, RANK_SELECT_SPLIT}, "seed_wpb": {1, 4},
                       "knn_bitonic": {1}, "kabsch_fused": {0, 1}, "tail_fused": {1}}
    every = values([expected(v) for v in VARIANTS])
    assert every["nms_rpt"] == {0, 1, 2, 4} and every["seed_wpb"] == {1, 2, 4} and every["tail_fused"] == {0, 1}
    assert every["seed_rank"] == {RANK_COMPARE, RANK_SORT, RANK_SELECT, RANK_SELECT_SPLIT}
    # the two Q / K / V split rules differ: pw_first's holds in exact fp32 never, pw_mid's on 8 waves only
    t = expected("PDSC_PW_WAVES=4").reshape(-1, len(COLUMNS))
    assert ((t[:, 3] == 1) & (t[:, 4] == 0)).any()
    # the LDS cap of the select form: a shape with B N^2 >= 1e8 that stays on the compare kernel
    assert expected_row(128, 12000, False, {})[8] == RANK_COMPARE and expected_row(128, 9000, False, {})[8] == RANK_SELECT_SPLIT


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        np.save(sys.argv[2], record())
    else:
        sys.exit("usage: test_launch_plan.py --record PATH")
