"""The encoder's attention plan, as the host-only queries of the C ABI report it,
replayed against a recorded table (tests/golden/plan/plan_table.npz) -- no GPU needed.

The table is the product of B, N and both precisions below, under the default
knobs and under each knob variant of VARIANTS (one fresh process per variant:
the library reads its knobs once).  B and N straddle every threshold of the
planner's rules: the 16-block limits, the 24-tile tiny limit, the nsplit >= 16
precombine rule, the 128-block w64 rule and the 320-tile pw2 rule.  A change of
which attention kernel runs at a shape, of a split count or of a workspace
size (ABI-visible) shows here as a differing row.

`python tests/test_plan_table.py --write` records the table from the built
library; only a commit whose plans are MEANT to change should do that.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "plan", "plan_table.npz")

BS = (1, 2, 3, 4, 5, 8, 16, 17, 32, 64, 65, 128)
NS = (2, 100, 500, 512, 513, 700, 777, 1000, 1024, 1025, 1500, 1536, 1537, 2000, 2048, 2049, 3000, 5000, 9000,
      12000, 32767)
PRECISIONS = (0, 1)  # enum pdsc_precision: H3, F32
VARIANTS = ("", "PDSC_FUSE=0", "PDSC_W64_SK=0", "PDSC_W64=0", "PDSC_W64=1", "PDSC_ATT_TINY=0", "PDSC_PRECOMBINE=0",
            "PDSC_DENSE_M=1")
COLUMNS = ("encoder_plan", "layout_Npad", "layout_nsplit", "forward_workspace_bytes",
           "forward_training_workspace_bytes", "encoder_workspace_bytes", "attention_workspace_bytes")


def record():
    """[len(BS)][len(NS)][len(PRECISIONS)][len(COLUMNS)] int64 from the loaded library (this process's knobs)."""
    sys.path.insert(0, os.path.dirname(HERE))
    from pointdsc_amd import _lib
    lib = _lib.load()
    out = np.zeros((len(BS), len(NS), len(PRECISIONS), len(COLUMNS)), np.int64)
    plan, npad, nsplit = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    for p, prec in enumerate(PRECISIONS):
        cfg = _lib.make_config(precision="f32" if prec else "h3")
        for i, B in enumerate(BS):
            for j, N in enumerate(NS):
                assert lib.pdsc_encoder_plan(B, N, prec, ctypes.byref(plan)) == 0
                assert lib.pdsc_attention_layout(B, N, prec, ctypes.byref(npad), ctypes.byref(nsplit)) == 0
                out[i, j, p] = (plan.value, npad.value, nsplit.value,
                                lib.pdsc_forward_workspace_bytes(ctypes.byref(cfg), B, N),
                                lib.pdsc_forward_training_workspace_bytes(ctypes.byref(cfg), B, N),
                                lib.pdsc_encoder_workspace_bytes(ctypes.byref(cfg), B, N),
                                lib.pdsc_attention_workspace_bytes(B, N, 128, prec))
    return out


def record_variant(variant, path):
    """record() in a fresh process with the variant's knob set, through a file."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDSC_") or k == "PDSC_LIB_VARIANT"}
    if variant:
        k, v = variant.split("=")
        env[k] = v
    subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env=env, check=True, timeout=120)
    return np.load(path)


def test_plan_table_matches_recording(tmp_path):
    with np.load(FIXTURE, allow_pickle=False) as z:
        assert tuple(z["B"]) == BS and tuple(z["N"]) == NS and tuple(z["precision"]) == PRECISIONS
        assert tuple(str(v) for v in z["variants"]) == VARIANTS and tuple(str(c) for c in z["columns"]) == COLUMNS
        want = z["table"]
    assert want.shape == (len(VARIANTS), len(BS), len(NS), len(PRECISIONS), len(COLUMNS))
    # the table does reach every plan kind pdsc_encoder_plan reports
    assert set(np.unique(want[0, ..., 0])) == {0, 1, 2}
    for v, variant in enumerate(VARIANTS):
        got = record_variant(variant, str(tmp_path / f"v{v}.npy"))
        bad = np.argwhere((got != want[v]).any(-1))
        rows = [(BS[i], NS[j], PRECISIONS[p], got[i, j, p].tolist(), want[v, i, j, p].tolist()) for i, j, p in bad[:5]]
        assert not len(bad), f"{variant or 'default knobs'}: {len(bad)} rows differ; (B, N, precision, got, want): {rows}"


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        np.save(sys.argv[2], record())
    elif sys.argv[1:2] == ["--write"]:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            table = np.stack([record_variant(v, os.path.join(d, "t.npy")) for v in VARIANTS])
        np.savez_compressed(FIXTURE, B=np.array(BS), N=np.array(NS), precision=np.array(PRECISIONS),
                            variants=np.array(VARIANTS), columns=np.array(COLUMNS), table=table)
        print("wrote", FIXTURE, table.shape)
    else:
        sys.exit("usage: test_plan_table.py --write | --record PATH")
