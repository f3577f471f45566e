"""Every encoder attention plan held to fp64 at edge shapes (DESIGN.md §7 "Encoder
plans: edge-shape bars"; run with -m gpu).

For every knob set and shape of encoder_edge_cases.py and for pairs 0 and B - 1 of
the batch, against conftest.encoder_torch in fp64 on the same pair:
  standalone encoder (kernels.encoder on the dense M of kernels.compat)
      max|feat - f64| / max|f64| <= ENVELOPE e_f + FEAT_FLOOR, max|conf - c64| <=
      ENVELOPE e_c + LOGIT_FLOOR, normed within 2 rel_row + 1e-6 of the fp64 unit
      rows (test_gpu_parity.test_encoder_and_classifier's rule; e_f, e_c:
      conftest.fp32_envelope, one plain-order fp32 run as the reference's output);
  forwards (packed M; the only entries that run attention_w64)
      kernels.forward_training's conf to the same logit bar, its M to ENVELOPE e_m +
      M_FLOOR (test_gpu_training's rule); kernels.forward_stages' conf bitwise the
      training forward's (both run run_encoder_fwd on the same plan, api.hip);
  ragged batch (counts 257, 33, 129, 10; k = 9, see encoder_edge_cases.RAGGED_K)
      kernels.forward_ragged's conf[b, :n_b] to the bar of pair b alone, labels past
      n_b exactly 0;
  every input is the leading part of a larger allocation whose remainder holds NaN,
  and the ragged batch's rows past a pair's count hold NaN in corr_pos, src and tgt
  (include/pdsc.h: "rows past counts[b] are ignored"); every output is finite;
  two calls give the same bits.
The yardstick is computed once per pair and shared by all knob sets.  One child
process per knob set, one at a time (encoder_edge_cases.child_result); after a child
that ended by a signal, its time limit or a HIP fault, no further GPU process starts.
"""
import numpy as np
import pytest

import encoder_edge_cases as C
from conftest import ENVELOPE, FEAT_FLOOR, LOGIT_FLOOR

pytestmark = pytest.mark.gpu

M_FLOOR = 2e-6  # test_gpu_training.M_FLOOR
_CASES = {}


def _cases():
    if not _CASES:
        for key, i, g in C.all_pairs():
            _CASES.setdefault(key, []).append((i, g))
    return _CASES


def _result(sid, dev):
    try:
        return C.child_result(sid, dev)
    except C.KnobSetFailed as e:
        pytest.fail(str(e), pytrace=False)


def _ratio(err, noise):
    return err / max(noise, 1e-300)


@pytest.mark.parametrize("sid", list(C.KNOB_SETS))
def test_set_ran_its_plans(sid, gpu_device):
    """The process that computed the set's outputs planned what the recording says
    (tests/golden/encoder_edges/plans.json): its knobs were in force."""
    import json
    assert json.loads(str(_result(sid, gpu_device)["plans"])) == C.recorded_plans()[sid]


@pytest.mark.parametrize("key", [C.shape_key(B, N) for B, N in C.SHAPES])
@pytest.mark.parametrize("sid", list(C.KNOB_SETS))
def test_encoder_edges(sid, key, gpu_device):
    z = _result(sid, gpu_device)
    assert z[key + ":fin"].all(), (sid, key, "a non-finite output (encoder, training forward, stage forward)")
    assert z[key + ":det"].all(), (sid, key, "two calls differ (encoder, training forward, stage forward)")
    assert z[key + ":stg_eq_trn"], (sid, key, "forward_stages' conf is not the training forward's")
    for slot, (i, g) in enumerate(_cases()[key]):
        r = C.reference(g, gpu_device)
        tol_f, tol_c, tol_m = ENVELOPE * r["e_f"] + FEAT_FLOOR, ENVELOPE * r["e_c"] + LOGIT_FLOOR, \
            ENVELOPE * r["e_m"] + M_FLOOR
        f = z[key + ":feat"][slot].astype(np.float64)
        err_f = np.abs(f - r["f64"]).max() / r["mx"]
        err_c = np.abs(z[key + ":conf"][slot] - r["c64"]).max()
        err_t = np.abs(z[key + ":trn_conf"][slot] - r["c64"]).max()
        err_m = np.abs(z[key + ":trn_M"][slot] - r["M64"]).max()
        print(f"edges {sid} {key} pair {i}: err/noise features {_ratio(err_f, r['e_f']):.2f} "
              f"logits {_ratio(err_c, r['e_c']):.2f} forward logits {_ratio(err_t, r['e_c']):.2f} "
              f"M {_ratio(err_m, r['e_m']):.2f}  (err {err_f:.3g} {err_c:.3g} {err_t:.3g} {err_m:.3g}; "
              f"noise {r['e_f']:.3g} {r['e_c']:.3g} {r['e_m']:.3g})")
        assert err_f <= tol_f, (sid, key, i, "features", err_f, r["e_f"])
        assert err_c <= tol_c, (sid, key, i, "logits", err_c, r["e_c"])
        assert err_t <= tol_c, (sid, key, i, "training forward's logits", err_t, r["e_c"])
        assert err_m <= tol_m, (sid, key, i, "training forward's M", err_m, r["e_m"])
        norm = np.maximum(np.linalg.norm(r["f64"], axis=1), 1e-12)
        rel_row = (np.abs(f - r["f64"]).max(1) / norm).max()
        assert np.abs(z[key + ":normed"][slot] - r["f64"] / norm[:, None]).max() <= 2 * rel_row + 1e-6, (sid, key, i)


@pytest.mark.parametrize("sid", list(C.KNOB_SETS))
def test_ragged_edges(sid, gpu_device):
    z = _result(sid, gpu_device)
    key = C.RAGGED_KEY
    assert z[key + ":fin"], (sid, "a non-finite pose, label or logit of a pair's own rows")
    assert z[key + ":det"], (sid, "two calls differ")
    for i, g in _cases()[key]:
        n = C.RAGGED[i]
        r = C.reference(g, gpu_device)
        err_c = np.abs(z[key + ":conf"][i, :n] - r["c64"]).max()
        print(f"edges {sid} ragged pair {i} (n = {n}): err/noise logits {_ratio(err_c, r['e_c']):.2f} "
              f"(err {err_c:.3g}; noise {r['e_c']:.3g})")
        assert err_c <= ENVELOPE * r["e_c"] + LOGIT_FLOOR, (sid, i, err_c, r["e_c"])
        assert (z[key + ":labels"][i, n:] == 0).all(), (sid, i)
