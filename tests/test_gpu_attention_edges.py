"""The standalone attention (kernels.attention: pdsc_attention_f32, the split launch
on the caller's dense M, which follows the encoder's knobs) held to fp64 at edge
shapes (DESIGN.md §7 "Encoder plans: edge-shape bars"; run with -m gpu).

In the test process under the default knobs in both precisions, and inside the
nw1 / nw2 / nw4 children of encoder_edge_cases.py (ATT_H3 at 1, 2 and 4 waves, with
the early-issue loop where a split has 3 key tiles): B in {1, 3} x N in ATT_NS plus
1 x 993; q, k, v ~ N(0, 1), M from kernels.compat on a synthetic pair; inputs are the
leading part of a larger allocation whose remainder holds NaN.  The reference is
test_gpu_parity._attention_fp64 and the bar that file's, max|out - ref| <= 1e-6 max|v|.
  dead rows and columns of M (0, N // 2, N - 1 at N = 33, 129, 257) and M == 0
  (N = 31, 257): those rows' msg is the mean of v over the N keys, same bar;
  one case of test_attention_adversarial_magnitudes at 2 x 257 (sq, sk = 7, 1; v rows
  scaled by 1e-3 inside a tile; a last key tile of one row), that test's tolerance;
  in f32 precision msg is bitwise kernels.attention_lse's at every N (pdsc.h).
"""
import numpy as np
import pytest
import torch

import encoder_edge_cases as C
from test_gpu_parity import _attention_fp64

pytestmark = pytest.mark.gpu

RUNS = [("default", "h3"), ("default", "f32"), ("nw1", "h3"), ("nw2", "h3"), ("nw4", "h3")]
SHAPE_KEYS = [f"att:{C.shape_key(B, N)}" for B, N in C.ATT_SHAPES]
DEAD_KEYS = [f"dead:{N}" for N in C.DEAD_NS]
ZERO_KEYS = [f"zero:{N}" for N in C.ZERO_NS]
_REF = {}


def _refs(dev):
    """key -> (fp64 msg, v, M, max|logit|), once per session: the cases' inputs are
    regenerated here from their seeds (they do not depend on the knobs)."""
    if not _REF:
        for key, q, k, v, M in C.attention_cases(dev):
            lg = M.double() * (q.double() @ k.double().transpose(1, 2)) / 128 ** 0.5
            _REF[key] = (_attention_fp64(q, k, v, M).cpu().numpy(), v.double().cpu().numpy(), M.cpu().numpy(),
                         lg.abs().max().item(), (lg.max(-1).values - lg.min(-1).values).max().item())
    return _REF


def _out(sid, pr, key, dev):
    try:
        z = C.child_result(sid, dev)
    except C.KnobSetFailed as e:
        pytest.fail(str(e), pytrace=False)
    out = z[f"{key}:{pr}"]
    assert np.isfinite(out).all(), (sid, pr, key, "non-finite msg")
    assert z[f"{key}:{pr}:det"], (sid, pr, key, "two calls differ")
    return out.astype(np.float64), z


@pytest.mark.parametrize("key", SHAPE_KEYS)
@pytest.mark.parametrize("sid,pr", RUNS)
def test_attention_edges(sid, pr, key, gpu_device):
    ref, v, _, _, _ = _refs(gpu_device)[key]
    out, z = _out(sid, pr, key, gpu_device)
    err, bar = np.abs(out - ref).max(), 1e-6 * np.abs(v).max()
    print(f"attention {sid} {pr} {key}: err / bar {err / bar:.3f} (err {err:.3g})")
    assert err <= bar, (sid, pr, key, err, bar)
    if pr == "f32":
        assert z[f"{key}:lse_eq"], (key, "msg is not bitwise kernels.attention_lse's")


@pytest.mark.parametrize("key", DEAD_KEYS + ZERO_KEYS)
@pytest.mark.parametrize("sid,pr", RUNS)
def test_dead_rows_average_the_keys(sid, pr, key, gpu_device):
    ref, v, M, _, _ = _refs(gpu_device)[key]
    out, _ = _out(sid, pr, key, gpu_device)
    bar = 1e-6 * np.abs(v).max()
    dead = (M == 0).all(2)
    N = M.shape[1]
    assert dead[:, [0, N // 2, N - 1]].all() and (key.startswith("dead") or dead.all())
    err, err_mean = np.abs(out - ref).max(), np.abs(out - v.mean(1, keepdims=True))[dead].max()
    print(f"attention {sid} {pr} {key}: err / bar {err / bar:.3f}, dead rows against mean(v) {err_mean / bar:.3f}")
    assert err <= bar and err_mean <= bar, (sid, pr, key, err, err_mean, bar)


@pytest.mark.parametrize("sid,pr", RUNS)
def test_adversarial_magnitudes_one_row_tile(sid, pr, gpu_device):
    ref, v, _, lgmax, spread = _refs(gpu_device)["adv"]
    assert spread > 30 * np.log(2)
    out, _ = _out(sid, pr, "adv", gpu_device)
    tol = 2e-6 + 4 * 2.0 ** -24 * max(1.0, lgmax)  # test_attention_adversarial_magnitudes' formula
    err, bar = np.abs(out - ref).max(), tol * np.abs(v).max()
    print(f"attention {sid} {pr} adv: err / bar {err / bar:.3f} (err {err:.3g})")
    assert err <= bar, (sid, pr, err, bar)
