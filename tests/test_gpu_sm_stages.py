"""The spectral-matching baseline (pointdsc_amd/csrc/sm.hip: pdsc_sm_compat,
pdsc_sm_matvec, pdsc_spectral_matching) stage by stage against the restatement of
tests/sm_reference.py, at the sizes where a kernel takes another path: the scalar
store and load branches (N % 4 != 0), tile edges, the 256-element step of the vector
matvec, the 1024 stride of normalize and select, S = 0 and 1, exact ties at the
selection boundary across 1024-chunks, zero iterations, all-zero M (run with -m gpu).
Inputs and their preconditions: tests/test_sm_reference.py, which also shows on the
CPU that these assertions reject the kernels with one branch or rule taken out.

Bars: M bitwise; each matvec row within (N + 2) 2^-24 sum |M_ij v_j| of fp64; the
iterate within ENVELOPE x (fp32 noise of the case) + FEAT_FLOOR x max|v64| of fp64;
labels equal to `select` on the GPU's own vector; trans bitwise equal to
rigid_transform_3d on the GPU's own weights, and within 1e-4 of the oracle's where the
labels are the restatement's too.

Measured on an MI355X ("SM baseline"): 0 differing elements of M on every
case; worst matvec row 0.19 of its bound; the iterate's err / noise 0.30 .. 1.20 (worst at
N = 252, ten iterates); pose within 8.4e-7 (3dmatch) and 6.7e-6 (kitti) of the oracle's."""
import numpy as np
import pytest
import torch

import nsm_reference as K
import sm_reference as R
from conftest import ENVELOPE, FEAT_FLOOR

pytestmark = pytest.mark.gpu
f32 = np.float32


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, f32)).to(dev)


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _guarded(n, dev, pad=R.MATVEC_PAD):
    """A NaN-filled buffer of n + pad elements: (the first n as a view, the whole)."""
    buf = torch.full((n + pad,), float("nan"), dtype=torch.float32, device=dev)
    return buf[:n], buf


def _gpu_compat(d, dev):
    """pdsc_sm_compat into a buffer with one guard row: (M [N,N] numpy, guard row numpy)."""
    from pointdsc_amd.baselines import sm_compat
    N = d["N"]
    buf = torch.full((N + 1, N), float("nan"), dtype=torch.float32, device=dev)
    out = sm_compat(_t(d["corr"], dev), d["thr"], out=buf[:N])
    assert out.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    return host[:N], host[N]


def _sm(d, dev, **kw):
    from pointdsc_amd.baselines import SM
    T, lab, v = SM(_t(d["corr"][None], dev), _t(d["src"][None], dev), _t(d["tgt"][None], dev),
                   inlier_threshold=d["thr"], return_eig=True, **kw)
    return T[0].cpu().numpy(), lab[0].cpu().numpy(), v[0].cpu().numpy()


def _check_selection(d, T, lab, v, S, dev):
    """labels == select(the GPU's own v, S) with no allowance; trans bitwise the Kabsch
    launch on the GPU's own weights, and finite."""
    from pointdsc_amd import kernels
    assert np.array_equal(lab, R.select(v, S)), np.nonzero(lab != R.select(v, S))[0]
    assert int(lab.sum()) == S
    w = (v * lab).astype(f32)
    T2 = kernels.rigid_transform_3d(_t(d["src"][None], dev), _t(d["tgt"][None], dev), _t(w[None], dev))[0].cpu().numpy()
    assert np.isfinite(T).all()
    assert np.array_equal(_bits(T), _bits(T2))


# ------------------------------------------------------------------- M
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_compat_bits(c, gpu_device):
    """sm_compat == matrix() bit for bit (contraction off, IEEE sqrtf and /), the
    diagonal +0, the guard row behind M untouched."""
    d = R.random_case(*c)
    M, guard = _gpu_compat(d, gpu_device)
    diff = int((_bits(M) != _bits(d["M"])).sum())
    print(f"{R.case_id(c)}: {diff} of {M.size} elements differ")
    assert diff == 0
    assert not _bits(np.diag(M)).any()
    assert np.isnan(guard).all()


@pytest.mark.parametrize("key", [(2500, 900, 500), (70, 30, 20)], ids=lambda k: "N%d-a%d-b%d" % k)
def test_compat_bits_tie_case(key, gpu_device):
    d = R.tie_case(*key)
    M, guard = _gpu_compat(d, gpu_device)
    assert np.array_equal(_bits(M), _bits(d["M"]))
    assert np.isnan(guard).all()


# -------------------------------------------------------------- matvec
def _matvec(M, v, dev):
    """pdsc_sm_matvec with MATVEC_PAD NaNs behind M and behind v: a read past either
    end poisons the row."""
    from pointdsc_amd.baselines import sm_matvec
    N = len(v)
    Mv, _ = _guarded(N * N, dev)
    vv, _ = _guarded(N, dev)
    Mv.copy_(_t(M, dev).reshape(-1))
    vv.copy_(_t(v, dev))
    return sm_matvec(Mv.view(N, N), vv).cpu().numpy()


@pytest.mark.parametrize("kind", ["compat", "signed"])
@pytest.mark.parametrize("N", R.SIZES)
def test_matvec_rows(N, kind, gpu_device):
    """Every row within (N + 2) 2^-24 sum_j |M_ij v_j| of the fp64 product: M from
    sm_compat with a positive v, and a random signed M with a signed v."""
    if kind == "compat":
        M, _ = _gpu_compat(R.random_case(N, "3dmatch"), gpu_device)
        v = np.random.RandomState(N).rand(N).astype(f32)
    else:
        M, v = R.signed_matvec_case(N)
    y = _matvec(M, v, gpu_device)
    y64, s = R.row_abs_sums(M, v)
    bound = R.matvec_bound(N, s)
    err = np.abs(y - y64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"N{N}-{kind}: worst |y - y64| / bound {worst:.3g}")
    assert y.shape == (N,)
    assert np.all(err <= bound), np.nonzero(~(err <= bound))[0]


# ------------------------------------------------- one and ten iterates
@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_iterates_and_selection(c, iters, gpu_device):
    """The returned vector against iterate(M, iters, float64) by the envelope rule; the
    selection and the pose on the GPU's own vector; the oracle's pose where the labels
    are the restatement's and the chosen points determine a rotation (rank(H) >= 2)."""
    N, preset = c
    d = R.random_case(N, preset)
    S = R.top_count(N, R.TOP_RATIO)
    T, lab, v = _sm(d, gpu_device, num_iterations=iters)
    v64, nz = d["v64"][iters], d["noise"][iters]
    err = float(np.abs(v - v64).max())
    bound = ENVELOPE * nz + FEAT_FLOOR * float(np.abs(v64).max())
    print(f"{R.case_id(c)} iters {iters}: |v - v64| {err:.3g}, noise {nz:.3g}, err/noise "
          f"{err / nz if nz else float('nan'):.3g}, bound {bound:.3g}")
    assert err <= bound
    _check_selection(d, T, lab, v, S, gpu_device)
    T_ref, lab_ref, _ = R.oracle_run(N, preset, iters)
    same = np.array_equal(lab, R.select(v64, S)) and np.array_equal(lab, lab_ref)
    if same and K.rank_ok(K.kabsch_fp64(d["src"], d["tgt"], v64 * lab_ref)[1]):
        dT = float(np.abs(T - T_ref).max())
        print(f"{R.case_id(c)} iters {iters}: |T - T_oracle| {dT:.3g}")
        assert dT < 1e-4


# ------------------------------------------------------------ exact ties
def _tie_params():
    return [pytest.param(key, ratio, id="N%d-a%d-b%d-r%g" % (key + (ratio,)))
            for key, ratios in R.TIE_CASES.items() for ratio in ratios]


@pytest.mark.parametrize("key,ratio", _tie_params())
def test_exact_ties(key, ratio, gpu_device):
    """One iterate on a tie case: v has three distinct values (row sums are exact in any
    order), and the boundary falls among equal entries -- of the large group, of the
    small one, of the zeros -- which must be taken in index order across 1024-chunks."""
    N, a, b = key
    d = R.tie_case(N, a, b)
    S = R.top_count(N, ratio)
    T, lab, v = _sm(d, gpu_device, num_iterations=1, top_ratio=ratio)
    g = d["group"]
    assert len(np.unique(v)) == 3
    assert np.all(v[g == 1] == v[g == 1][0]) and np.all(v[g == 2] == v[g == 2][0]) and not v[g == 0].any()
    assert v[g == 1][0] > v[g == 2][0] > 0
    v64 = d["v64"][1]
    assert np.abs(v - v64).max() <= ENVELOPE * d["noise"][1] + FEAT_FLOOR * v64.max()
    _check_selection(d, T, lab, v, S, gpu_device)
    # stated directly: the greater groups whole, then the tied group's first members by index
    tied = 1 if S < a else 2 if S < a + b else 0
    idx = np.nonzero(g == tied)[0]
    want = np.zeros(N, f32)
    want[g == 1] = S >= a
    want[g == 2] = S >= a + b
    want[idx[:S - int(want.sum())]] = 1
    assert np.array_equal(lab, want)


@pytest.mark.parametrize("ratio", R.ZERO_ITER_RATIOS)
def test_zero_iterations(ratio, gpu_device):
    """num_iterations = 0: v == 1, every entry tied, labels = the first S indices."""
    d = R.tie_case(2500, 900, 500)
    S = R.top_count(2500, ratio)
    T, lab, v = _sm(d, gpu_device, num_iterations=0, top_ratio=ratio)
    assert np.array_equal(_bits(v), _bits(np.ones(2500, f32)))
    assert np.array_equal(lab, (np.arange(2500) < S).astype(f32))
    _check_selection(d, T, lab, v, S, gpu_device)


# -------------------------------------------------------------- extremes
@pytest.mark.parametrize("N", [10, 65, 1025])
@pytest.mark.parametrize("ratio", [0.0, 1.0])
def test_top_ratio_extremes(N, ratio, gpu_device):
    d = R.random_case(N, "3dmatch")
    T, lab, v = _sm(d, gpu_device, top_ratio=ratio)
    assert np.array_equal(lab, np.full(N, ratio, f32))
    assert np.abs(v - d["v64"][10]).max() <= ENVELOPE * d["noise"][10] + FEAT_FLOOR * np.abs(d["v64"][10]).max()
    _check_selection(d, T, lab, v, int(N * ratio), gpu_device)


@pytest.mark.parametrize("ratio", [0.1, 1.0])
@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("N", [1, 65])
def test_dead_case(N, iters, ratio, gpu_device):
    """No compatible pair: M == 0, v exactly +-0 after any iterate, labels the first S."""
    d = R.dead_case(N)
    M, guard = _gpu_compat(d, gpu_device)
    assert not _bits(M).any() and np.isnan(guard).all()
    S = R.top_count(N, ratio)
    T, lab, v = _sm(d, gpu_device, num_iterations=iters, top_ratio=ratio)
    assert not v.any()
    assert np.array_equal(lab, (np.arange(N) < S).astype(f32))
    _check_selection(d, T, lab, v, S, gpu_device)


# ------------------------------------------------------------ properties
@pytest.mark.parametrize("N", [67, 1028])
def test_two_runs_bitwise(N, gpu_device):
    d = R.random_case(N, "3dmatch")
    a, b = _sm(d, gpu_device), _sm(d, gpu_device)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("N", [67, 1028])
def test_null_leading_eig(N, gpu_device):
    """leading_eig = NULL: the vector lives in the workspace; same labels and trans."""
    from pointdsc_amd._call import call
    d = R.random_case(N, "3dmatch")
    T, lab, _ = _sm(d, gpu_device)
    trans = torch.full((4, 4), float("nan"), dtype=torch.float32, device=gpu_device)
    labels = torch.full((N,), float("nan"), dtype=torch.float32, device=gpu_device)
    call("pdsc_spectral_matching", _t(d["corr"], gpu_device), _t(d["src"], gpu_device), _t(d["tgt"], gpu_device), N,
         float(d["thr"]), float(R.TOP_RATIO), 10, trans, labels, None, device=gpu_device,
         ws=("pdsc_spectral_matching_workspace_bytes", N))
    assert np.array_equal(_bits(labels.cpu().numpy()), _bits(lab))
    assert np.array_equal(_bits(trans.cpu().numpy()), _bits(T))


@pytest.mark.parametrize("N", [67, 1028])
def test_non_contiguous_corr(N, gpu_device):
    """A strided view of corr gives the bits of its contiguous copy (SM and sm_compat)."""
    from pointdsc_amd.baselines import SM, sm_compat
    d = R.random_case(N, "3dmatch")
    wide = torch.full((1, N, 12), float("nan"), dtype=torch.float32, device=gpu_device)
    wide[..., ::2] = _t(d["corr"][None], gpu_device)
    view = wide[..., ::2]
    assert not view.is_contiguous()
    src, tgt = _t(d["src"][None], gpu_device), _t(d["tgt"][None], gpu_device)
    got = SM(view, src, tgt, inlier_threshold=d["thr"], return_eig=True)
    want = SM(view.contiguous(), src, tgt, inlier_threshold=d["thr"], return_eig=True)
    for x, y in zip(got, want):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy()))
    assert np.array_equal(_bits(sm_compat(view[0], d["thr"]).cpu().numpy()), _bits(d["M"]))
