"""The sparse TSDF volume on the GPU (csrc/tsdf.hip, include/pdsc.h f14) at the edge
cases of tests/tsdf_edge_cases.py, against tests/fragments_reference.Volume, at
test_gpu_tsdf.py's bars: block sets, n_blocks, weights and point counts exact;
tsdf and colour within 2 fp32 ulps; extracted positions within 1e-6
voxel_length and colours within 1e-6, row by row in the emitted order; a
read-back of written blocks bitwise.  blocks() sorts by key: slot order is not
part of the contract.  tests/test_tsdf_edge_cases.py asserts each case's
preconditions and shows that these assertions reject a volume with one rule
broken.

Left out: the grid-stride branch of tsdf_integrate_kernel (more than 8192 touched
blocks in one frame: a fabricated state of several hundred MB), and duplicate
coordinates within one write_blocks call, which the contract leaves undefined.
Every volume here has max_blocks <= 512."""
import numpy as np
import pytest
import torch

import fragments_reference as R
import tsdf_edge_cases as T
from pointdsc_amd import fragments as F

pytestmark = pytest.mark.gpu

IC, EC = T.integrate_cases(), T.extraction_cases()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _integrate(vol, frame, K, dev):
    d, c, E = frame
    vol.integrate(_t(d, dev), _t(c, dev), K, _t(E, dev))


def _bits(blocks):
    return tuple(x.cpu().numpy() for x in blocks)


def _assert_untouched_bitwise(before, after, touched):
    """Every block of `before` that is not in `touched` is bit for bit the same in `after`."""
    at = {tuple(k): i for i, k in enumerate(after[0].tolist())}
    same = [(i, at[tuple(k)]) for i, k in enumerate(before[0].tolist()) if tuple(k) not in touched]
    i0, i1 = [s[0] for s in same], [s[1] for s in same]
    T.assert_blocks_bitwise([x[i1] for x in after], [x[i0] for x in before])
    return len(same)


# ------------------------------------------------------------------ integrate
@pytest.mark.parametrize("name", [n for n in IC if IC[n].error is None])
def test_integrate_case(gpu_device, name):
    case = IC[name]
    _, snaps = T.reference_run(name)
    vol = F.TSDFVolume(case.vl, case.trunc, case.max_blocks, gpu_device)
    worst, before = 0, None
    for frame, (touched, expect) in zip(case.frames, snaps):
        _integrate(vol, frame, case.K, gpu_device)
        assert vol.n_blocks == len(expect[0])
        after = _bits(vol.blocks())
        worst = max(worst, T.assert_blocks_equal(after, expect))
        if before is not None:
            _assert_untouched_bitwise(before, after, touched)
        before = after
    print(f"{name}: {vol.n_blocks} blocks, worst ulp {worst}")


def test_subset5_untouched_blocks_stay(gpu_device):
    """Frame k touches a strict subset of frame k - 1's blocks; the rest keep their bits."""
    case = IC["subset5"]
    _, snaps = T.reference_run("subset5")
    vol = F.TSDFVolume(case.vl, case.trunc, case.max_blocks, gpu_device)
    before = None
    for frame, (touched, _) in zip(case.frames, snaps):
        _integrate(vol, frame, case.K, gpu_device)
        after = _bits(vol.blocks())
        if before is not None:
            assert _assert_untouched_bitwise(before, after, touched) >= 1
        before = after
    assert after[2].max() == 5.0


def test_inf_depth_is_a_range_error_and_changes_nothing(gpu_device):
    case = IC["bad_depth_inf"]
    ref, _ = T.run_reference(case)  # its own copy: this test integrates one more frame into it
    vol = F.TSDFVolume(case.vl, case.trunc, case.max_blocks, gpu_device)
    _integrate(vol, case.frames[0], case.K, gpu_device)
    before, n = _bits(vol.blocks()), vol.n_blocks
    with pytest.raises(RuntimeError, match="outside"):
        _integrate(vol, case.frames[1], case.K, gpu_device)
    assert vol.n_blocks == n
    T.assert_blocks_bitwise(_bits(vol.blocks()), before)
    T.assert_blocks_equal(vol.blocks(), ref)
    # and the volume still works: the same frame without the inf integrates like the restatement's
    d, c, E = case.frames[1]
    d = np.where(np.isinf(d), 0, d).astype(np.float32)
    assert ref.integrate(d, c, case.K, E)
    _integrate(vol, (d, c, E), case.K, gpu_device)
    T.assert_blocks_equal(vol.blocks(), ref)


def test_overflow_of_a_volume_that_holds_data(gpu_device):
    case, n2 = T.overflow_case()
    ref = R.Volume(case.vl, case.trunc, case.max_blocks)
    vol = F.TSDFVolume(case.vl, case.trunc, case.max_blocks, gpu_device)
    for frame in case.frames[:2]:
        assert ref.integrate(frame[0], frame[1], case.K, frame[2])
        _integrate(vol, frame, case.K, gpu_device)
    assert vol.n_blocks == n2
    before = _bits(vol.blocks())
    T.assert_blocks_equal(before, ref)
    d, c, E = case.frames[2]
    new = ref.touched(d, case.K, E) - set(ref.blocks)
    with pytest.raises(RuntimeError, match="full"):
        _integrate(vol, case.frames[2], case.K, gpu_device)
    assert vol.n_blocks == case.max_blocks
    after = _bits(vol.blocks())
    assert _assert_untouched_bitwise(before, after, set()) == n2  # every voxel of every earlier block
    slotted = [i for i, k in enumerate(after[0].tolist()) if tuple(k) not in ref.blocks]
    assert len(slotted) == case.max_blocks - n2 and all(tuple(after[0][i].tolist()) in new for i in slotted)
    assert not after[1][slotted].any() and not after[2][slotted].any() and not after[3][slotted].any()
    p, _ = vol.extract_surface_points()
    assert ref.integrate(d, c, case.K, E, slotted=[tuple(after[0][i].tolist()) for i in slotted]) is False
    assert p.shape[0] == len(ref.extract()[0])
    # a frame that touches only blocks the volume holds integrates as if nothing had happened
    frame = case.frames[3]
    assert ref.touched(frame[0], case.K, frame[2]) <= set(ref.blocks)
    assert ref.integrate(frame[0], frame[1], case.K, frame[2])
    _integrate(vol, frame, case.K, gpu_device)
    assert vol.n_blocks == case.max_blocks
    T.assert_blocks_equal(vol.blocks(), ref)
    rp, rc, _ = ref.extract()
    p, c = vol.extract_surface_points()
    print("overflow: position / colour error", T.assert_points_equal(p, c, rp, rc, case.vl))


# ------------------------------------------------------------------ hash and capacity
def _write(vol, coords, t, w, c, dev, idx=slice(None)):
    vol.write_blocks(_t(coords[idx], dev), _t(t[idx], dev), _t(w[idx], dev), _t(c[idx], dev))


def _sorted(coords, t, w, c):
    order = np.argsort(R.block_key(coords))
    return coords[order], t[order], w[order], c[order]


def test_hash_round_trips(gpu_device):
    """40 sets of 16 blocks in a table of 64 entries (25 % load), from a small cube and from the whole range.  The
    hash function is not restated: with 16 keys in 64 entries a set has a collision with probability 1 - 64! /
    (48! 64^16) > 0.87 under any hash that spreads keys, so over 40 sets and three write patterns chains through
    foreign keys are certain whatever the function.  The wrap at the table's end is rarer and has a test of its own
    below."""
    for s, coords in enumerate(T.hash_sets()):
        t, w, c = T.block_data(16, 500 + s)
        want = _sorted(coords, t, w, c)
        one = F.TSDFVolume(0.01, 0.04, 16, gpu_device)
        _write(one, coords, t, w, c, gpu_device)
        assert one.n_blocks == 16
        T.assert_blocks_bitwise(_bits(one.blocks()), want)
        two = F.TSDFVolume(0.01, 0.04, 16, gpu_device)
        _write(two, coords, t, w, c, gpu_device, slice(0, 8))
        assert two.n_blocks == 8
        T.assert_blocks_bitwise(_bits(two.blocks()), _sorted(coords[:8], t[:8], w[:8], c[:8]))
        _write(two, coords, t, w, c, gpu_device, slice(8, 16))
        assert two.n_blocks == 16
        T.assert_blocks_bitwise(_bits(two.blocks()), want)
        # again after a partial overlap: blocks 4 .. 15 with other voxels; found, not duplicated
        t2, w2, c2 = T.block_data(16, 900 + s)
        _write(two, coords, t2, w2, c2, gpu_device, slice(4, 16))
        assert two.n_blocks == 16
        mixed = [np.concatenate([a[:4], b[4:]]) for a, b in ((t, t2), (w, w2), (c, c2))]
        T.assert_blocks_bitwise(_bits(two.blocks()), _sorted(coords, *mixed))


def test_hash_wrap_at_the_tables_end(gpu_device):
    """tsdf_edge_cases.wrap_sets(): enough whole-range sets that a probe from the last entry to entry 0 fails to
    occur with probability below 2e-7 under any hash that spreads keys (the bound is in its docstring).  Each set
    is written in two overlapping calls into a reset volume, so both the insertion and the look-up of existing
    keys cross the table's end, and read back bitwise."""
    pools = [T.block_data(16, 700 + k) for k in range(4)]
    dev_pools = [tuple(_t(x, gpu_device) for x in p) for p in pools]
    vol = F.TSDFVolume(0.01, 0.04, 16, gpu_device)
    for s, coords in enumerate(T.wrap_sets()):
        a, b = s % 4, (s + 1) % 4
        cd = _t(coords, gpu_device)
        vol.reset()
        vol.write_blocks(cd[:8], *(x[:8] for x in dev_pools[a]))
        assert vol.n_blocks == 8
        vol.write_blocks(cd[4:], *(x[4:] for x in dev_pools[b]))
        assert vol.n_blocks == 16, s
        mixed = [np.concatenate([x[:4], y[4:]]) for x, y in zip(pools[a], pools[b])]
        T.assert_blocks_bitwise(_bits(vol.blocks()), _sorted(coords, *mixed))


@pytest.mark.parametrize("max_blocks", [1, 2, 16, 64])
def test_capacity_and_range_errors_of_write_blocks(gpu_device, max_blocks):
    rng = np.random.default_rng(max_blocks)
    coords = np.unique(rng.integers(-5, 5, (4 * max_blocks + 8, 3)), axis=0)
    coords = coords[rng.permutation(len(coords))][:max_blocks + 1].astype(np.int32)
    t, w, c = T.block_data(max_blocks + 1, 40 + max_blocks)
    vol = F.TSDFVolume(0.01, 0.04, max_blocks, gpu_device)
    _write(vol, coords, t, w, c, gpu_device, slice(0, max_blocks))
    want = _sorted(coords[:max_blocks], t[:max_blocks], w[:max_blocks], c[:max_blocks])
    assert vol.n_blocks == max_blocks
    T.assert_blocks_bitwise(_bits(vol.blocks()), want)
    for bad in T.OUTSIDE:  # alone, and among blocks that exist
        for rows in (bad[None], np.concatenate([coords[:1], bad[None]])[:max_blocks + 1]):
            with pytest.raises(RuntimeError, match="outside"):
                _write(vol, rows, t, w, c, gpu_device, slice(0, len(rows)))
            assert vol.n_blocks == max_blocks
    T.assert_blocks_bitwise(_bits(vol.blocks()), want)
    with pytest.raises(RuntimeError, match="full"):  # one block too many, alone
        _write(vol, coords[max_blocks:], t[:1], w[:1], c[:1], gpu_device)
    assert vol.n_blocks == max_blocks
    T.assert_blocks_bitwise(_bits(vol.blocks()), want)
    # max_blocks + 1 blocks in one call into an empty volume: full, no voxel written, max_blocks of them at weight 0
    vol = F.TSDFVolume(0.01, 0.04, max_blocks, gpu_device)
    with pytest.raises(RuntimeError, match="full"):
        _write(vol, coords, t, w, c, gpu_device)
    got = _bits(vol.blocks())
    assert vol.n_blocks == max_blocks and len(np.unique(got[0], axis=0)) == max_blocks
    assert {tuple(k) for k in got[0].tolist()} <= {tuple(k) for k in coords.tolist()}
    assert not got[1].any() and not got[2].any() and not got[3].any()
    # a range error in an empty volume gives no block a slot, whatever else the call names
    vol = F.TSDFVolume(0.01, 0.04, max_blocks, gpu_device)
    rows = np.concatenate([coords[:max_blocks - 1], T.OUTSIDE[:1]]) if max_blocks > 1 else T.OUTSIDE[:1]
    with pytest.raises(RuntimeError, match="outside"):
        _write(vol, rows, t, w, c, gpu_device, slice(0, len(rows)))
    assert vol.n_blocks == 0


def test_extreme_block_indices_round_trip(gpu_device):
    t, w, c = T.block_data(len(T.EXTREME), 66)
    vol = F.TSDFVolume(0.01, 0.04, 16, gpu_device)
    _write(vol, T.EXTREME, t, w, c, gpu_device)
    assert vol.n_blocks == len(T.EXTREME)
    T.assert_blocks_bitwise(_bits(vol.blocks()), _sorted(T.EXTREME, t, w, c))
    ref = R.Volume(0.01, 0.04, 16)
    ref.write_blocks(T.EXTREME, t, w, c)
    rp, rc, _ = ref.extract()  # the +1 neighbours of the highest indices are out of range: absent
    p, col = vol.extract_surface_points()
    T.assert_points_equal(p, col, rp, rc, 0.01)


# ------------------------------------------------------------------ extraction
@pytest.mark.parametrize("name", list(EC))
def test_extraction_case(gpu_device, name):
    case = EC[name]
    ref, rp, rc, _ = T.reference_extract(name)
    vol = F.TSDFVolume(case.vl, 4 * case.vl, 32, gpu_device)
    _write(vol, case.coords, case.tsdf, case.weight, case.colour, gpu_device)
    assert vol.n_blocks == len(case.coords)
    T.assert_blocks_bitwise(_bits(vol.blocks()), ref.sorted_blocks())
    p, c = vol.extract_surface_points()
    p2, c2 = vol.extract_surface_points()
    assert torch.equal(p, p2) and torch.equal(c, c2)
    assert p.shape[0] == len(rp) > 0
    print(f"{name}: {len(rp)} points, position / colour error", T.assert_points_equal(p, c, rp, rc, case.vl))
    T.assert_blocks_bitwise(_bits(vol.blocks()), ref.sorted_blocks())  # extraction changes no voxel
