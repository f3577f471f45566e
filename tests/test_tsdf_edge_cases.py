"""The TSDF edge cases on the CPU (tests/tsdf_edge_cases.py): every case's
preconditions on the restatement, the restatement's extract() against a brute-force
per-edge restatement of the contract sentence, and the proof that the GPU file's
assertions tell a right volume from one with a single rule broken."""
import numpy as np
import pytest

import fragments_reference as R
import tsdf_edge_cases as T

f32 = np.float32
IC, EC = T.integrate_cases(), T.extraction_cases()
GROUP_CASES = [n for n in EC if n.startswith("group_")] + ["dense_checker"]


# ------------------------------------------------------------------ integrate preconditions
def _touched(case, depth, E):
    return R.Volume(case.vl, case.trunc).touched(depth, case.K, E)


@pytest.mark.parametrize("size", T.SIZES)
def test_size_cases(size):
    H, W = size
    case = IC[f"size_{H}x{W}"]
    vol, snaps = T.reference_run(case.name)
    assert len(vol.blocks) >= 1 and vol.stats["integrated"] > 0 and vol.sorted_blocks()[2].max() == 2.0
    if H % 4 or W % 4:
        d, _, E = case.frames[0]
        part = np.zeros((H, W), bool)
        part[4 * (H // 4):, :] = True
        part[:, 4 * (W // 4):] = True
        only = _touched(case, np.where(part, d, 0), E) - _touched(case, np.where(part, 0, d), E)
        assert only, "a block must come from the last partial column or row alone"


def test_edge_uv_case():
    vol, _ = T.reference_run("edge_uv")
    assert vol.stats["u_neg"] >= 8 and vol.stats["v_neg"] >= 8 and vol.stats["u_out"] >= 8, vol.stats


def test_camera_inside_case():
    vol, _ = T.reference_run("camera_inside")
    assert vol.stats["pz_le0"] >= 8 and vol.stats["integrated"] >= 8, vol.stats


def test_dyadic_case():
    case = IC["dyadic"]
    assert all(float(x) * 1024 == int(float(x) * 1024) for x in (case.vl, case.trunc, case.frames[0][0][0, 0]))
    vol, _ = T.reference_run("dyadic")
    assert vol.stats["sdf_eq_lo"] >= 8 and vol.stats["sdf_eq_hi"] >= 8, vol.stats
    # frame 1 alone: the plane i = 68 (voxel z = 4 of the blocks at bz = 4) stays at weight 0 beside integrated
    # planes, the plane i = 60 (z = 12 at bz = 3) holds exactly 1
    once = T.run_reference(T.IntegrateCase("once", case.vl, case.trunc, case.K, case.frames[:1]))[0]
    assert once.stats["sdf_eq_lo"] * 2 == vol.stats["sdf_eq_lo"]
    z = T.OFF[:, 2]
    lo = sum(int((b[1][z == 3] == 1).sum()) for k, b in once.blocks.items() if k[2] == 4)
    assert lo >= once.stats["sdf_eq_lo"]
    assert all((b[1][z == 4] == 0).all() for k, b in once.blocks.items() if k[2] == 4)
    hi = [b[0][(z == 12) & (b[1] == 1)] for k, b in once.blocks.items() if k[2] == 3]
    assert sum(len(h) for h in hi) >= once.stats["sdf_eq_hi"] and all((h == 1).all() for h in hi)


def test_bad_depth_cases():
    case = IC["bad_depth"]
    d = case.frames[1][0]
    with np.errstate(invalid="ignore"):
        assert (d[::4, ::4] == 0).any() and (d[::4, ::4] < 0).any() and np.isnan(d[::4, ::4]).any()
        assert np.isnan(d).sum() > np.isnan(d[::4, ::4]).sum() and (d == 0).sum() > (d[::4, ::4] == 0).sum()
    vol, snaps = T.reference_run("bad_depth")
    assert vol.stats["integrated"] > 0 and vol.sorted_blocks()[2].max() == 3.0
    assert np.isfinite(vol.sorted_blocks()[1]).all() and np.isfinite(vol.sorted_blocks()[3]).all()
    # +inf in a sampled pixel: the range error, and nothing changes although the other samples reach new blocks
    case = IC["bad_depth_inf"]
    d, _, E = case.frames[1]
    assert np.isposinf(d[::4, ::4]).sum() == 1
    vol, snaps = T.reference_run("bad_depth_inf")
    T.assert_blocks_bitwise(snaps[1][1], snaps[0][1])
    assert _touched(case, np.where(np.isinf(d), 0, d), E) - set(vol.blocks)


def test_truncation_and_voxel_length_cases():
    case = IC["big_trunc"]
    assert case.trunc > 16 * case.vl
    for d, _, E in case.frames:
        for v, u in ((0, 0), (0, 4)):
            one = np.zeros_like(d)
            one[v, u] = d[v, u]
            t = np.array(sorted(_touched(case, one, E)))
            assert len(t) >= 27 and all(t[:, a].max() - t[:, a].min() >= 2 for a in range(3))
    assert len(T.reference_run("big_trunc")[0].blocks) <= 512
    assert IC["tiny_trunc"].trunc < IC["tiny_trunc"].vl and T.reference_run("tiny_trunc")[0].stats["integrated"] > 0
    vls = {c.vl for c in IC.values()}
    assert len(vls - {0.01}) >= 2 and any(np.log2(v) == round(np.log2(v)) for v in vls)
    assert T.reference_run("vl_0.023")[0].stats["integrated"] > 0
    for name in IC:
        assert len(T.reference_run(name)[0].blocks) <= 512, name


def test_subset5_case():
    vol, snaps = T.reference_run("subset5")
    for (t0, _), (t1, _) in zip(snaps, snaps[1:]):
        assert t1 < t0, "each frame must touch a strict subset of the one before"
    assert vol.sorted_blocks()[2].max() == 5.0 and vol.sorted_blocks()[2].min() == 0.0
    for (_, before), (touched, after) in zip(snaps, snaps[1:]):
        assert np.array_equal(before[0], after[0])
        same = [i for i, k in enumerate(map(tuple, before[0].tolist())) if k not in touched]
        assert same
        T.assert_blocks_bitwise([x[same] for x in after], [x[same] for x in before])


def test_overflow_case_and_the_restatements_overflow_rule():
    case, n2 = T.overflow_case()
    vol = R.Volume(case.vl, case.trunc, case.max_blocks)
    for d, c, E in case.frames[:2]:
        assert vol.integrate(d, c, case.K, E)
    before = tuple(x.copy() for x in vol.sorted_blocks())
    d, c, E = case.frames[2]
    new = vol.touched(d, case.K, E) - set(vol.blocks)
    assert len(new) > 3 and len(vol.blocks) == n2
    assert vol.integrate(d, c, case.K, E) is False
    assert len(vol.blocks) == case.max_blocks
    keys = [tuple(k) for k in vol.sorted_blocks()[0].tolist()]
    old = [i for i, k in enumerate(keys) if k not in new]
    T.assert_blocks_bitwise([x[old] for x in vol.sorted_blocks()], before)
    for k in set(vol.blocks) & new:
        assert not vol.blocks[k][0].any() and not vol.blocks[k][1].any() and not vol.blocks[k][2].any()
    # `slotted` names which of the frame's blocks got the slots; anything else is refused
    other = R.Volume(case.vl, case.trunc, case.max_blocks)
    for dd, cc, EE in case.frames[:2]:
        other.integrate(dd, cc, case.K, EE)
    pick = sorted(new)[-3:]
    assert other.integrate(d, c, case.K, E, slotted=pick) is False and set(other.blocks) - set(keys[i] for i in old) == set(pick)
    with pytest.raises(AssertionError):
        R.Volume(case.vl, case.trunc, 2).integrate(d, c, case.K, E, slotted=[(0, 0, 0), (9, 9, 9)])
    d, c, E = case.frames[3]
    assert vol.touched(d, case.K, E) <= set(vol.blocks)
    assert vol.integrate(d, c, case.K, E) and len(vol.blocks) == case.max_blocks
    assert vol.sorted_blocks()[2].max() == 3.0


def test_restatement_write_blocks():
    """write_blocks in the restatement: the round trip, found-not-duplicated, both errors."""
    sets = T.hash_sets()
    assert len(sets) == 40 and all(len({tuple(r) for r in s.tolist()}) == 16 for s in sets)
    assert all(np.abs(s).max() < 3 for s in sets[:20]) and all(np.abs(s).max() > 1000 for s in sets[20:])
    assert all((s < 0).any() and (s >= 0).any() for s in sets)
    more = T.wrap_sets()
    assert len(more) == T.N_WRAP_SETS and all(len({tuple(r) for r in s.tolist()}) == 16 for s in more)
    assert 0.9747 ** (20 + len(more)) < 2e-7  # the bound of wrap_sets' docstring
    vol = R.Volume(0.01, 0.04, 16)
    t, w, c = T.block_data(16, 1)
    vol.write_blocks(sets[0][:8], t[:8], w[:8], c[:8])
    vol.write_blocks(sets[0][4:], t[4:], w[4:], c[4:])
    assert len(vol.blocks) == 16
    order = np.argsort(R.block_key(sets[0]))
    T.assert_blocks_bitwise(vol.sorted_blocks(), (sets[0][order], t[order], w[order], c[order]))
    with pytest.raises(R.TsdfError, match="full"):
        vol.write_blocks(sets[1][:1], t[:1], w[:1], c[:1])
    for bad in T.OUTSIDE:
        with pytest.raises(R.TsdfError, match="outside"):
            vol.write_blocks(bad[None], t[:1], w[:1], c[:1])
    T.assert_blocks_bitwise(vol.sorted_blocks(), (sets[0][order], t[order], w[order], c[order]))


# ------------------------------------------------------------------ extraction: the contract sentence, edge by edge
def _brute_force(vol):
    """"The edge (v, axis) is emitted once iff (f0 < 0) != (f1 < 0) and at least one of its four adjacent cubes
    is valid", by loops over blocks in key order, voxels and axes; no helper of the restatement is used.  Returns
    (rows [(key, voxel, axis, x, y, z, r, g, b)], the number of valid adjacent cubes per row, the number of
    sign-changing edges that are not emitted)."""
    grid = {}
    for (bx, by, bz), (t, w, c) in vol.blocks.items():
        tl, wl, cl = t.tolist(), w.tolist(), c.tolist()
        for i in range(4096):
            grid[(16 * bx + i % 16, 16 * by + (i // 16) % 16, 16 * bz + i // 256)] = (tl[i], wl[i], cl[i])
    valid = {}

    def cube(x, y, z):
        got = valid.get((x, y, z))
        if got is None:
            got = True
            for dx in (0, 1):
                for dy in (0, 1):
                    for dz in (0, 1):
                        corner = grid.get((x + dx, y + dy, z + dz))
                        if corner is None or corner[1] == 0.0:
                            got = False
            valid[(x, y, z)] = got
        return got

    rows, alive, silent = [], [], 0
    keyed = sorted((((bx + 2 ** 20) << 42) | ((by + 2 ** 20) << 21) | (bz + 2 ** 20), (bx, by, bz)) for bx, by, bz in vol.blocks)
    for key, (bx, by, bz) in keyed:
        for i in range(4096):
            v = (16 * bx + i % 16, 16 * by + (i // 16) % 16, 16 * bz + i // 256)
            f0, _, c0 = grid[v]
            for axis in range(3):
                e = tuple(v[a] + (a == axis) for a in range(3))
                if e not in grid:
                    continue  # the other end does not exist: none of the four cubes has all its corners
                f1, _, c1 = grid[e]
                if (f0 < 0) == (f1 < 0):
                    continue
                o1, o2 = [a for a in range(3) if a != axis]
                n = 0
                for s1 in (0, 1):
                    for s2 in (0, 1):
                        q = list(v)
                        q[o1] -= s1
                        q[o2] -= s2
                        n += cube(*q)
                if n == 0:
                    silent += 1
                    continue
                a0, a1 = abs(f0), abs(f1)
                p = [(g + 0.5) * vol.vl for g in v]
                p[axis] += a0 * vol.vl / (a0 + a1)
                rows.append([key, i, axis] + p + [(a1 * c0[ch] + a0 * c1[ch]) / (a0 + a1) / 255.0 for ch in range(3)])
                alive.append(n)
    return rows, np.array(alive), silent


@pytest.mark.parametrize("name", GROUP_CASES)
def test_extract_matches_the_contract_sentence(name):
    vol, p, c, keys = T.reference_extract(name)
    rows, alive, silent = _brute_force(vol)
    assert len(rows) == len(p) > 0
    rows = np.array(rows, dtype=object)
    assert np.array_equal(rows[:, :3].astype(np.int64), keys)  # the same edges, in the same order
    assert np.abs(rows[:, 3:6].astype(np.float64) - p).max() <= 1e-15 * np.abs(p).max()
    assert np.abs(rows[:, 6:9].astype(np.float64) - c).max() <= 1e-15
    if "_w0_seed" in name:
        assert (alive == 1).sum() > 0, "some edge must live on exactly one valid cube"
        assert silent > 0, "some sign change must stay silent"
    if name == "group_centre_w0":
        assert silent >= 1


# ------------------------------------------------------------------ extraction preconditions
def _keyset(name):
    return {tuple(k) for k in T.reference_extract(name)[3].tolist()}


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_group_removals(kind):
    """Every removal loses points.  An edge based in ANOTHER block goes only if it ends in the removed block (an
    edge that ends elsewhere keeps its own base cube or the one below it), so the base lies across a face in a
    block of the group with a lower index: never for the lowest block (-1, -1, -1), and for a block at index -1
    along z only where the surface cuts the x or y face beside it.  The sphere does that for all seven blocks that
    have a lower neighbour; the plane, which lies along z = 0, for the four blocks at z = 0 and, below them, for
    (0, 0, -1) alone, whose x and y faces its tilt cuts."""
    full, case = _keyset(f"group_{kind}"), EC[f"group_{kind}"]
    assert (case.weight != 0).all()
    assert not np.array_equal(case.coords, case.coords[np.argsort(R.block_key(case.coords))]), "written in key order"
    foreign = []
    for i in range(8):
        gone = int(R.block_key(case.coords[i]))
        lost = full - _keyset(f"group_{kind}_minus_{i}")
        assert _keyset(f"group_{kind}_minus_{i}") < full and lost
        if any(k[0] != gone for k in lost):
            foreign.append(tuple(int(x) for x in case.coords[i]))
    if kind == "sphere":
        assert set(foreign) == set(T.GROUP) - {(-1, -1, -1)}, foreign
    else:  # the four blocks above the plane through the z face, and (0, 0, -1) through its x and y faces
        assert set(foreign) == {b for b in T.GROUP if b[2] == 0} | {(0, 0, -1)}, foreign


def test_group_crossings():
    """Sign changes across every face, every edge and the centre corner of the group: emitted edges whose two
    ends lie in different blocks, per axis, and cubes at local (15, *, *) .. (15, 15, 15) with a sign change."""
    for kind in ("plane", "sphere"):
        keys = T.reference_extract(f"group_{kind}")[3]
        v = T.OFF[keys[:, 1]]
        for a in range(3):
            assert ((keys[:, 2] == a) & (v[:, a] == 15)).any(), "an edge through the face across axis %d" % a
    vol = T.reference_extract("group_plane")[0]
    near = [vol.blocks[k][0][T.OFF @ [1, 16, 256]][(T.OFF == np.where(np.array(k) < 0, 15, 0)).all(1)] for k in T.GROUP]
    near = np.concatenate(near)  # the 8 voxels around the centre corner
    assert (near < 0).any() and (near > 0).any()


def test_zero_single_extreme_and_dense_cases():
    case = EC["group_zeros"]
    bits = case.tsdf.view(np.uint32)
    assert (bits == 0).sum() > 1000 and (bits == 0x80000000).sum() > 1000
    # a zero of either sign beside a negative voxel is an emitted edge; beside a positive one it is not
    vol, p, c, keys = T.reference_extract("group_zeros")
    blk = {int(R.block_key(k)): vol.blocks[k] for k in vol.blocks}
    f0 = np.array([blk[k][0][v] for k, v, _ in keys.tolist()])
    assert (f0.view(np.uint32) == 0).any() and (f0.view(np.uint32) == 0x80000000).any()
    assert np.isfinite(p).all() and np.isfinite(c).all()
    # one block alone: only edges that end inside it, and sign changes towards the absent neighbours stay silent
    vol, p, _, keys = T.reference_extract("single_block")
    v = T.OFF[keys[:, 1]]
    assert len(p) > 100 and (v[np.arange(len(v)), keys[:, 2]] <= 14).all()
    t = vol.blocks[(3, -2, 5)][0]
    assert any((t[T.OFF[:, a] == 15] < 0).any() for a in range(3))
    # extreme coordinates: points from the lone block and across the pair's shared face
    vol, p, _, keys = T.reference_extract("extreme")
    ks = sorted(int(R.block_key(k)) for k in vol.blocks)
    assert (keys[:, 0] == ks[0]).any() and ((keys[:, 2] == 0) & (T.OFF[keys[:, 1], 0] == 15)).any()
    assert np.abs(p).max() > 0.01 * 16 * (2 ** 20 - 1)
    # the dense block: every voxel, every axis; before it a block with no edge, before that one with some
    vol, p, _, keys = T.reference_extract("dense_checker")
    ks = sorted(int(R.block_key(k)) for k in vol.blocks)
    count = [int((keys[:, 0] == k).sum()) for k in ks]
    assert ks[2] == int(R.block_key((-1, -1, -1))) and count[0] > 0 and count[1] == 0 and count[2] == 3 * 4096
    assert 0 < max(count[3:]) < 3 * 4096 // 2


# ------------------------------------------------------------------ the assertions can tell right from wrong
class SampleFloor(R.Volume):
    def sample_grid(self, H, W):
        return np.arange(H // 4) * 4, np.arange(W // 4) * 4


class PixelFloor(R.Volume):
    def pixel(self, xf):
        return np.floor(xf).astype(np.int64)


class KeepEqual(R.Volume):
    def keep(self, sdf):
        return sdf >= -self.trunc


class IntegrateAll(R.Volume):
    def integration_set(self, touched):
        return set(self.blocks)


class NoDiagonal(R.Volume):
    def cube_valid(self, nz):
        loose = nz.copy()
        loose[0::16, 0::16, 0::16] = True  # voxel (0, 0, 0) of every block: the corner-diagonal neighbour's only corner
        cube = super().cube_valid(loose)
        strict = super().cube_valid(nz)
        at = np.zeros(nz.shape, bool)
        at[15::16, 15::16, 15::16] = True
        return np.where(at, cube, strict)


class NegativeOrZero(R.Volume):
    def negative(self, F):
        return F <= 0


class BaseCubeOnly(R.Volume):
    def edge_alive(self, cube, o1, o2):
        return cube


class SlotOrder(R.Volume):
    def block_rank(self, blk):
        slot = {int(R.block_key(k)): i for i, k in enumerate(self.blocks)}  # the order they were written in
        return np.array([slot[int(k)] for k in R.block_key(blk)])


INTEGRATE_DEFECTS = {SampleFloor: "size_3x5", PixelFloor: "edge_uv", KeepEqual: "dyadic", IntegrateAll: "subset5"}
EXTRACT_DEFECTS = {NoDiagonal: "group_centre_w0", NegativeOrZero: "group_zeros", BaseCubeOnly: "group_sphere_w0_seed1",
                   SlotOrder: "group_plane"}


@pytest.mark.parametrize("defect", list(INTEGRATE_DEFECTS), ids=lambda d: d.__name__)
def test_integrate_defects_fall_outside_the_bars(defect):
    name = INTEGRATE_DEFECTS[defect]
    wrong, _ = T.run_reference(IC[name], defect)
    with pytest.raises(AssertionError):
        T.assert_blocks_equal(wrong.sorted_blocks(), T.reference_run(name)[0])


@pytest.mark.parametrize("defect", list(EXTRACT_DEFECTS), ids=lambda d: d.__name__)
def test_extract_defects_fall_outside_the_bars(defect):
    name = EXTRACT_DEFECTS[defect]
    wrong = EC[name].volume(defect)
    T.assert_blocks_bitwise(wrong.sorted_blocks(), T.reference_extract(name)[0].sorted_blocks())
    p, c, _ = wrong.extract()
    _, rp, rc, _ = T.reference_extract(name)
    with pytest.raises(AssertionError):
        T.assert_points_equal(p, c, rp, rc, EC[name].vl)


def test_every_defect_is_caught_by_more_than_its_own_case():
    """The removal cases catch the two validity defects as well (not only the weight-0 states)."""
    caught = {NoDiagonal: 0, BaseCubeOnly: 0}
    for defect in caught:
        for i in range(8):
            name = f"group_plane_minus_{i}"
            p, c, _ = EC[name].volume(defect).extract()
            _, rp, rc, _ = T.reference_extract(name)
            try:
                T.assert_points_equal(p, c, rp, rc, EC[name].vl)
            except AssertionError:
                caught[defect] += 1
    assert caught[NoDiagonal] >= 1 and caught[BaseCubeOnly] >= 4, caught
