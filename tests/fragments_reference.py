"""A numpy restatement of include/pdsc.h f13 (RGB-D odometry, hybrid term) and f14
(sparse TSDF volume), written from the contract: the geometry in fp64, fp32
wherever the contract stores fp32.  tests/test_fragments_reference.py holds it to
analytic truth; the GPU tests hold the kernels to it."""
import numpy as np

f32 = np.float32
LAMBDA_DEP = 0.968
SOBEL_SCALE = 0.125
ITERATIONS = (20, 10, 5)
B = 16


# ------------------------------------------------------------------ f13 frames
def _tap(a, b, c):
    return (f32(0.25) * a + f32(0.5) * b) + f32(0.25) * c


def gauss3(img):
    p = np.pad(img.astype(f32), ((0, 0), (1, 1)), mode="edge")
    h = _tap(p[:, :-2], p[:, 1:-1], p[:, 2:])
    p = np.pad(h, ((1, 1), (0, 0)), mode="edge")
    return _tap(p[:-2], p[1:-1], p[2:])


def down2(img):
    return (((img[0::2, 0::2] + img[0::2, 1::2]) + img[1::2, 0::2]) + img[1::2, 1::2]) * f32(0.25)


def sobel(img):
    p = np.pad(img, ((0, 0), (1, 1)), mode="edge")
    h = np.pad(p[:, 2:] - p[:, :-2], ((1, 1), (0, 0)), mode="edge")
    dx = (h[:-2] + f32(2) * h[1:-1]) + h[2:]
    p = np.pad(img, ((1, 1), (0, 0)), mode="edge")
    k = np.pad(p[2:] - p[:-2], ((0, 0), (1, 1)), mode="edge")
    dy = (k[:, :-2] + f32(2) * k[:, 1:-1]) + k[:, 2:]
    return dx, dy


def preprocess(intensity, depth, min_depth=0.0, max_depth=4.0):
    """One frame -> its three levels: dicts of I, D, Idx, Idy, Ddx, Ddy (fp32 [H_l, W_l])."""
    with np.errstate(invalid="ignore"):
        d = depth.astype(f32).copy()
        d[(d < f32(min_depth)) | (d > f32(max_depth)) | (d <= 0)] = np.nan
        I, D = gauss3(intensity), gauss3(d)
        out = []
        for l in range(3):
            if l:
                I, D = down2(gauss3(I)), down2(D)
            Idx, Idy = sobel(I)
            Ddx, Ddy = sobel(D)
            out.append(dict(I=I, D=D, Idx=Idx, Idy=Idy, Ddx=Ddx, Ddy=Ddy))
    return out


def level_K(K, l):
    return tuple(float(v) * 0.5 ** l for v in K)


def apply_T(T, X, Y, Z):
    return (((T[0, 0] * X + T[0, 1] * Y) + T[0, 2] * Z) + T[0, 3], ((T[1, 0] * X + T[1, 1] * Y) + T[1, 2] * Z) + T[1, 3],
            ((T[2, 0] * X + T[2, 1] * Y) + T[2, 2] * Z) + T[2, 3])


def correspondences(Ls, Lt, K, T, max_depth_diff):
    """corr int64 [H W]: target pixel -> source pixel or -1, and per source pixel p (x, y, z)."""
    fx, fy, cx, cy = K
    H, W = Ls["D"].shape
    with np.errstate(invalid="ignore", divide="ignore"):
        d = Ls["D"].reshape(-1).astype(np.float64)
        i = np.arange(H * W)
        us, vs = (i % W).astype(np.float64), (i // W).astype(np.float64)
        X, Y = ((us - cx) * d) / fx, ((vs - cy) * d) / fy
        px, py, pz = apply_T(T, X, Y, d)
        ok = np.isfinite(d) & (pz > 0)
        uf, vf = (fx * px) / pz + cx + 0.5, (fy * py) / pz + cy + 0.5
        ok &= (uf > -1.0) & (uf < W) & (vf > -1.0) & (vf < H)
        ut, vt = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)  # truncation
        j = vt * W + ut
        dt = Lt["D"].reshape(-1)[j].astype(np.float64)
        ok &= np.isfinite(dt) & (np.abs(pz - dt) <= max_depth_diff)
    key = (pz[ok].astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | i[ok].astype(np.uint64)
    best = np.full(H * W, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, j[ok], key)
    corr = np.where(best == np.iinfo(np.uint64).max, -1, (best & np.uint64(0xffffffff)).astype(np.int64))
    return corr, (px, py, pz)


def intensity_scales(Ls, Lt, K, T, max_depth_diff):
    corr, _ = correspondences(Ls, Lt, K, T, max_depth_diff)
    j = np.nonzero(corr >= 0)[0]
    if not len(j):
        return 1.0, 1.0
    Is, It = Ls["I"].reshape(-1)[corr[j]].astype(np.float64), Lt["I"].reshape(-1)[j].astype(np.float64)
    return 0.5 / (Is.sum() / len(j)), 0.5 / (It.sum() / len(j))


def rows(Ls, Lt, K, T, max_depth_diff, a_s=1.0, a_t=1.0):
    """Per correspondence (in target pixel order): J_I, J_D [n,6], r_I, r_D [n], and the map."""
    fx, fy, cx, cy = K
    corr, (px, py, pz) = correspondences(Ls, Lt, K, T, max_depth_diff)
    j = np.nonzero(corr >= 0)[0]
    i = corr[j]
    px, py, pz = px[i], py[i], pz[i]
    g = lambda name: np.nan_to_num(Lt[name].reshape(-1)[j].astype(np.float64), nan=0.0)
    si, sd = np.sqrt(1.0 - LAMBDA_DEP), np.sqrt(LAMBDA_DEP)
    sI = SOBEL_SCALE * a_t
    c0, c1 = sI * g("Idx") * fx / pz, sI * g("Idy") * fy / pz
    c2 = -(c0 * px + c1 * py) / pz
    d0, d1 = SOBEL_SCALE * g("Ddx") * fx / pz, SOBEL_SCALE * g("Ddy") * fy / pz
    d2 = -(d0 * px + d1 * py) / pz
    JI = si * np.stack([-pz * c1 + py * c2, pz * c0 - px * c2, -py * c0 + px * c1, c0, c1, c2], 1)
    JD = sd * np.stack([-pz * d1 + py * d2 - py, pz * d0 - px * d2 + px, -py * d0 + px * d1, d0, d1, d2 - 1.0], 1)
    rI = si * (a_t * Lt["I"].reshape(-1)[j].astype(np.float64) - a_s * Ls["I"].reshape(-1)[i].astype(np.float64))
    rD = sd * (Lt["D"].reshape(-1)[j].astype(np.float64) - pz)
    return JI, JD, rI, rD, corr


def linearize(Ls, Lt, K, T, max_depth_diff, a_s=1.0, a_t=1.0):
    """(JtJ [6,6], Jtr [6], count, abs_JtJ, abs_Jtr, corr): the abs_* are the sums of
    the absolute terms, the scale of a summation-order difference."""
    JI, JD, rI, rD, corr = rows(Ls, Lt, K, T, max_depth_diff, a_s, a_t)
    terms = JI[:, :, None] * JI[:, None, :] + JD[:, :, None] * JD[:, None, :]
    rterms = JI * rI[:, None] + JD * rD[:, None]
    return terms.sum(0), rterms.sum(0), len(rI), np.abs(terms).sum(0), np.abs(rterms).sum(0), corr


def exp6(x):
    cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, x[3]],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, x[4]],
                     [-sy, cy * sx, cy * cx, x[5]], [0.0, 0.0, 0.0, 1.0]])


def aff_mul(A, Bm):
    C = np.eye(4)
    for r in range(3):
        for c in range(4):
            s = (A[r, 0] * Bm[0, c] + A[r, 1] * Bm[1, c]) + A[r, 2] * Bm[2, c]
            C[r, c] = s + A[r, 3] if c == 3 else s
    return C


def aff_inv(T):
    I = np.eye(4)
    I[:3, :3] = T[:3, :3].T
    for r in range(3):
        I[r, 3] = -((I[r, 0] * T[0, 3] + I[r, 1] * T[1, 3]) + I[r, 2] * T[2, 3])
    return I


def cholesky_solve(A, b):
    """x with A x = b, or None at a pivot that is not positive and finite."""
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not (d > 0.0) or not np.isfinite(d):
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    z = np.zeros(6)
    for i in range(6):
        z[i] = (b[i] - (L[i, :i] * z[:i]).sum()) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (z[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def information(L0s, L0t, K, T, max_depth_diff):
    fx, fy, cx, cy = K
    H, W = L0s["D"].shape
    corr, _ = correspondences(L0s, L0t, K, T, max_depth_diff)
    j = np.nonzero(corr >= 0)[0]
    if not len(j):
        return np.zeros((6, 6))
    z = L0t["D"].reshape(-1)[j].astype(np.float64)
    x, y = (((j % W) - cx) * z) / fx, (((j // W) - cy) * z) / fy
    n, sx, sy, sz = float(len(j)), x.sum(), y.sum(), z.sum()
    xx, xy, xz, yy, yz, zz = (x * x).sum(), (x * y).sum(), (x * z).sum(), (y * y).sum(), (y * z).sum(), (z * z).sum()
    return np.array([[yy + zz, -xy, -xz, 0.0, -sz, sy], [-xy, xx + zz, -yz, sz, 0.0, -sx],
                     [-xz, -yz, xx + yy, -sy, sx, 0.0], [0.0, sz, -sy, n, 0.0, 0.0], [-sz, 0.0, sx, 0.0, n, 0.0],
                     [sy, -sx, 0.0, 0.0, 0.0, n]])


def odometry_pair(Ps, Pt, K, init=None, max_depth_diff=0.07, iterations=ITERATIONS):
    """Ps, Pt: preprocess() of the source and the target frame.  Returns (trans,
    info, success, n_corr_last, iterations_run)."""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    a_s, a_t = intensity_scales(Ps[0], Pt[0], K, T, max_depth_diff)
    ok, n_last, runs = True, 0, 0
    for k in range(3):
        l = 2 - k
        Kl = level_K(K, l)
        for _ in range(iterations[k]):
            JtJ, Jtr, n_last, _, _, _ = linearize(Ps[l], Pt[l], Kl, T, max_depth_diff, a_s, a_t)
            x = cholesky_solve(JtJ, -Jtr) if n_last > 0 else None
            if x is None:
                ok = False
                break
            T = aff_mul(exp6(x), T)
            runs += 1
        if not ok:
            break
    return T, information(Ps[0], Pt[0], K, T, max_depth_diff), ok, n_last, runs


def rgbd_from_color_and_depth(color, depth16, depth_scale=1000.0, depth_trunc=3.0):
    c = color.astype(f32)
    inten = ((f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1]) + f32(0.114) * c[..., 2]) / f32(255)
    d = depth16.astype(f32) / f32(depth_scale)
    return inten, np.where(d > f32(depth_trunc), f32(0), d)


# ------------------------------------------------------------------ f14
def block_key(c):
    c = np.asarray(c, dtype=np.int64) + (1 << 20)
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


class TsdfError(RuntimeError):
    """The library's PDSC_ERR_UNSUPPORTED of f14: "outside" (a block index) or "full"."""


def _range_check(lo, hi):
    if not (np.all(lo >= -(1 << 20)) and np.all(hi < (1 << 20))):  # also NaN
        raise TsdfError("a block index outside [-2^20, 2^20) (or a non-finite point)")


class Volume:
    """blocks: {(bx, by, bz): [tsdf fp32 [4096], weight fp32 [4096], colour fp32 [4096,3]]}, voxel x + 16 y + 256 z.

    Each rule of the contract is one small method, so that a test can derive a volume with
    one rule broken and show that its assertions tell the two apart.  `stats` counts, over
    all integrate calls, the voxels that went through each branch of the inside test."""

    def __init__(self, voxel_length, sdf_trunc, max_blocks=1 << 19):
        self.vl, self.trunc, self.max_blocks = float(voxel_length), float(sdf_trunc), max_blocks
        self.blocks = {}
        self.stats = dict.fromkeys(("integrated", "u_neg", "v_neg", "u_out", "pz_le0", "sdf_eq_lo", "sdf_eq_hi",
                                    "sdf_gt_hi"), 0)
        self.last_keys = np.zeros((0, 3), np.int64)  # of the last extract(): (block key, voxel index, axis) per point

    # ---- the rules
    def sample_grid(self, H, W):
        return np.arange(0, H, 4), np.arange(0, W, 4)

    def pixel(self, xf):
        return xf.astype(np.int64)  # truncation

    def keep(self, sdf):
        return sdf > -self.trunc

    def integration_set(self, touched):
        return touched

    def negative(self, F):
        return F < 0

    def cube_valid(self, nz):
        """cube[v]: all 8 corners v + {0,1}^3 have weight != 0 (on the dense grid; absent blocks are 0)."""
        n = nz.shape
        cube = np.zeros(n, bool)
        cube[:-1, :-1, :-1] = True
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    cube[:-1, :-1, :-1] &= nz[dx:n[0] - 1 + dx, dy:n[1] - 1 + dy, dz:n[2] - 1 + dz]
        return cube

    def edge_alive(self, cube, o1, o2):
        """any of the four cubes around the edge (v, a): v - {0,1} e_o1 - {0,1} e_o2"""
        return cube | np.roll(cube, 1, o1) | np.roll(cube, 1, o2) | np.roll(np.roll(cube, 1, o1), 1, o2)

    def block_rank(self, blk):
        return block_key(blk)

    # ---- f14
    def _zeros(self):
        return [np.zeros(B ** 3, f32), np.zeros(B ** 3, f32), np.zeros((B ** 3, 3), f32)]

    def touched(self, depth, K, extrinsic):
        fx, fy, cx, cy = K
        Ei = aff_inv(np.asarray(extrinsic, dtype=np.float64))
        vs, us = self.sample_grid(*depth.shape)
        v, u = np.meshgrid(vs, us, indexing="ij")
        d = depth[v, u].astype(np.float64)
        with np.errstate(invalid="ignore"):
            m = d > 0
        u, v, d = u[m].astype(np.float64), v[m].astype(np.float64), d[m]
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.stack(apply_T(Ei, ((u - cx) * d) / fx, ((v - cy) * d) / fy, d), 1)
            edge = self.vl * B
            lo, hi = np.floor((p - self.trunc) / edge), np.floor((p + self.trunc) / edge)
        _range_check(lo, hi)
        out = set()
        for a, b in zip(lo.astype(np.int64), hi.astype(np.int64)):
            for bx in range(a[0], b[0] + 1):
                for by in range(a[1], b[1] + 1):
                    for bz in range(a[2], b[2] + 1):
                        out.add((bx, by, bz))
        return out

    def integrate(self, depth, colour, K, extrinsic, slotted=None):
        """False when the frame needs more than max_blocks blocks: no voxel changes, and as
        many of the frame's new blocks as there are free slots come into being at weight 0 --
        on the GPU whichever win the race (`slotted`: those, as read back), here the lowest
        keys.  TsdfError, and no change at all, at a block index out of range."""
        fx, fy, cx, cy = K
        E = np.asarray(extrinsic, dtype=np.float64)
        H, W = depth.shape
        touched = self.touched(depth, K, E)
        new = touched - set(self.blocks)
        if len(self.blocks) + len(new) > self.max_blocks:
            room = self.max_blocks - len(self.blocks)
            take = sorted(new, key=lambda c: int(block_key(c)))[:room] if slotted is None else [tuple(k) for k in slotted]
            assert set(take) <= new and len(set(take)) == room, "the slotted blocks are not the frame's"
            for key in take:
                self.blocks[key] = self._zeros()
            return False
        for key in new:
            self.blocks[key] = self._zeros()
        vi = np.arange(B ** 3)
        off = np.stack([vi & 15, (vi >> 4) & 15, vi >> 8], 1)
        st = self.stats
        for key in self.integration_set(touched):
            blk = self.blocks[key]
            w = ((np.array(key) * B + off).astype(np.float64) + 0.5) * self.vl
            px, py, pz = apply_T(E, w[:, 0], w[:, 1], w[:, 2])
            with np.errstate(invalid="ignore", divide="ignore"):
                uf, vf = (fx * px) / pz + cx + 0.5, (fy * py) / pz + cy + 0.5
                front = pz > 0
                ok = front & (uf > -1.0) & (uf < W) & (vf > -1.0) & (vf < H)
                st["pz_le0"] += int((~front).sum())
                st["u_out"] += int((front & ((uf <= -1.0) | (uf >= W))).sum())
                u, v = self.pixel(np.where(ok, uf, 0)), self.pixel(np.where(ok, vf, 0))
                d = depth[v, u]
                ok &= d > 0
                rx, ry = (u - cx) / fx, (v - cy) / fy
                sdf = (d.astype(np.float64) - pz) * np.sqrt((rx * rx + ry * ry) + 1.0)
                st["sdf_eq_lo"] += int((ok & (sdf == -self.trunc)).sum())
                ok &= self.keep(sdf)
                tn = np.minimum(1.0, sdf / self.trunc).astype(f32)
            st["integrated"] += int(ok.sum())
            st["u_neg"] += int((ok & (uf < 0)).sum())
            st["v_neg"] += int((ok & (vf < 0)).sum())
            st["sdf_eq_hi"] += int((ok & (sdf == self.trunc)).sum())
            st["sdf_gt_hi"] += int((ok & (sdf > self.trunc)).sum())
            t, wt, col = blk
            w1 = wt + f32(1)
            with np.errstate(invalid="ignore"):
                t[ok] = ((t * wt + tn) / w1)[ok]
                col[ok] = ((col * wt[:, None] + colour[v, u].astype(f32)) / w1[:, None])[ok]
            wt[ok] = w1[ok]
        return True

    def write_blocks(self, coords, tsdf, weight, colour):
        """pdsc_tsdf_write_blocks: TsdfError "outside" with no change at all; "full" with no
        voxel written, the free slots filled from the new blocks (here: in the given order)."""
        coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
        _range_check(coords, coords)
        keys = [tuple(int(x) for x in c) for c in coords]
        new = [k for k in dict.fromkeys(keys) if k not in self.blocks]
        if len(self.blocks) + len(new) > self.max_blocks:
            for k in new[:self.max_blocks - len(self.blocks)]:
                self.blocks[k] = self._zeros()
            raise TsdfError(f"the volume is full: more than max_blocks={self.max_blocks} blocks")
        for i, k in enumerate(keys):
            self.blocks[k] = [np.array(tsdf[i], f32), np.array(weight[i], f32), np.array(colour[i], f32).reshape(-1, 3)]

    def sorted_blocks(self):
        keys = sorted(self.blocks, key=lambda c: int(block_key(c)))
        if not keys:
            return (np.zeros((0, 3), np.int32), np.zeros((0, B ** 3), f32), np.zeros((0, B ** 3), f32),
                    np.zeros((0, B ** 3, 3), f32))
        return (np.array(keys, dtype=np.int32).reshape(-1, 3), np.stack([self.blocks[k][0] for k in keys]),
                np.stack([self.blocks[k][1] for k in keys]), np.stack([self.blocks[k][2] for k in keys]))

    def extract(self):
        """(points [n,3], colours [n,3], fsum [n] = |f0| + |f1|) in (block key, voxel
        index, axis) order, straight from the definition on a dense grid: an edge is
        emitted iff its ends differ in sign and one of its four cubes is valid.  The grid
        is the bounding box of each 26-connected group of blocks (a cube never spans two
        groups), so far-apart blocks cost nothing."""
        self.last_keys = np.zeros((0, 3), np.int64)
        recs = []
        for group in self._groups():
            recs += self._extract_group(group)
        if not recs:
            return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0)
        ok = np.concatenate([r[0] for r in recs])
        rank = np.concatenate([r[4] for r in recs])
        order = np.lexsort((ok[:, 2], ok[:, 1], rank))
        self.last_keys = ok[order]
        return (np.concatenate([r[1] for r in recs])[order], np.concatenate([r[2] for r in recs])[order],
                np.concatenate([r[3] for r in recs])[order])

    def _groups(self):
        left, groups = set(self.blocks), []
        while left:
            stack, group = [left.pop()], []
            while stack:
                k = stack.pop()
                group.append(k)
                for dx in (-1, 0, 1):
                    for dy in (-1, 0, 1):
                        for dz in (-1, 0, 1):
                            q = (k[0] + dx, k[1] + dy, k[2] + dz)
                            if q in left:
                                left.remove(q)
                                stack.append(q)
            groups.append(group)
        return groups

    def _extract_group(self, group):
        keys = np.array(group, dtype=np.int64)
        lo = keys.min(0) - 1
        n = (keys.max(0) - lo + 2) * B
        F, Wt, C = np.zeros(n, f32), np.zeros(n, f32), np.zeros(tuple(n) + (3,), f32)
        for k in group:
            t, w, c = self.blocks[k]
            o = (np.array(k) - lo) * B
            sl = tuple(slice(o[a], o[a] + B) for a in range(3))
            F[sl] = t.reshape(B, B, B).transpose(2, 1, 0)  # [x, y, z] from index x + 16 y + 256 z
            Wt[sl] = w.reshape(B, B, B).transpose(2, 1, 0)
            C[sl] = c.reshape(B, B, B, 3).transpose(2, 1, 0, 3)
        cube = self.cube_valid(Wt != 0)
        neg = self.negative(F)
        recs = []
        for a in range(3):
            o1, o2 = [x for x in range(3) if x != a]
            near = self.edge_alive(cube, o1, o2)
            sign = neg != np.roll(neg, -1, a)
            idx = np.argwhere(sign & near)
            if not len(idx):
                continue
            nb = idx.copy()
            nb[:, a] += 1
            f0 = np.abs(F[tuple(idx.T)].astype(np.float64))
            f1 = np.abs(F[tuple(nb.T)].astype(np.float64))
            g = idx + lo * B
            p = (g.astype(np.float64) + 0.5) * self.vl
            p[:, a] += f0 * self.vl / (f0 + f1)
            col = (f1[:, None] * C[tuple(idx.T)].astype(np.float64) + f0[:, None] * C[tuple(nb.T)].astype(np.float64)) \
                / (f0 + f1)[:, None] / 255.0
            blk, v = g // B, g % B
            order_key = np.stack([block_key(blk), v[:, 0] + 16 * v[:, 1] + 256 * v[:, 2], np.full(len(g), a)], 1)
            recs.append((order_key, p, col, f0 + f1, np.asarray(self.block_rank(blk))))
        return recs


# ------------------------------------------------------------------ scenes
def texture(p):
    """A smooth analytic texture in [0.2, 0.8] of a world point (vectorised)."""
    return 0.5 + 0.1 * (np.sin(5.0 * p[..., 0] + 1.0) + np.sin(6.0 * p[..., 1] + 2.0 * p[..., 2]) +
                        np.sin(4.0 * p[..., 2] - 3.0 * p[..., 0] + 0.5))


# three planes n . p = d (a back wall, a floor, a side wall), seen from near the origin looking along +z
PLANES = [(np.array([0.1, 0.05, 1.0]) / np.linalg.norm([0.1, 0.05, 1.0]), 2.0),
          (np.array([0.0, 1.0, 0.15]) / np.linalg.norm([0.0, 1.0, 0.15]), 0.9),
          (np.array([1.0, 0.0, 0.2]) / np.linalg.norm([1.0, 0.0, 0.2]), 1.2)]


def render(pose, K, H, W, planes=PLANES):
    """The scene from camera `pose` (camera -> world): (intensity fp32 [H,W], depth
    fp32 [H,W] metres, colour uint8 [H,W,3]) by ray casting, exact per pixel."""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    R, t = pose[:3, :3], pose[:3, 3]
    rw = ray @ R.T
    best = np.full((H, W), np.inf)
    for nrm, d in planes:
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (d - nrm @ t) / (rw @ nrm)
        s = np.where(s > 0, s, np.inf)
        best = np.minimum(best, s)
    depth = np.where(np.isfinite(best), best, 0.0)
    pw = t + rw * depth[..., None]
    inten = texture(pw)
    colour = np.stack([inten, 0.5 * inten + 0.25, 1.0 - inten], -1)
    return inten.astype(f32), depth.astype(f32), np.clip(np.round(colour * 255.0), 0, 255).astype(np.uint8)


def small_motion(rx=0.004, ry=-0.012, rz=0.006, t=(0.015, -0.008, 0.01)):
    """About 1 degree and 2 cm."""
    return exp6(np.array([rx, ry, rz, *t]))


def pose_errors(T, T_true):
    """(rotation error in radians, translation error in metres) of T against T_true."""
    D = T @ np.linalg.inv(T_true)
    return float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(D[:3, 3]))
