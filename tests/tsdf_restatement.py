"""Independent numpy restatement of the TSDF volume (DESIGN.md section 4 "TSDF volume").

A frame's float work in float32 in the documented operation order (whole arrays with float32 scalars: numpy rounds every
operation once, as the device does without contraction), the adds to the planes in integers; the raycast's march, the trilinear
sample and the export likewise.  ``integrate_loop`` is the contract once more as a plain per-frame, per-voxel loop over scalars:
tests/test_tsdf_restatement.py checks the vectorised form against it.  The library must give the same bits.  Nothing here knows
the library.
"""
import numpy as np

from clip_projective_restatement import se3_inverse, xform

F = np.float32
MAX_SIDE, MASK_SIDE, MAX_MARCH = 2048, 8, 2 ** 20


def volume(nx, ny, nz, voxel_size=0.02, origin=(0.0, 0.0, 0.0), with_intensity=False):
    return {"nx": int(nx), "ny": int(ny), "nz": int(nz), "vs": F(voxel_size), "o": np.asarray(origin, F).reshape(3),
            "with_intensity": bool(with_intensity)}


def camera(K, rows, cols, depth_scale=0.001, depth_min=0.4, depth_max=8.0):
    return {"K": np.asarray(K, F).reshape(3, 3), "rows": int(rows), "cols": int(cols), "scale": F(depth_scale), "dmin": F(depth_min),
            "dmax": F(depth_max)}


def new_planes(v):
    shape = (v["nz"], v["ny"], v["nx"])
    return [np.zeros(shape, np.int32) for _ in range(3 if v["with_intensity"] else 2)]


def centres(v):
    """(n, 3) float32: the centre of every voxel in plane-index order, origin + ((float) i + 0.5f) * voxel_size per axis"""
    ax = [v["o"][a] + (np.arange(n, dtype=F) + F(0.5)) * v["vs"] for a, n in enumerate((v["nx"], v["ny"], v["nz"]))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(F)


def depth_metres(depth, cam):
    """(d as float32, passes the gate): U16 counts * scale with 0 = no reading, F32 metres as they are"""
    depth = np.asarray(depth)
    with np.errstate(invalid="ignore", over="ignore"):
        if depth.dtype == np.uint16:
            d, read = depth.astype(F) * cam["scale"], depth != 0
        else:
            assert depth.dtype == np.float32
            d, read = depth, np.ones(depth.shape, bool)
        return d, read & np.isfinite(d) & (d >= cam["dmin"]) & (d <= cam["dmax"])


def intensity_value(inten):
    """U8 as it is; F32 as floorf(x + 0.5f) clamped to 0 .. 255, NaN = 0"""
    inten = np.asarray(inten)
    if inten.dtype == np.uint8:
        return inten.astype(np.int64)
    assert inten.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.floor(inten + F(0.5))
        return np.where(r >= F(255), 255, np.where(r > F(0), r, 0)).astype(np.int64)


def frame_update(v, cam, depth, pose, mu, intensity=None):
    """one frame: (voxel plane indices that receive an add, their q, their I or None)"""
    P = centres(v)
    W = se3_inverse(pose)
    K, rows, cols, mu = cam["K"], cam["rows"], cam["cols"], F(mu)
    d_img, ok_img = depth_metres(depth, cam)
    with np.errstate(all="ignore"):
        c = xform(W, P)
        cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
        uf = ((K[0, 0] * cx) / cz + K[0, 2]) + F(0.5)
        vf = ((K[1, 1] * cy) / cz + K[1, 2]) + F(0.5)
        seen = (cz > F(0)) & (uf >= F(0)) & (uf < F(cols)) & (vf >= F(0)) & (vf < F(rows))
        idx = np.flatnonzero(seen)
        pr, pc = np.floor(vf[idx]).astype(np.int64), np.floor(uf[idx]).astype(np.int64)
        good = ok_img[pr, pc]
        idx, pr, pc = idx[good], pr[good], pc[good]
        s = d_img[pr, pc] - cz[idx]
        near = ~(s < -mu)
        idx, pr, pc, s = idx[near], pr[near], pc[near], s[near]
        t = np.minimum(s, mu)
        q = np.floor((t / mu) * F(32767.0) + F(0.5)).astype(np.int64)
    inten = None if intensity is None else intensity_value(intensity)[pr, pc]
    return idx, q, inten


def integrate(planes, v, cam, depths, poses, mu, intensities=None, weight=1):
    """adds the batch to the planes in place; returns the counters of srrg2_tsdf_result"""
    assert weight in (1, -1) and (intensities is not None) == v["with_intensity"]
    poses = np.asarray(poses, F).reshape(-1, 3, 4)
    K = poses.shape[0]
    out = {"num_frames": K, "num_pixels": K * cam["rows"] * cam["cols"], "num_valid_depth": 0, "num_voxel_updates": 0}
    if K * cam["rows"] * cam["cols"] == 0:
        return out
    flat = [p.reshape(-1) for p in planes]
    for k in range(K):
        out["num_valid_depth"] += int(depth_metres(depths[k], cam)[1].sum())
        if flat[0].size == 0:
            continue
        idx, q, inten = frame_update(v, cam, depths[k], poses[k], mu, None if intensities is None else intensities[k])
        flat[0][idx] += (weight * q).astype(np.int32)  # (a frame names a voxel at most once)
        flat[1][idx] += np.int32(weight)
        if inten is not None:
            flat[2][idx] += (weight * inten).astype(np.int32)
        out["num_voxel_updates"] += int(idx.size)
    return out


def integrate_loop(planes, v, cam, depths, poses, mu, intensities=None, weight=1):
    """the contract as a plain loop over frames and voxels with float32 scalars; returns num_voxel_updates"""
    K, mu, updates = cam["K"], F(mu), 0
    for k, pose in enumerate(np.asarray(poses, F).reshape(-1, 3, 4)):
        W = se3_inverse(pose)
        for iz in range(v["nz"]):
            for iy in range(v["ny"]):
                for ix in range(v["nx"]):
                    with np.errstate(all="ignore"):
                        p = [v["o"][a] + (F(i) + F(0.5)) * v["vs"] for a, i in enumerate((ix, iy, iz))]
                        c = [((W[r, 0] * p[0] + W[r, 1] * p[1]) + W[r, 2] * p[2]) + W[r, 3] for r in range(3)]
                        if not c[2] > 0:
                            continue
                        uf = ((K[0, 0] * c[0]) / c[2] + K[0, 2]) + F(0.5)
                        vf = ((K[1, 1] * c[1]) / c[2] + K[1, 2]) + F(0.5)
                        if not (uf >= 0 and uf < F(cam["cols"]) and vf >= 0 and vf < F(cam["rows"])):
                            continue
                        r_, c_ = int(np.floor(vf)), int(np.floor(uf))
                        raw = depths[k][r_, c_]
                        if depths[k].dtype == np.uint16:
                            if raw == 0:
                                continue
                            d = F(raw) * cam["scale"]
                        else:
                            d = F(raw)
                        if not (np.isfinite(d) and cam["dmin"] <= d <= cam["dmax"]):
                            continue
                        s = F(d - c[2])
                        if s < -mu:
                            continue
                        q = int(np.floor(F(F(min(s, mu) / mu) * F(32767.0)) + F(0.5)))
                    planes[0][iz, iy, ix] += weight * q
                    planes[1][iz, iy, ix] += weight
                    if intensities is not None:
                        planes[2][iz, iy, ix] += weight * int(intensity_value(intensities[k][r_:r_ + 1, c_:c_ + 1])[0, 0])
                    updates += 1
    return updates


# ---- raycast -------------------------------------------------------------------------------------------------------------------

def block_mask(weight, min_weight):
    """per 8 x 8 x 8 block: does it hold a voxel with weight >= min_weight"""
    nz, ny, nx = weight.shape
    m = np.zeros(tuple(-(-n // MASK_SIDE) for n in (nz, ny, nx)), bool)
    z, y, x = np.nonzero(weight >= min_weight)
    m[z // MASK_SIDE, y // MASK_SIDE, x // MASK_SIDE] = True
    return m


def sample(planes, v, min_weight, Pw, mask=None):
    """trilinear samples at the world points Pw (n, 3): (F as float32, valid)"""
    sums, weights = planes[0], planes[1]
    n = Pw.shape[0]
    side = (v["nx"], v["ny"], v["nz"])
    with np.errstate(all="ignore"):
        g = [(Pw[:, a] - v["o"][a]) / v["vs"] - F(0.5) for a in range(3)]
        b = [np.floor(x) for x in g]
        ok = np.ones(n, bool)
        for a in range(3):
            ok &= (b[a] >= F(0)) & (b[a] <= F(side[a] - 2))
        idx = np.flatnonzero(ok)
        ix, iy, iz = (b[a][idx].astype(np.int64) for a in range(3))
        if mask is not None:
            keep = mask[iz // MASK_SIDE, iy // MASK_SIDE, ix // MASK_SIDE]
            idx, ix, iy, iz = idx[keep], ix[keep], iy[keep], iz[keep]
        f, good = [], np.ones(idx.size, bool)
        for cnr in range(8):
            x, y, z = ix + (cnr & 1), iy + ((cnr >> 1) & 1), iz + (cnr >> 2)
            w = weights[z, y, x]
            good &= w >= min_weight
            f.append(sums[z, y, x].astype(F) / w.astype(F))
        t = [(g[a] - b[a])[idx] for a in range(3)]
        c00, c10 = f[0] + t[0] * (f[1] - f[0]), f[2] + t[0] * (f[3] - f[2])
        c01, c11 = f[4] + t[0] * (f[5] - f[4]), f[6] + t[0] * (f[7] - f[6])
        c0, c1 = c00 + t[1] * (c10 - c00), c01 + t[1] * (c11 - c01)
        val = c0 + t[2] * (c1 - c0)
    Fv, valid = np.zeros(n, F), np.zeros(n, bool)
    Fv[idx[good]], valid[idx[good]] = val[good].astype(F), True
    return Fv, valid


def march_last(cam, step):
    """the largest sample index, float32 as the library counts it (-1: no sample; None: refused)"""
    with np.errstate(all="ignore"):
        span = np.floor((cam["dmax"] - cam["dmin"]) / F(step))
    if not span <= F(MAX_MARCH):
        return None
    return int(span) if span >= 0 else -1


def raycast(planes, v, cam, pose, step, min_weight=1, skip_empty=False):
    """(depth (rows, cols) float32, intensity (rows, cols) uint8 or None)"""
    rows, cols, K, step = cam["rows"], cam["cols"], cam["K"], F(step)
    T = np.asarray(pose, F).reshape(3, 4)
    n = rows * cols
    last = march_last(cam, step)
    mask = block_mask(planes[1], min_weight) if skip_empty and planes[1].size else None
    with np.errstate(all="ignore"):
        cc, rr = np.meshgrid(np.arange(cols, dtype=F), np.arange(rows, dtype=F))
        xn, yn = ((cc - K[0, 2]) / K[0, 0]).reshape(-1), ((rr - K[1, 2]) / K[1, 1]).reshape(-1)
        depth = np.zeros(n, F)
        found = np.zeros(n, bool)
        Fp, vp, zp = np.zeros(n, F), np.zeros(n, bool), np.zeros(n, F)
        for i in range(last + 1):
            live = np.flatnonzero(~found)
            if live.size == 0:
                break
            z = cam["dmin"] + F(i) * step
            Pc = np.stack([xn[live] * z, yn[live] * z, np.full(live.size, z, F)], 1).astype(F)
            Fc, vc = sample(planes, v, min_weight, xform(T, Pc), mask)
            hit = vp[live] & vc & (Fp[live] > F(0)) & (Fc <= F(0))
            h = live[hit]
            depth[h] = zp[h] + (step * Fp[h]) / (Fp[h] - Fc[hit])
            found[h] = True
            Fp[live], vp[live], zp[live] = Fc, vc, z
        ok = found & (depth >= cam["dmin"]) & (depth <= cam["dmax"])
        depth = np.where(ok, depth, F(0)).astype(F)
        inten = None
        if v["with_intensity"]:
            inten = np.zeros(n, np.uint8)
            h = np.flatnonzero(ok)
            Pc = np.stack([xn[h] * depth[h], yn[h] * depth[h], depth[h]], 1).astype(F)
            Pw = xform(T, Pc)
            b = [np.floor((Pw[:, a] - v["o"][a]) / v["vs"]) for a in range(3)]
            inside = np.ones(h.size, bool)
            for a, side in enumerate((v["nx"], v["ny"], v["nz"])):
                inside &= (b[a] >= F(0)) & (b[a] <= F(side - 1))
            h = h[inside]
            ix, iy, iz = (b[a][inside].astype(np.int64) for a in range(3))
            w, s = planes[1][iz, iy, ix].astype(np.int64), planes[2][iz, iy, ix].astype(np.int64)
            mean = np.where(w >= 1, (s + w // 2) // np.maximum(w, 1), 0)
            inten[h] = np.clip(mean, 0, 255).astype(np.uint8)
            inten = inten.reshape(rows, cols)
    return depth.reshape(rows, cols), inten


# ---- export --------------------------------------------------------------------------------------------------------------------

def to_scene(planes, v, min_weight=1):
    """(points (k, 3) float32, normals (k, 3) float32 with NaN rows, global indices (k,) int32) in (voxel, axis) order"""
    sums, weights = planes[0], planes[1]
    nz, ny, nx = weights.shape
    valid = weights >= min_weight
    with np.errstate(all="ignore"):
        Fv = sums.astype(F) / weights.astype(F)
        grad, whole = [], np.ones(weights.shape, bool)
        for axis in (2, 1, 0):  # x, y, z as array axes
            lo, hi = np.roll(Fv, 1, axis), np.roll(Fv, -1, axis)
            vlo, vhi = np.roll(valid, 1, axis), np.roll(valid, -1, axis)
            i = np.arange(weights.shape[axis]).reshape([-1 if a == axis else 1 for a in range(3)])
            whole &= (i >= 1) & (i + 1 < weights.shape[axis]) & vlo & vhi
            grad.append(hi - lo)
        length = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2])
        ok = whole & (length > F(0))
        normal = np.stack([np.where(ok, g / length, F(np.nan)) for g in grad], -1).astype(F)
        flags = np.zeros((nz, ny, nx, 3), bool)
        tpar = np.zeros((nz, ny, nx, 3), F)
        for a, axis in enumerate((2, 1, 0)):
            F1, v1 = np.roll(Fv, -1, axis), np.roll(valid, -1, axis)
            i = np.arange(weights.shape[axis]).reshape([-1 if b == axis else 1 for b in range(3)])
            cross = ((Fv < 0) & (F1 > 0)) | ((Fv > 0) & (F1 < 0)) | ((Fv == 0) != (F1 == 0))
            flags[..., a] = valid & v1 & (i + 1 < weights.shape[axis]) & cross
            tpar[..., a] = Fv / (Fv - F1)
        e = np.flatnonzero(flags.reshape(-1))
        vox, a = e // 3, e % 3
        ix, iy, iz = vox % max(nx, 1), (vox // max(nx, 1)) % max(ny, 1), vox // max(nx * ny, 1)
        idx = [ix, iy, iz]
        pts = np.zeros((e.size, 3), F)
        t = tpar.reshape(-1)[e]
        for b in range(3):
            mid = v["o"][b] + (idx[b].astype(F) + F(0.5)) * v["vs"]
            moved = v["o"][b] + ((idx[b].astype(F) + F(0.5)) + t) * v["vs"]
            pts[:, b] = np.where(a == b, moved, mid)
    return pts, normal.reshape(-1, 3)[vox], e.astype(np.int32)


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN == NaN whatever the payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
