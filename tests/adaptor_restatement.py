"""Independent numpy restatement of the measurement adaptors (DESIGN.md section 4 "Measurement adaptors").

Depth image -> 3-D points + normals and laser scan -> 2-D points + normals, in float32 in the documented operation order
(bearings and their sine / cosine in float64, with the polynomial of csrc/det_math.h restated with + - * only), so the
library must give the same bits.  Every function works on whole arrays; nothing here knows the library.
"""
import numpy as np

F = np.float32
IMAGE_NONE, IMAGE_U8, IMAGE_U16, IMAGE_F32 = 0, 1, 2, 3


def _depth_z(depth, depth_scale):
    """(z as float32, readable): U16 counts * scale with 0 = no reading, F32 metres as they are"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(F) * F(depth_scale), depth != 0
    if depth.dtype != np.float32:
        raise ValueError("depth image: uint16 or float32, got %s" % depth.dtype)
    return depth, np.ones(depth.shape, bool)


def _unproject(z, K):
    rows, cols = z.shape
    K = np.asarray(K, F).reshape(3, 3)
    ifx, ify = F(1.0) / K[0, 0], F(1.0) / K[1, 1]
    c = np.arange(cols, dtype=F)[None, :]
    r = np.arange(rows, dtype=F)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((c - K[0, 2]) * ifx) * z
        y = ((r - K[1, 2]) * ify) * z
    return np.stack([x, y, z], -1).astype(F)


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def adapt_depth_image(depth, K, depth_scale=0.001, depth_min=0.4, depth_max=8.0, col_gap=1, row_gap=1,
                      max_distance_squared=0.0625, drop_points_without_normal=True, compact=False, intensity=None):
    """dict(points (n, 3), normals (n, 3) or None, intensity (n,) or None, global_indices (compact) or None, depth_valid,
    has_normal, valid (rows*cols masks), num_raw, num_in_range, num_valid).  Organised: n = rows*cols, invalid = NaN."""
    z, readable = _depth_z(depth, depth_scale)
    rows, cols = z.shape
    n = rows * cols
    with np.errstate(invalid="ignore"):
        dvalid = readable & np.isfinite(z) & (F(depth_min) <= z) & (z <= F(depth_max))
    P = _unproject(z, K)
    want_normals = col_gap > 0
    N = np.full((rows, cols, 3), np.nan, F)
    has_n = np.zeros((rows, cols), bool)
    gc, gr = int(col_gap), int(row_gap)
    if want_normals and cols > 2 * gc and rows > 2 * gr:
        ctr = (slice(gr, rows - gr), slice(gc, cols - gc))
        lf, rt = (ctr[0], slice(0, cols - 2 * gc)), (ctr[0], slice(2 * gc, cols))
        up, dn = (slice(0, rows - 2 * gr), ctr[1]), (slice(2 * gr, rows), ctr[1])
        ok = dvalid[ctr] & dvalid[lf] & dvalid[rt] & dvalid[up] & dvalid[dn]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            dc = P[rt] - P[lf]
            dr = P[dn] - P[up]
            ok &= ~(_sq(dc) > F(max_distance_squared)) & ~(_sq(dr) > F(max_distance_squared))
            nx = dc[..., 1] * dr[..., 2] - dc[..., 2] * dr[..., 1]
            ny = dc[..., 2] * dr[..., 0] - dc[..., 0] * dr[..., 2]
            nz = dc[..., 0] * dr[..., 1] - dc[..., 1] * dr[..., 0]
            nn = np.stack([nx, ny, nz], -1)
            ln = np.sqrt(_sq(nn))
            ok &= ln > 0
            nn = nn / ln[..., None]
            q = P[ctr]
            flip = (nn[..., 0] * q[..., 0] + nn[..., 1] * q[..., 1]) + nn[..., 2] * q[..., 2] > 0
            nn = np.where(flip[..., None], -nn, nn)
        Nc = N[ctr]
        Nc[ok] = nn[ok]
        N[ctr] = Nc
        has_n[ctr] = ok
    valid = dvalid & (has_n | (not drop_points_without_normal)) if want_normals else dvalid.copy()
    pts = np.where(valid[..., None], P, F(np.nan)).astype(F).reshape(n, 3)
    nrm = N.reshape(n, 3) if want_normals else None
    it = None if intensity is None else np.asarray(intensity).astype(F).reshape(n)
    vflat = valid.reshape(n)
    out = {"depth_valid": dvalid.reshape(n), "has_normal": has_n.reshape(n), "valid": vflat, "num_raw": n,
           "num_in_range": int(dvalid.sum()), "num_valid": int(vflat.sum()), "global_indices": None}
    if compact:
        g = np.flatnonzero(vflat).astype(np.int32)
        pts, nrm, it = pts[g], (None if nrm is None else nrm[g]), (None if it is None else it[g])
        out["global_indices"] = g
    out.update(points=pts, normals=nrm, intensity=it)
    return out


# ---- sine / cosine of csrc/det_math.h: fixed argument reduction + polynomial kernels, float64, + - * only -----------------
_INV_PIO2 = 6.36619772367581382433e-01
_PIO2_HI = 1.57079632673412561417e+00
_PIO2_LO = 6.07710050650619224932e-11
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06,
      -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07,
      2.08757232129817482790e-09, -1.13596475577881948265e-11)


def sincos(x):
    x = np.asarray(x, np.float64)
    kx = x * _INV_PIO2
    k = np.trunc(kx + np.where(kx >= 0.0, 0.5, -0.5)).astype(np.int64)
    kd = k.astype(np.float64)
    r = (x - kd * _PIO2_HI) - kd * _PIO2_LO
    z = r * r
    ps = _S[0] + z * (_S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5]))))
    sn = r + (r * z) * ps
    pc = _C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5]))))
    cs = (1.0 - 0.5 * z) + (z * z) * pc
    q = k & 3
    s = np.choose(q, [sn, cs, -sn, -cs])
    c = np.choose(q, [cs, -sn, -cs, sn])
    return s, c


def adapt_laser_scan(ranges, angle_min, angle_increment, range_min=0.05, range_max=30.0, half_window=1,
                     max_distance_squared=0.01, drop_points_without_normal=True, compact=False):
    """as adapt_depth_image, for a scan: points / normals (n, 2); global indices = beam indices"""
    r = np.asarray(ranges, F).reshape(-1)
    n = r.shape[0]
    w = int(half_window)
    bearing = np.float64(angle_min) + np.arange(n, dtype=np.float64) * np.float64(angle_increment)
    s, c = sincos(bearing)
    cf, sf = c.astype(F), s.astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        rvalid = np.isfinite(r) & (F(range_min) <= r) & (r <= F(range_max))
        P = np.stack([cf * r, sf * r], -1).astype(F)
    N = np.full((n, 2), np.nan, F)
    has_n = np.zeros(n, bool)
    if w > 0 and n > 2 * w:
        ctr, a, b = slice(w, n - w), slice(0, n - 2 * w), slice(2 * w, n)
        ok = rvalid[ctr] & rvalid[a] & rvalid[b]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = P[b] - P[a]
            t2 = t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]
            ok &= t2 <= F(max_distance_squared)
            ln = np.sqrt(t2)
            ok &= ln > 0
            nn = np.stack([t[:, 1] / ln, -t[:, 0] / ln], -1)
            q = P[ctr]
            flip = nn[:, 0] * q[:, 0] + nn[:, 1] * q[:, 1] > 0
            nn = np.where(flip[:, None], -nn, nn)
        Nc = N[ctr]
        Nc[ok] = nn[ok]
        N[ctr] = Nc
        has_n[ctr] = ok
    valid = rvalid & (has_n | (not drop_points_without_normal)) if w > 0 else rvalid.copy()
    pts = np.where(valid[:, None], P, F(np.nan)).astype(F)
    nrm = N if w > 0 else None
    out = {"depth_valid": rvalid, "has_normal": has_n, "valid": valid, "num_raw": n, "num_in_range": int(rvalid.sum()),
           "num_valid": int(valid.sum()), "global_indices": None, "intensity": None}
    if compact:
        g = np.flatnonzero(valid).astype(np.int32)
        pts, nrm = pts[g], (None if nrm is None else nrm[g])
        out["global_indices"] = g
    out.update(points=pts, normals=nrm)
    return out


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN == NaN whatever the payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
