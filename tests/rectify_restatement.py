"""numpy restatement of the rectification contract (DESIGN.md section 4 "Rectification"; include/srrg2_slam_amd.h): the map of
a camera and a target, the remap of U8 / U16 / F32 images through it, and the rotations of a stereo calibration.  The library
(csrc/rectify.hip) must give the same bits.  float64 with + - * / floor (sqrt in stereo_rectify) in exactly the written order;
numpy evaluates every operator on its own, nothing is fused.  Nothing here knows the library.
"""
import numpy as np

INVALID = np.iinfo(np.int32).min
QUIET_NAN = np.uint32(0x7fc00000)
F64 = np.float64


def _k4(K):
    K = np.asarray(K, F64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def identity_rotation():
    return np.eye(3, dtype=F64)


def build_map(K, distortion, rotation, new_K, src_shape, dst_shape):
    """(uv, info): uv (dst_rows, dst_cols, 2) int32, entries (U, V) in 1/256 source pixel or INVALID twice; info: num_pixels,
    num_valid, first / last row and column holding a valid entry (-1 without one)"""
    fx, fy, cx, cy = _k4(K)
    nfx, nfy, ncx, ncy = _k4(new_K)
    k1, k2, p1, p2, k3, k4, k5, k6 = (F64(v) for v in np.asarray(distortion, F64).reshape(8))
    R = np.asarray(identity_rotation() if rotation is None else rotation, F64).reshape(3, 3)
    src_rows, src_cols = src_shape
    rows, cols = dst_shape
    c, r = np.meshgrid(np.arange(cols, dtype=F64), np.arange(rows, dtype=F64))
    with np.errstate(all="ignore"):
        x = (c - ncx) / nfx
        y = (r - ncy) / nfy
        X = (R[0, 0] * x + R[1, 0] * y) + R[2, 0]
        Y = (R[0, 1] * x + R[1, 1] * y) + R[2, 1]
        W = (R[0, 2] * x + R[1, 2] * y) + R[2, 2]
        xn = X / W
        yn = Y / W
        r2 = xn * xn + yn * yn
        num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
        rad = num / den
        xy = xn * yn
        xd = xn * rad + ((2.0 * p1) * xy + p2 * (r2 + 2.0 * (xn * xn)))
        yd = yn * rad + (p1 * (r2 + 2.0 * (yn * yn)) + (2.0 * p2) * xy)
        u = fx * xd + cx
        v = fy * yd + cy
        Ud = np.floor(u * 256.0 + 0.5)
        Vd = np.floor(v * 256.0 + 0.5)
        # validity on the doubles, before any conversion to an integer
        ok = (W > 0.0) & (den > 0.0) & np.isfinite(u) & np.isfinite(v) & (Ud >= 0.0) & (Ud <= 256.0 * (src_cols - 1)) & \
            (Vd >= 0.0) & (Vd <= 256.0 * (src_rows - 1))
    uv = np.full((rows, cols, 2), INVALID, np.int32)
    uv[..., 0][ok] = Ud[ok].astype(np.int32)
    uv[..., 1][ok] = Vd[ok].astype(np.int32)
    return uv, map_info(uv)


def map_info(uv):
    ok = uv[..., 0] != INVALID
    rr, cc = np.nonzero(ok)
    any_ = rr.size > 0
    return dict(num_pixels=int(ok.size), num_valid=int(rr.size), first_row=int(rr.min()) if any_ else -1,
                last_row=int(rr.max()) if any_ else -1, first_col=int(cc.min()) if any_ else -1,
                last_col=int(cc.max()) if any_ else -1)


def remap(uv, src, border=0):
    """the image of the map's shape: U8 bilinear with `border` at invalid entries; U16 / F32 the nearest pixel bit for bit, 0 /
    the quiet NaN at invalid entries"""
    src = np.asarray(src)
    rows, cols = uv.shape[:2]
    U, V = uv[..., 0].astype(np.int64), uv[..., 1].astype(np.int64)
    ok = uv[..., 0] != INVALID
    if src.dtype == np.uint8:
        out = np.full((rows, cols), border, np.uint8)
        if not ok.any():
            return out
        Uo, Vo = U[ok], V[ok]
        x0, y0 = Uo >> 8, Vo >> 8
        x1, y1 = np.minimum(x0 + 1, src.shape[1] - 1), np.minimum(y0 + 1, src.shape[0] - 1)
        fx, fy = Uo & 255, Vo & 255
        I = src.astype(np.int64)
        val = (I[y0, x0] * (256 - fx) * (256 - fy) + I[y0, x1] * fx * (256 - fy) + I[y1, x0] * (256 - fx) * fy +
               I[y1, x1] * fx * fy + 32768) >> 16
        out[ok] = val.astype(np.uint8)
        return out
    if src.dtype == np.uint16:
        bits, none = src, np.uint16(0)
    elif src.dtype == np.float32:
        bits, none = src.view(np.uint32), QUIET_NAN
    else:
        raise ValueError("uint8, uint16 or float32 expected")
    out = np.full((rows, cols), none, bits.dtype)
    if ok.any():
        out[ok] = bits[(V[ok] + 128) >> 8, (U[ok] + 128) >> 8]
    return out.view(src.dtype)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F64)


def stereo_rectify(KL, KR, R, t):
    """(R1, R2, Knew, baseline), or None for a degenerate calibration; X_right = R X_left + t"""
    KL, KR = np.asarray(KL, F64).reshape(3, 3), np.asarray(KR, F64).reshape(3, 3)
    R, t = np.asarray(R, F64).reshape(3, 3), np.asarray(t, F64).reshape(3)
    c = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)], F64)
    b = np.sqrt(_dot3(c, c))
    if not (b > 0.0) or not np.isfinite(b):
        return None
    e1 = c / b
    zm = np.array([(0.0 + R[2, 0]) / 2.0, (0.0 + R[2, 1]) / 2.0, (1.0 + R[2, 2]) / 2.0], F64)
    z = _cross3(zm, e1)
    zn = np.sqrt(_dot3(z, z))
    if not (zn > 0.0) or not np.isfinite(zn):
        return None
    e2 = z / zn
    e3 = _cross3(e1, e2)
    R1 = np.stack([e1, e2, e3])
    R2 = np.array([[_dot3(R1[i], R[j]) for j in range(3)] for i in range(3)], F64)
    f = (KL[1, 1] + KR[1, 1]) / 2.0
    Knew = np.array([[f, 0.0, (KL[0, 2] + KR[0, 2]) / 2.0], [0.0, f, (KL[1, 2] + KR[1, 2]) / 2.0], [0.0, 0.0, 1.0]], F64)
    return R1, R2, Knew, float(b)
