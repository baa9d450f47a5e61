"""Independent numpy restatement of the scan clipper's contract (DESIGN.md section 4 "Scan clipping"): float32 in the written
operation order, the bearing by a float64 restatement of ``dm::atan2`` (csrc/det_math.h: fixed reduction + polynomial, + - * /
only), ``np.minimum.at`` for the per-beam range minimum.  It knows nothing of the library: the GPU tests compare
srrg2_scene_clip_scan against it bit for bit."""
import numpy as np

from clip_projective_restatement import same_bits  # noqa: F401  (the tests take it from here)

F = np.float32
D = np.float64
CLIPPER_SUCCESSFUL, CLIPPER_READY = 1, 2
TWO_PI = 6.283185307179586

# ---- atan2 of csrc/det_math.h ------------------------------------------------------------------------------------------
_HI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_LO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_A = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
      9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
      4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)
_PI_HI = 3.14159265358979311600e+00
_PI_LO = 1.22464679914735317720e-16


def _atan_pos(x):
    """atan of x >= 0: the interval of x picks a reduction, one polynomial serves all"""
    x = np.asarray(x, D)
    iv = np.full(x.shape, -1, np.int64)  # -1: x < 0.4375, no reduction
    iv[x >= 0.4375] = 0
    iv[x >= 0.6875] = 1
    iv[x >= 1.1875] = 2
    iv[x >= 2.4375] = 3
    with np.errstate(all="ignore"):
        red = [x, (2.0 * x - 1.0) / (2.0 + x), (x - 1.0) / (x + 1.0), (x - 1.5) / (1.0 + 1.5 * x), -1.0 / x]
        xr = np.choose(iv + 1, red)
        hi = np.choose(iv + 1, [0.0, *_HI])
        lo = np.choose(iv + 1, [0.0, *_LO])
        z = xr * xr
        w = z * z
        s1 = z * (_A[0] + w * (_A[2] + w * (_A[4] + w * (_A[6] + w * (_A[8] + w * _A[10])))))
        s2 = w * (_A[1] + w * (_A[3] + w * (_A[5] + w * (_A[7] + w * _A[9]))))
        return np.where(iv < 0, xr - xr * (s1 + s2), hi - ((xr * (s1 + s2) - lo) - xr))


def atan2(y, x):
    """dm::atan2: 0 at the origin, +-pi/2 on the y axis; the sign of the result is `y < 0`, so y = -0 counts as +0"""
    y, x = np.broadcast_arrays(np.asarray(y, D), np.asarray(x, D))
    ay, ax = np.where(y < 0.0, -y, y), np.where(x < 0.0, -x, x)
    with np.errstate(all="ignore"):
        z = _atan_pos(ay / ax)
    z = np.where(x < 0.0, _PI_HI - (z - _PI_LO), z)
    z = np.where(ax == 0.0, 0.5 * _PI_HI, z)
    z = np.where(y < 0.0, -z, z)
    return np.where((x == 0.0) & (y == 0.0), 0.0, z)


# ---- SE(2) ---------------------------------------------------------------------------------------------------------------
def se2_inverse(T):
    """row-major 3x3 [R|t] -> [R^T | -(R^T t)]: the translation summed in float64, rounded once"""
    T = np.asarray(T, F).reshape(3, 3)
    A = T.astype(D)
    out = np.eye(3, dtype=F)
    out[:2, :2] = T[:2, :2].T
    out[0, 2] = F(-(A[0, 0] * A[0, 2] + A[1, 0] * A[1, 2]))
    out[1, 2] = F(-(A[0, 1] * A[0, 2] + A[1, 1] * A[1, 2]))
    return out


def xform(M, P):
    """rows of [R|t] applied as (m0*x + m1*y) + m2, float32 throughout"""
    x, y = P[:, 0], P[:, 1]
    return np.stack([(M[r, 0] * x + M[r, 1] * y) + M[r, 2] for r in range(2)], axis=1).astype(F)


def rotate(M, N):
    x, y = N[:, 0], N[:, 1]
    return np.stack([M[r, 0] * x + M[r, 1] * y for r in range(2)], axis=1).astype(F)


def beam_of(cx, cy, angle_min, angle_increment, num_beams):
    """step 5: (beam, in sector) of sensor-frame points; float64"""
    angle_min, inc = D(angle_min), D(angle_increment)
    W = np.copysign(D(TWO_PI), inc)
    beta = atan2(cy.astype(D), cx.astype(D))
    d = beta - angle_min
    t = d / inc
    low, high = t < -0.5, t >= D(num_beams) - 0.5
    t = np.where(low, (d + W) / inc, np.where(high, (d - W) / inc, t))
    tf = t + 0.5
    ok = (tf >= 0.0) & (tf < D(num_beams))
    return np.where(ok, np.floor(np.where(ok, tf, 0.0)), -1).astype(np.int64), ok


def clip_scan(points, robot_in_local_map, angle_min, angle_increment, num_beams, range_min=0.05, range_max=30.0,
              sensor_in_robot=None, occlusion_margin=-1.0, normals=None, descriptors=None, intensity=None):
    """-> dict: points / normals (robot frame; normals None when the scene has none), global_indices, descriptors, intensity,
    num_valid, num_in_view, num_kept, status, and per scene point: beam (-1 = not in view) and rho (sensor-frame range)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 2)
    n = P.shape[0]
    L = se2_inverse(robot_in_local_map)
    S = se2_inverse(np.eye(3, dtype=F) if sensor_in_robot is None else sensor_in_robot)
    margin = F(occlusion_margin)
    with np.errstate(all="ignore"):
        valid = np.isfinite(P).all(axis=1)
        R = xform(L, P)
        Cm = xform(S, R)
        cx, cy = Cm[:, 0], Cm[:, 1]
        rho = np.sqrt(cx * cx + cy * cy).astype(F)
        ok = valid & np.isfinite(Cm).all(axis=1) & (rho >= F(range_min)) & (rho <= F(range_max))
        beam, in_sector = beam_of(np.where(ok, cx, F(1.0)), np.where(ok, cy, F(0.0)), angle_min, angle_increment, num_beams)
        in_view = ok & in_sector
        beam = np.where(in_view, beam, -1)
        keep = in_view.copy()
        if margin >= 0:
            rmin = np.full(num_beams, np.inf, F)
            np.minimum.at(rmin, beam[in_view], rho[in_view])
            keep[in_view] = rho[in_view] <= rmin[beam[in_view]] + margin
        g = np.flatnonzero(keep).astype(np.int32)
        out_n = None if normals is None else rotate(L, np.ascontiguousarray(normals, F).reshape(-1, 2)[g])
    return {"points": R[g], "normals": out_n, "global_indices": g,
            "descriptors": None if descriptors is None else np.ascontiguousarray(descriptors, np.uint8)[g],
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F)[g],
            "num_valid": int(valid.sum()), "num_in_view": int(in_view.sum()), "num_kept": int(len(g)),
            "status": CLIPPER_READY if n == 0 else CLIPPER_SUCCESSFUL, "beam": beam, "rho": rho}
