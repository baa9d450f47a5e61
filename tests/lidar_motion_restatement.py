"""Independent numpy restatement of DESIGN.md section 4 "Lidar sweeps", contracts 1 (ring elevation tables, shared by adaptor
and clipper) and 2 (motion de-skew, adaptor only).  Everything the uniform model and the single-pose sweep already say is taken
from ``lidar_restatement``; ``sincos`` is the float64 restatement of ``dm::sincos`` (adaptor_restatement), ``atan2`` that of
``dm::atan2`` (clip_scan_restatement).  It knows nothing of the library: the GPU tests compare srrg2_adapt_lidar_sweep_ex and
srrg2_scene_clip_spherical_rings against it bit for bit."""
import math

import numpy as np

import lidar_restatement as lr
from adaptor_restatement import sincos
from clip_projective_restatement import rotate, se3_inverse, xform
from clip_scan_restatement import atan2
from lidar_restatement import same_bits  # noqa: F401  (the tests take it from here)

F = np.float32
D = np.float64
HALF_PI = 1.5707963267948966
MAX_RING_ROWS = 256


# ---- contract 1: ring tables ----------------------------------------------------------------------------------------------
def ring_table_status(e, rows):
    """None when the table is usable, else 'invalid' / 'unsupported' (the refusals of contract 1, in their order)"""
    e = np.asarray(e, D).reshape(-1)
    if rows < 2:
        return "invalid"
    if rows > MAX_RING_ROWS:
        return "unsupported"
    lim = HALF_PI * (1.0 + lr.SLACK)
    if not np.all(np.isfinite(e)) or not np.all(np.abs(e) <= lim):
        return "invalid"
    d = np.diff(e)
    if not (np.all(d > 0) or np.all(d < 0)):
        return "invalid"
    return None


def ring_boundaries(e):
    """-> (B[0 .. rows] = sigma * b, ascending either way; descending?)"""
    e = np.asarray(e, D).reshape(-1)
    rows = e.shape[0]
    b = np.empty(rows + 1, D)
    b[0] = e[0] - (e[1] - e[0]) * 0.5
    b[1:rows] = (e[:-1] + e[1:]) * 0.5
    b[rows] = e[rows - 1] + (e[rows - 1] - e[rows - 2]) * 0.5
    descending = bool(e[1] < e[0])
    return (-b if descending else b), descending


def project_rings(x, y, z, m, e):
    """steps 1-7 with the rows of the table `e` -> (pixel or -1, rho, tf: the continuous column coordinate of step 3)"""
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    B, descending = ring_boundaries(e)
    rows = len(B) - 1
    with np.errstate(all="ignore"):
        rho = np.sqrt((x * x + y * y) + z * z).astype(F)
        ok = (rho >= m.range_min) & (rho <= m.range_max)
        xd, yd, zd = x.astype(D), y.astype(D), z.astype(D)
        W = np.copysign(D(lr.TWO_PI), m.azimuth_increment)
        d = atan2(yd, xd) - m.azimuth_min
        t = d / m.azimuth_increment
        low, high = t < -0.5, t >= D(m.cols) - 0.5
        t = np.where(low, (d + W) / m.azimuth_increment, np.where(high, (d - W) / m.azimuth_increment, t))
        tf = t + 0.5
        ok &= (tf >= 0.0) & (tf < D(m.cols))
        h = np.sqrt(xd * xd + yd * yd)
        eps = atan2(zd, h)
        u = -eps if descending else eps
        ok &= (u >= B[0]) & (u < B[rows])
        # row = max{k : B[k] <= u}: the number of boundaries <= u, less one
        row = np.searchsorted(B, np.where(ok, u, B[0]), side="right") - 1
        col = np.floor(np.where(ok, tf, 0.0)).astype(np.int64)
    return np.where(ok, row * m.cols + col, -1), rho, tf


def project_uniform(x, y, z, m):
    """the uniform model's projection, with the column coordinate the azimuth fallback needs -> (pixel or -1, rho, tf)"""
    pix, rho = lr.project(x, y, z, m)
    x, y = np.asarray(x, F).astype(D), np.asarray(y, F).astype(D)
    with np.errstate(all="ignore"):
        W = np.copysign(D(lr.TWO_PI), m.azimuth_increment)
        d = atan2(y, x) - m.azimuth_min
        t = d / m.azimuth_increment
        t = np.where(t < -0.5, (d + W) / m.azimuth_increment, np.where(t >= D(m.cols) - 0.5, (d - W) / m.azimuth_increment, t))
    return pix, rho, t + 0.5


# ---- contract 2: de-skew ------------------------------------------------------------------------------------------------
def _r_to_quat(R):
    """dm::R_to_quat: unit quaternion (w, x, y, z), w >= 0, float64 in the written order"""
    R = [D(v) for v in np.asarray(R, D).reshape(9)]
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        s = D(math.sqrt(tr + 1.0)) * 2.0
        w, x, y, z = 0.25 * s, (R[7] - R[5]) / s, (R[2] - R[6]) / s, (R[3] - R[1]) / s
    elif R[0] > R[4] and R[0] > R[8]:
        s = D(math.sqrt(((1.0 + R[0]) - R[4]) - R[8])) * 2.0
        w, x, y, z = (R[7] - R[5]) / s, 0.25 * s, (R[1] + R[3]) / s, (R[2] + R[6]) / s
    elif R[4] > R[8]:
        s = D(math.sqrt(((1.0 + R[4]) - R[0]) - R[8])) * 2.0
        w, x, y, z = (R[2] - R[6]) / s, (R[1] + R[3]) / s, 0.25 * s, (R[5] + R[7]) / s
    else:
        s = D(math.sqrt(((1.0 + R[8]) - R[0]) - R[4])) * 2.0
        w, x, y, z = (R[3] - R[1]) / s, (R[2] + R[6]) / s, (R[5] + R[7]) / s, 0.25 * s
    n = D(math.sqrt(((w * w + x * x) + y * y) + z * z))
    w, x, y, z = w / n, x / n, y / n, z / n
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    return D(w), D(x), D(y), D(z)


def axis_angle(motion):
    """the host side: motion (3x4 float32) -> (theta, axis (3,), t (3,)), float64"""
    M = np.asarray(motion, F).reshape(3, 4).astype(D)
    w, x, y, z = _r_to_quat(M[:, :3])
    vn = D(math.sqrt((x * x + y * y) + z * z))
    if vn == 0.0:
        return D(0.0), np.array([0.0, 0.0, 1.0], D), M[:, 3].copy()
    theta = 2.0 * D(atan2(vn, w))
    return D(theta), np.array([x / vn, y / vn, z / vn], D), M[:, 3].copy()


def _rodrigues(a, sn, cs, p):
    """p*cs + (a x p)*sn + a*((a.p)*(1 - cs)) for points p (..., 3); sn, cs scalars or (...,)"""
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    omc = 1.0 - cs
    cx, cy, cz = a[1] * pz - a[2] * py, a[2] * px - a[0] * pz, a[0] * py - a[1] * px
    k = ((a[0] * px + a[1] * py) + a[2] * pz) * omc
    return np.stack([(px * cs + cx * sn) + a[0] * k, (py * cs + cy * sn) + a[1] * k, (pz * cs + cz * sn) + a[2] * k], -1)


def deskew(points, s, motion, reference=1.0):
    """raw points (n, 3) float32 fired at normalised times s (n,) float64 -> float32 points in the sensor frame at `reference`"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3).astype(D)
    s = np.asarray(s, D).reshape(-1)
    theta, a, t = axis_angle(motion)
    reference = D(reference)
    with np.errstate(all="ignore"):
        sr, cr = sincos(reference * theta)
        Rref = _rodrigues(a, D(sr), D(cr), np.eye(3, dtype=D)).T  # column j = the rotation of e_j
        rt = reference * t
        sn, cs = sincos(s * theta)
        q = _rodrigues(a, sn, cs, P)
        q = q + s[:, None] * t[None, :]
        v = q - rt[None, :]
        out = np.stack([(Rref[0, j] * v[:, 0] + Rref[1, j] * v[:, 1]) + Rref[2, j] * v[:, 2] for j in range(3)], -1)
    return out.astype(F)


def normalised_time(times, time_begin, time_end):
    return (np.asarray(times, F).astype(D) - D(time_begin)) / (D(time_end) - D(time_begin))


# ---- the adaptor with extras -----------------------------------------------------------------------------------------------
def adapt_lidar_sweep_ex(points, m, ring_elevations=None, motion=None, reference=1.0, times=None, time_begin=0.0, time_end=1.0,
                         col_gap=1, row_gap=1, max_distance_squared=1.0, drop_points_without_normal=True, compact=False,
                         intensity=None):
    """lidar_restatement.adapt_lidar_sweep's dict.  ring_elevations None: the model's uniform rows; motion None: no de-skew;
    times None with a motion: the time comes from the raw azimuth."""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, rows, cols = P.shape[0], m.rows, m.cols
    if ring_elevations is None and motion is None:
        return lr.adapt_lidar_sweep(P, m, col_gap, row_gap, max_distance_squared, drop_points_without_normal, compact, intensity)
    npix = rows * cols
    gc, gr = int(col_gap), int(row_gap)
    want_normals = gc > 0
    if n == 0:
        return lr.adapt_lidar_sweep(P, m, col_gap, row_gap, max_distance_squared, drop_points_without_normal, compact, intensity)
    # step A, from the RAW coordinates
    finite = np.isfinite(P).all(axis=1)
    s = None
    if motion is not None and times is not None:
        s = normalised_time(times, time_begin, time_end)
        finite &= np.isfinite(np.asarray(times, F).reshape(-1))
    Q = np.where(finite[:, None], P, F(1.0))
    if ring_elevations is None:
        pix, rho, tf = project_uniform(Q[:, 0], Q[:, 1], Q[:, 2], m)
    else:
        pix, rho, tf = project_rings(Q[:, 0], Q[:, 1], Q[:, 2], m, ring_elevations)
    seen = finite & (pix >= 0)
    winner = np.full(npix, lr.EMPTY, np.uint64)
    keys = (rho.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    np.minimum.at(winner, pix[seen], keys[seen])
    candidates = np.bincount(pix[seen], minlength=npix)
    # what step B reads as a winner's coordinates
    if motion is not None:
        if s is None:
            s = tf / D(cols)
        C = deskew(Q, np.where(seen, s, 0.0), motion, reference)
    else:
        C = P
    occ = (winner != lr.EMPTY).reshape(rows, cols)
    idx = np.where(occ, (winner & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(rows, cols), 0)
    img = C[idx]
    N = np.full((rows, cols, 3), np.nan, F)
    has_n = np.zeros((rows, cols), bool)
    if want_normals:
        r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        inside = (r >= gr) & (r < rows - gr)
        if m.columns_wrap():
            cl, cr = (c - gc) % cols, (c + gc) % cols
        else:
            inside &= (c >= gc) & (c < cols - gc)
            cl, cr = np.clip(c - gc, 0, cols - 1), np.clip(c + gc, 0, cols - 1)
        ru, rd = np.clip(r - gr, 0, rows - 1), np.clip(r + gr, 0, rows - 1)
        ok = occ & inside & occ[r, cl] & occ[r, cr] & occ[ru, c] & occ[rd, c]
        with np.errstate(all="ignore"):
            dc = img[r, cr] - img[r, cl]
            dr = img[rd, c] - img[ru, c]
            ok &= ~(lr._sq(dc) > F(max_distance_squared)) & ~(lr._sq(dr) > F(max_distance_squared))
            nx = dc[..., 1] * dr[..., 2] - dc[..., 2] * dr[..., 1]
            ny = dc[..., 2] * dr[..., 0] - dc[..., 0] * dr[..., 2]
            nz = dc[..., 0] * dr[..., 1] - dc[..., 1] * dr[..., 0]
            nn = np.stack([nx, ny, nz], -1)
            ln = np.sqrt(lr._sq(nn))
            ok &= ln > 0
            nn = nn / ln[..., None]
            flip = (nn[..., 0] * img[..., 0] + nn[..., 1] * img[..., 1]) + nn[..., 2] * img[..., 2] > 0
            nn = np.where(flip[..., None], -nn, nn)
        N[ok] = nn[ok]
        has_n = ok
    valid = occ & (has_n | (not drop_points_without_normal)) if want_normals else occ.copy()
    pts = np.where(valid[..., None], img, F(np.nan)).astype(F).reshape(npix, 3)
    nrm = N.reshape(npix, 3) if want_normals else None
    it = None
    if intensity is not None:
        it = np.where(occ, np.ascontiguousarray(intensity, F).reshape(-1)[idx], F(0.0)).astype(F).reshape(npix)
    vflat = valid.reshape(npix)
    out = {"occupied": occ.reshape(npix), "has_normal": has_n.reshape(npix), "valid": vflat, "candidates": candidates,
           "num_raw": n, "num_in_range": int(occ.sum()), "num_valid": int(vflat.sum()), "global_indices": None,
           "status": lr.ADAPTOR_READY, "winner_index": np.where(occ, idx, -1).reshape(npix)}
    if compact:
        g = np.flatnonzero(vflat).astype(np.int32)
        pts, nrm, it = pts[g], (None if nrm is None else nrm[g]), (None if it is None else it[g])
        out["global_indices"] = g
    out.update(points=pts, normals=nrm, intensity=it, scene_size=int(pts.shape[0]))
    return out


# ---- the clipper with a ring table --------------------------------------------------------------------------------------
def clip_spherical_rings(points, robot_in_local_map, m, ring_elevations, sensor_in_robot=None, occlusion_margin=-1.0,
                         normals=None, intensity=None):
    """lidar_restatement.clip_spherical's dict, the rows from the table"""
    if ring_elevations is None:
        return lr.clip_spherical(points, robot_in_local_map, m, sensor_in_robot, occlusion_margin, normals=normals,
                                 intensity=intensity)
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = P.shape[0]
    L = se3_inverse(robot_in_local_map)
    S = se3_inverse(np.eye(3, 4, dtype=F) if sensor_in_robot is None else sensor_in_robot)
    margin = F(occlusion_margin)
    with np.errstate(all="ignore"):
        valid = np.isfinite(P).all(axis=1)
        R = xform(L, P)
        Cm = xform(S, R)
        ok = valid & np.isfinite(Cm).all(axis=1)
        Q = np.where(ok[:, None], Cm, F(1.0))
        pix, rho, _ = project_rings(Q[:, 0], Q[:, 1], Q[:, 2], m, ring_elevations)
        in_view = ok & (pix >= 0)
        pix = np.where(in_view, pix, -1)
        keep = in_view.copy()
        if margin >= 0:
            rmin = np.full(m.rows * m.cols, np.inf, F)
            np.minimum.at(rmin, pix[in_view], rho[in_view])
            keep[in_view] = rho[in_view] <= rmin[pix[in_view]] + margin
        g = np.flatnonzero(keep).astype(np.int32)
        out_n = None if normals is None else rotate(L, np.ascontiguousarray(normals, F).reshape(-1, 3)[g])
    return {"points": R[g], "normals": out_n, "global_indices": g,
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F)[g],
            "num_valid": int(valid.sum()), "num_in_view": int(in_view.sum()), "num_kept": int(len(g)),
            "status": lr.CLIPPER_READY if n == 0 else lr.CLIPPER_SUCCESSFUL, "pix": pix, "rho": rho}
