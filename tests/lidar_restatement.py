"""Independent numpy restatement of DESIGN.md section 4 "Lidar sweeps": the spherical sensor model and its projection, the sweep
adaptor (point list -> range image -> scene with normals) and the spherical clipper.  float32 in the written operation order,
both angles by the float64 restatement of ``dm::atan2`` (clip_scan_restatement), ``np.minimum.at`` on uint64 keys for the
per-pixel winner and on float32 ranges for the clipper's per-pixel minimum.  It knows nothing of the library: the GPU tests
compare srrg2_adapt_lidar_sweep and srrg2_scene_clip_spherical against it bit for bit."""
import numpy as np

from clip_projective_restatement import rotate, se3_inverse, xform
from clip_scan_restatement import atan2, same_bits  # noqa: F401  (the tests take same_bits from here)

F = np.float32
D = np.float64
PI = 3.141592653589793
TWO_PI = 6.283185307179586
SLACK = 2.0 ** -20
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ADAPTOR_READY, ADAPTOR_INITIALIZING = 0, 1
CLIPPER_SUCCESSFUL, CLIPPER_READY = 1, 2


class Model:
    """srrg2_spherical_model: azimuth of column c = azimuth_min + c*azimuth_increment, elevation of row r likewise"""

    def __init__(self, azimuth_min, azimuth_increment, elevation_min, elevation_increment, rows, cols, range_min=0.5,
                 range_max=120.0):
        self.azimuth_min, self.azimuth_increment = D(azimuth_min), D(azimuth_increment)
        self.elevation_min, self.elevation_increment = D(elevation_min), D(elevation_increment)
        self.rows, self.cols = int(rows), int(cols)
        self.range_min, self.range_max = F(range_min), F(range_max)

    @classmethod
    def full_turn(cls, rows, cols, elevation_first, elevation_last, **kw):
        """columns tiling [-pi, pi), rows from elevation_first to elevation_last"""
        return cls(-PI + PI / D(cols), (2.0 * PI) / D(cols), elevation_first,
                   (D(elevation_last) - D(elevation_first)) / D(rows - 1), rows, cols, **kw)

    def valid(self):
        with np.errstate(all="ignore"):
            if self.rows <= 0 or self.cols <= 0 or self.rows * self.cols > 0x7FFFFFFF:
                return False
            ai, ei = self.azimuth_increment, self.elevation_increment
            if not (np.isfinite(ai) and np.isfinite(ei)) or ai == 0.0 or ei == 0.0:
                return False
            if not np.isfinite(self.azimuth_min) or abs(self.azimuth_min) > TWO_PI:
                return False
            if abs(ai) * D(self.cols) > (TWO_PI + abs(ai)) * (1.0 + SLACK):
                return False
            last = self.elevation_min + D(self.rows - 1) * ei
            lim = (0.5 * PI) * (1.0 + SLACK)
            if not np.isfinite(self.elevation_min) or not abs(self.elevation_min) <= lim or not abs(last) <= lim:
                return False
            return bool(self.range_min > 0 and self.range_max >= self.range_min)

    def columns_wrap(self):
        return bool(abs(abs(self.azimuth_increment) * D(self.cols) - TWO_PI) <= TWO_PI * SLACK)


def project(x, y, z, m):
    """steps 1-7 for float32 arrays of finite sensor-frame coordinates -> (pixel or -1, rho)"""
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    with np.errstate(all="ignore"):
        rho = np.sqrt((x * x + y * y) + z * z).astype(F)
        ok = (rho >= m.range_min) & (rho <= m.range_max)
        xd, yd, zd = x.astype(D), y.astype(D), z.astype(D)
        # column: exactly the scan clipper's binning of a bearing
        W = np.copysign(D(TWO_PI), m.azimuth_increment)
        d = atan2(yd, xd) - m.azimuth_min
        t = d / m.azimuth_increment
        low, high = t < -0.5, t >= D(m.cols) - 0.5
        t = np.where(low, (d + W) / m.azimuth_increment, np.where(high, (d - W) / m.azimuth_increment, t))
        cf = t + 0.5
        ok &= (cf >= 0.0) & (cf < D(m.cols))
        # row: no wrap
        h = np.sqrt(xd * xd + yd * yd)
        rf = (atan2(zd, h) - m.elevation_min) / m.elevation_increment + 0.5
        ok &= (rf >= 0.0) & (rf < D(m.rows))
        col = np.floor(np.where(ok, cf, 0.0)).astype(np.int64)
        row = np.floor(np.where(ok, rf, 0.0)).astype(np.int64)
    return np.where(ok, row * m.cols + col, -1), rho


def _sq(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def bin_sweep(points, m):
    """step A -> (winner keys per pixel (uint64, EMPTY = none), candidates per pixel)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, npix = P.shape[0], m.rows * m.cols
    winner = np.full(npix, EMPTY, np.uint64)
    finite = np.isfinite(P).all(axis=1)
    Q = np.where(finite[:, None], P, F(1.0))
    pix, rho = project(Q[:, 0], Q[:, 1], Q[:, 2], m)
    seen = finite & (pix >= 0)
    keys = (rho.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    np.minimum.at(winner, pix[seen], keys[seen])
    return winner, np.bincount(pix[seen], minlength=npix)


def adapt_lidar_sweep(points, m, col_gap=1, row_gap=1, max_distance_squared=1.0, drop_points_without_normal=True,
                      compact=False, intensity=None):
    """dict(points (k, 3), normals (k, 3) or None, intensity (k,) or None, global_indices (compact) or None, occupied,
    has_normal, valid (rows*cols masks), candidates (per pixel), num_raw, num_in_range, num_valid, scene_size, status).
    Organised: k = rows*cols, empty or dropped = NaN (intensity of an empty pixel: 0)."""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, rows, cols = P.shape[0], m.rows, m.cols
    npix = rows * cols
    gc, gr = int(col_gap), int(row_gap)
    want_normals = gc > 0
    if n == 0:
        e3 = np.zeros((0, 3), F)
        return {"points": e3, "normals": e3 if want_normals else None, "intensity": None if intensity is None else np.zeros(0, F),
                "global_indices": np.zeros(0, np.int32) if compact else None, "num_raw": 0, "num_in_range": 0, "num_valid": 0,
                "scene_size": 0, "status": ADAPTOR_INITIALIZING}
    winner, candidates = bin_sweep(P, m)
    occ = (winner != EMPTY).reshape(rows, cols)
    idx = np.where(occ, (winner & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(rows, cols), 0)
    img = P[idx]  # (rows, cols, 3): the winners' input coordinates, verbatim (rubbish where the pixel is empty)
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
            ok &= ~(_sq(dc) > F(max_distance_squared)) & ~(_sq(dr) > F(max_distance_squared))
            nx = dc[..., 1] * dr[..., 2] - dc[..., 2] * dr[..., 1]
            ny = dc[..., 2] * dr[..., 0] - dc[..., 0] * dr[..., 2]
            nz = dc[..., 0] * dr[..., 1] - dc[..., 1] * dr[..., 0]
            nn = np.stack([nx, ny, nz], -1)
            ln = np.sqrt(_sq(nn))
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
           "status": ADAPTOR_READY}
    if compact:
        g = np.flatnonzero(vflat).astype(np.int32)
        pts, nrm, it = pts[g], (None if nrm is None else nrm[g]), (None if it is None else it[g])
        out["global_indices"] = g
    out.update(points=pts, normals=nrm, intensity=it, scene_size=int(pts.shape[0]))
    return out


def clip_ball(points, robot_in_local_map, range_max):
    """the ball clipper's contract, for comparison: (robot-frame points of the kept, their scene indices)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    L = se3_inverse(robot_in_local_map)
    with np.errstate(all="ignore"):
        R = xform(L, P)
        keep = np.isfinite(P).all(axis=1) & (_sq(R) <= F(range_max) * F(range_max))
    g = np.flatnonzero(keep).astype(np.int32)
    return R[g], g


def clip_spherical(points, robot_in_local_map, m, sensor_in_robot=None, occlusion_margin=-1.0, normals=None, descriptors=None,
                   intensity=None):
    """-> dict: points / normals (robot frame; normals None when the scene has none), global_indices, descriptors, intensity,
    num_valid, num_in_view, num_kept, status, and per scene point: pix (-1 = not in view) and rho (sensor-frame range)"""
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
        pix, rho = project(Q[:, 0], Q[:, 1], Q[:, 2], m)
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
            "descriptors": None if descriptors is None else np.ascontiguousarray(descriptors, np.uint8)[g],
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F)[g],
            "num_valid": int(valid.sum()), "num_in_view": int(in_view.sum()), "num_kept": int(len(g)),
            "status": CLIPPER_READY if n == 0 else CLIPPER_SUCCESSFUL, "pix": pix, "rho": rho}
