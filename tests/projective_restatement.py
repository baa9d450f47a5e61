"""Independent numpy restatement of the projective path (DESIGN.md "Projective path", section 4 "Fixed-point reduction").

Association in float32, in the documented operation order: it must give the library's correspondences bit for bit.
Factor rows in float64 for the correspondences the library reports: H, b, chi, the counts, one Gauss-Newton step, and
the fixed-point exponent with the largest scaled term and scaled sum -- the range contract the bit-for-bit tests cannot
see (oracle and device share the fixed-point arithmetic, so both would be wrong together).
Also a generator of random organised RGB-D pairs with every edge the finder has to handle.
"""
import math

import numpy as np

from srrg2_slam_interfaces_amd import _abi as abi

F = np.float32
PIX_BOUND = 8.0
SQRT3 = 1.7320508075688772


# ---- float32 transforms, operation order of the finder --------------------------------------------------------------
def se3_inverse32(A):
    """R^T, -R^T t (translation accumulated in float64, rounded once)"""
    A = np.asarray(A, F).reshape(3, 4)
    out = np.zeros((3, 4), F)
    out[:, :3] = A[:, :3].T
    for i in range(3):
        t = (float(A[0, i]) * float(A[0, 3]) + float(A[1, i]) * float(A[1, 3])) + float(A[2, i]) * float(A[2, 3])
        out[i, 3] = F(-t)
    return out


def se3_compose32(A, B):
    """A*B, every entry a float64 dot product rounded once to float32"""
    A = np.asarray(A, F).reshape(3, 4)
    B = np.asarray(B, F).reshape(3, 4)
    out = np.zeros((3, 4), F)
    a, b = A.astype(np.float64), B.astype(np.float64)
    for i in range(3):
        for j in range(3):
            out[i, j] = F((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j])
        out[i, 3] = F(((a[i, 0] * b[0, 3] + a[i, 1] * b[1, 3]) + a[i, 2] * b[2, 3]) + a[i, 3])
    return out


def finder_transform(X, sensor_in_robot=None):
    """robot_in_sensor * X: the transform that takes moving points into the camera frame"""
    S = np.eye(4, dtype=F)[:3] if sensor_in_robot is None else np.asarray(sensor_in_robot, F).reshape(3, 4)
    return se3_compose32(se3_inverse32(S), X)


def _xform(T, P):
    return np.stack([((T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2]) + T[i, 3] for i in range(3)], 1)


def _rot(T, P):
    return np.stack([(T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2] for i in range(3)], 1)


def project(cam, q):
    """pinhole projection with the image and depth bounds: (pixel or -1, u, v), all float32"""
    K = np.asarray(cam["K"], F).reshape(3, 3)
    with np.errstate(all="ignore"):
        u = (K[0, 0] * q[:, 0]) / q[:, 2] + K[0, 2]
        v = (K[1, 1] * q[:, 1]) / q[:, 2] + K[1, 2]
        uf, vf = u + F(0.5), v + F(0.5)
        ok = np.isfinite(q).all(1) & (q[:, 2] >= F(cam["depth_min"])) & (q[:, 2] <= F(cam["depth_max"]))
        ok &= (uf >= 0) & (uf < F(cam["cols"])) & (vf >= 0) & (vf < F(cam["rows"]))
        pix = np.where(ok, np.floor(np.where(ok, vf, 0)).astype(np.int64) * cam["cols"] +
                       np.floor(np.where(ok, uf, 0)).astype(np.int64), -1)
    return pix, u, v


def associate(data, X, gate, normal_cos=-2.0, sensor_in_robot=None, moving_normals=True):
    """the projective finder: (fixed_idx, moving_idx, response), ordered by moving index, float32 throughout.
    z-buffer: per pixel the moving point of minimum depth, ties to the smaller index."""
    T = finder_transform(X, sensor_in_robot)
    P = np.asarray(data["moving"], F).reshape(-1, 3)
    idx = np.arange(P.shape[0])
    with np.errstate(all="ignore"):
        q = _xform(T, P)
    pix, _, _ = project(data, q)
    pix[~np.isfinite(P).all(1)] = -1
    order = np.lexsort((idx, q[:, 2], pix))  # by pixel, then depth, then index
    order = order[pix[order] >= 0]
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = np.sort(order[first])
    fixed = np.asarray(data["fixed"], F)
    f, qw = fixed[pix[win]], q[win]
    with np.errstate(all="ignore"):
        dd = np.abs(f[:, 2] - qw[:, 2])
        d = f - qw
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        g = F(gate)
        keep = np.isfinite(f).all(1) & (dd <= g) & (d2 <= (F(2) * g) * (F(2) * g))
        nf_all, nm_all = data.get("fixed_normals"), data.get("moving_normals") if moving_normals else None
        if normal_cos > -1.0 and nf_all is not None and nm_all is not None:
            nf = np.asarray(nf_all, F)[pix[win]]
            rn = _rot(T, np.asarray(nm_all, F)[win])
            dot = (nf[:, 0] * rn[:, 0] + nf[:, 1] * rn[:, 1]) + nf[:, 2] * rn[:, 2]
            keep &= dot > F(normal_cos)
    return pix[win][keep].astype(np.int32), win[keep].astype(np.int32), dd[keep].astype(F)


# ---- factor rows in float64 ----------------------------------------------------------------------------------------
def _robust(kind, thr, chi):
    """float32 weight and kernelized flag (the classification is a float32 decision, as in the library)"""
    thr = F(thr)
    kern = np.zeros(chi.shape, bool) if kind == abi.ROBUST_NONE else ~(chi < thr)
    with np.errstate(all="ignore"):
        if kind == abi.ROBUST_CLAMP:
            wk = np.zeros_like(chi)
        elif kind == abi.ROBUST_SATURATED:
            wk = thr / chi
        else:
            wk = F(1) / (F(1) + chi / thr)
    return np.where(kern, wk, F(1)).astype(F), kern


def factor_rows(data, X, corr_fixed, corr_moving, slice_kind, kind, sensor_in_robot=None):
    """(J64 [C, rows, 6], e64 [C, rows], e32-based chi [C] float32, suppressed [C])"""
    T32 = finder_transform(X, sensor_in_robot)
    T = T32.astype(np.float64)
    P32 = np.asarray(data["moving"], F)[corr_moving]
    f32 = np.asarray(data["fixed"], F)[corr_fixed]
    p, f = P32.astype(np.float64), f32.astype(np.float64)
    q = p @ T[:, :3].T + T[:, 3]
    q32 = _xform(T32, P32)
    kk = 2.0 if kind == abi.SE3_QUAT_RIGHT else 1.0
    C = len(corr_fixed)
    with np.errstate(all="ignore"):
        if slice_kind == abi.SLICE_REPROJECTION:
            K = np.asarray(data["K"], F).reshape(3, 3)
            fx, fy = float(K[0, 0]), float(K[1, 1])
            e = np.stack([fx * (q[:, 0] / q[:, 2] - f[:, 0] / f[:, 2]), fy * (q[:, 1] / q[:, 2] - f[:, 1] / f[:, 2])], 1)
            g = np.zeros((C, 2, 3))
            g[:, 0, 0] = fx / q[:, 2]
            g[:, 0, 2] = -fx * q[:, 0] / q[:, 2] ** 2
            g[:, 1, 1] = fy / q[:, 2]
            g[:, 1, 2] = -fy * q[:, 1] / q[:, 2] ** 2
            m = g @ T[:, :3]  # m_r = T_R^T g_r
            # float32 residual for the classification, in the library's order
            uq = (K[0, 0] * q32[:, 0]) / q32[:, 2] + K[0, 2]
            vq = (K[1, 1] * q32[:, 1]) / q32[:, 2] + K[1, 2]
            uf = (K[0, 0] * f32[:, 0]) / f32[:, 2] + K[0, 2]
            vf = (K[1, 1] * f32[:, 1]) / f32[:, 2] + K[1, 2]
            e32 = np.stack([uq - uf, vq - vf], 1)
            bad = ~(f32[:, 2] > 0) | ~(np.abs(e32[:, 0]) <= F(PIX_BOUND)) | ~(np.abs(e32[:, 1]) <= F(PIX_BOUND))
            e32 = np.where(~(f32[:, 2] > 0)[:, None], F(0), e32)
        else:
            n32 = np.asarray(data["fixed_normals"], F)[corr_fixed]
            n = n32.astype(np.float64)
            e = np.sum(n * (q - f), 1)[:, None]
            m = (n @ T[:, :3])[:, None, :]
            d = q32 - f32
            e32 = ((n32[:, 0] * d[:, 0] + n32[:, 1] * d[:, 1]) + n32[:, 2] * d[:, 2])[:, None]
            bad = np.zeros(C, bool)
        chi32 = e32[:, 0] * e32[:, 0]
        for r in range(1, e32.shape[1]):
            chi32 = chi32 + e32[:, r] * e32[:, r]
    J = np.concatenate([m, kk * np.cross(p[:, None, :], m)], 2)
    supp = bad | ~np.isfinite(chi32)
    return J, e, chi32.astype(F), supp


def slice_exponent(data, slice_kind, kind, gate, moving=None):
    """k = min(62 - ceil(log2 Nm) - ceil(log2 B), 50 - ceil(log2 B), 50), B = rows * max(J_b, e_b)^2"""
    P = np.asarray(data["moving"] if moving is None else moving, F)
    fin = np.isfinite(P).all(1)
    pinf = float(np.max(np.abs(P[fin]))) if fin.any() else 0.0
    kk = 2.0 if kind == abi.SE3_QUAT_RIGHT else 1.0
    if slice_kind == abi.SLICE_REPROJECTION:
        K = np.asarray(data["K"], F).reshape(3, 3)
        K0, K4, K2, K5 = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
        tx = float(proj_extent(data["cols"], K2)) / K0
        ty = float(proj_extent(data["rows"], K5)) / K4
        gb = (((K0 if K0 > K4 else K4) / float(F(data["depth_min"]))) * (1.0 + (tx if tx > ty else ty))) * 1.01
        mb = (SQRT3 * gb) * 1.01
        rows = 2
    else:
        N = np.asarray(data["fixed_normals"], F)
        Na = np.abs(N[np.isfinite(N)])
        ninf = float(Na.max()) if Na.size else 0.0
        mb = (SQRT3 * ninf) * 1.01
        rows = 1
    pf = (2.0 * kk) * pinf
    jb = mb * (pf if pf > 1.0 else 1.0)
    eb = (mb * (2.0 * float(F(gate)))) * 1.01
    if slice_kind == abi.SLICE_REPROJECTION:
        eb = PIX_BOUND * 1.01
    mx = jb if jb > eb else eb
    B = rows * (mx * mx)
    return fixed_point_exponent(P.shape[0], B)


def proj_extent(n, c):
    """max |u - c| of a projected point, u + 0.5 in [0, n) (float32 operations)"""
    n, c = F(n), F(c)
    return max(n, abs(c + F(0.5)), abs((n - F(0.5)) - c))


def _ceil_log2(v):
    m, e = math.frexp(v)  # v = m 2^e, m in [0.5, 1)
    return e - 1 if m == 0.5 else e


def fixed_point_exponent(n_terms, B):
    n_terms = max(n_terms, 1)
    B = B if B > 1e-30 else 1e-30
    lb = _ceil_log2(B)
    k = min(62 - _ceil_log2(float(n_terms)) - lb, 50 - lb, 50)
    return max(k, -64)


def linearize(data, X, corr_fixed, corr_moving, slice_kind, kind, robust=abi.ROBUST_NONE, thr=1.0, gate=0.05,
              sensor_in_robot=None):
    """float64 H, b, chi, counts, and the range of the fixed-point terms for one slice"""
    J, e, chi32, supp = factor_rows(data, X, corr_fixed, corr_moving, slice_kind, kind, sensor_in_robot)
    w, kern = _robust(robust, thr, np.where(supp, F(0), chi32))
    ok = ~supp
    w64 = np.where(ok, w.astype(np.float64), 0.0)
    Jz = np.where(ok[:, None, None], J, 0.0)
    ez = np.where(ok[:, None], e, 0.0)
    Hc = np.einsum("c,cra,crb->cab", w64, Jz, Jz)
    bc = np.einsum("c,cra,cr->ca", w64, Jz, ez)
    chi64 = np.sum(ez * ez, 1)
    k = slice_exponent(data, slice_kind, kind, gate)
    s = 2.0 ** k
    iu = np.triu_indices(6)
    terms = np.concatenate([np.abs(Hc[:, iu[0], iu[1]]), np.abs(bc), np.where(ok, np.abs(chi32), 0)[:, None]], 1) * s
    inl, out = ok & ~kern, ok & kern
    return {
        "H": Hc.sum(0), "b": bc.sum(0),
        # (chi of a factor is a float32 value of the library, e^T e of the float32 residual, by specification)
        "chi_inliers": float(chi32[inl].astype(np.float64).sum()),
        "chi_outliers": float(chi32[out].astype(np.float64).sum()),
        "chi64_inliers": float(chi64[inl].sum()),
        "num_inliers": int(inl.sum()), "num_outliers": int(out.sum()), "num_suppressed": int(supp.sum()),
        "num_correspondences": len(corr_fixed),
        "status": np.where(supp, abi.FACTOR_SUPPRESSED, np.where(kern, abi.FACTOR_KERNELIZED, abi.FACTOR_INLIER)),
        "k": k,
        "max_scaled_term": float(terms.max()) if terms.size else 0.0,
        # any order of the integer sums: bounded by the sum of the magnitudes
        "max_scaled_sum": float(terms.sum(0).max()) if terms.size else 0.0,
    }


def v2t(kind, dx):
    R = np.eye(3)
    if kind == abi.SE3_QUAT_RIGHT:
        x, y, z = dx[3:]
        n2 = x * x + y * y + z * z
        if n2 < 1.0:
            w = math.sqrt(1.0 - n2)
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                          [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                          [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    else:
        a, b, c = dx[3:]
        Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
        Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
        R = Rx @ Ry @ Rz
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = R, dx[:3]
    return T


def gauss_newton_step(X, H, b, kind):
    """X * v2t(-H^-1 b) in float64"""
    dx = -np.linalg.solve(H, b)
    X = np.asarray(X, np.float64).reshape(3, 4)
    D = v2t(kind, dx)
    out = np.zeros((3, 4))
    out[:, :3] = X[:, :3] @ D[:, :3]
    out[:, 3] = X[:, :3] @ D[:, 3] + X[:, 3]
    return out


# ---- generator of organised RGB-D pairs ----------------------------------------------------------------------------
def _se3(t, rpy):
    a, b, c = rpy
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.zeros((3, 4))
    T[:, :3] = Rz @ Ry @ Rx
    T[:, 3] = t
    return T


def _inv(T):
    T = np.asarray(T, np.float64)
    out = np.zeros((3, 4))
    out[:, :3] = T[:, :3].T
    out[:, 3] = -T[:, :3].T @ T[:, 3]
    return out


def rgbd_case(seed, rows=60, cols=80, fx=120.0, fy=None, cx=None, cy=None, depth_min=0.4, depth_max=8.0,
              depth_range=None, holes=0.03, nan_normals=0.0, density=1.0, duplicates=0.0, equal_depth=0.0,
              behind=0.0, nonfinite=0.0, on_bounds=0, moving_offset=0.0, motion=(0.01, 0.02), moving_normals=True,
              fixed_behind=0.0):
    """a depth field over a rows x cols grid unprojected with K (fixed, organised) and a moving cloud sampled from the same
    surface (``density`` points per pixel, sub-pixel positions) expressed in a frame X_gt away.  Edges on request:
    holes / NaN normals in the fixed image, exact duplicates and equal-depth neighbours (z-buffer ties), points behind the
    camera, NaN / inf coordinates, ``fixed_behind`` fixed pixels mirrored behind the camera (-0.5 x the pixel's point:
    finite, f_z < 0, the same projection), and ``on_bounds`` points on u + 0.5 == cols, q_z == depth_min, q_z == depth_max (exact
    for the identity guess).  ``moving_offset`` moves the moving frame's origin far from the points."""
    rng = np.random.default_rng(seed)
    fy = fx if fy is None else fy
    cx = (cols - 1) / 2.0 if cx is None else cx
    cy = (rows - 1) / 2.0 if cy is None else cy
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    lo, hi = depth_range if depth_range is not None else (depth_min, depth_max)
    lo, hi = max(lo, depth_min), min(hi, depth_max)

    def depth(u, v):  # smooth field, a tilted plane plus waves, inside [lo, hi]
        s = 0.5 + 0.25 * np.sin(0.37 * u + 0.11 * v + seed) + 0.2 * np.cos(0.05 * u - 0.23 * v) * (u / max(cols, 1))
        return lo + (hi - lo) * np.clip(s, 0.0, 1.0)

    def unproject(u, v, z):
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)

    vv, uu = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    Pf = unproject(uu, vv, depth(uu, vv))
    # normals from the neighbours of the analytic surface
    e = 0.5
    du = unproject(uu + e, vv, depth(uu + e, vv)) - unproject(uu - e, vv, depth(uu - e, vv))
    dv = unproject(uu, vv + e, depth(uu, vv + e)) - unproject(uu, vv - e, depth(uu, vv - e))
    Nf = np.cross(du, dv)
    Nf /= np.linalg.norm(Nf, axis=1, keepdims=True)
    Nf *= -np.sign(Nf[:, 2:3] + 1e-30)  # towards the camera
    Pf[rng.random(rows * cols) < holes] = np.nan
    mirror = rng.random(rows * cols) < fixed_behind
    Pf[mirror] *= -0.5
    Nf[rng.random(rows * cols) < nan_normals] = np.nan

    n = max(int(round(density * rows * cols)), 1)
    us = rng.uniform(-0.5, cols - 0.5, n)
    vs = rng.uniform(-0.5, rows - 0.5, n)
    Q = unproject(us, vs, depth(us, vs) * (1.0 + rng.normal(0, 0.002, n)))
    Nq = Nf[np.clip(np.round(vs), 0, rows - 1).astype(int) * cols + np.clip(np.round(us), 0, cols - 1).astype(int)]
    Nq = np.nan_to_num(Nq, nan=0.0) + np.array([0.0, 0.0, -1e-3])
    Nq /= np.linalg.norm(Nq, axis=1, keepdims=True)

    X_gt = _se3(rng.normal(0, motion[0], 3) + moving_offset, rng.normal(0, motion[1], 3))
    Ti = _inv(X_gt)
    Pm = (Q @ Ti[:, :3].T + Ti[:, 3]).astype(np.float32)
    Nm = (Nq @ Ti[:, :3].T).astype(np.float32)

    extra_p, extra_n = [], []
    if duplicates > 0:
        sel = rng.choice(n, max(int(duplicates * n), 1))
        extra_p.append(Pm[sel])
        extra_n.append(Nm[sel])
    if equal_depth > 0:  # same depth, a hair apart sideways: ties for the identity guess
        sel = rng.choice(n, max(int(equal_depth * n), 1))
        P2 = Pm[sel].copy()
        P2[:, 0] = np.nextafter(P2[:, 0], np.float32(np.inf))
        extra_p.append(P2)
        extra_n.append(Nm[sel])
    if behind > 0:
        sel = rng.choice(n, max(int(behind * n), 1))
        P2 = Pm[sel].copy()
        P2[:, 2] = -np.abs(P2[:, 2]) - 0.1
        extra_p.append(P2)
        extra_n.append(Nm[sel])
    if on_bounds > 0:
        extra_p.append(_on_bounds(rng, on_bounds, K, rows, cols, depth_min, depth_max))
        extra_n.append(np.tile(np.float32([0, 0, -1]), (extra_p[-1].shape[0], 1)))
    if extra_p:
        Pm = np.concatenate([Pm] + extra_p)
        Nm = np.concatenate([Nm] + extra_n)
    perm = rng.permutation(Pm.shape[0])  # ties between any two indices, in either order
    Pm, Nm = Pm[perm], Nm[perm]
    if nonfinite > 0:
        sel = rng.choice(Pm.shape[0], max(int(nonfinite * Pm.shape[0]), 1), replace=False)
        Pm[sel, rng.integers(0, 3, sel.size)] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), sel.size)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    out = {"fixed": f32(Pf), "fixed_normals": f32(Nf), "moving": f32(Pm), "X_gt": f32(X_gt), "K": K, "rows": rows,
           "cols": cols, "depth_min": depth_min, "depth_max": depth_max}
    if moving_normals:
        out["moving_normals"] = f32(Nm)
    return out


def _on_bounds(rng, count, K, rows, cols, dmin, dmax):
    """points that land exactly on u + 0.5 == cols, q_z == depth_min or q_z == depth_max under the identity transform"""
    fx, cx, fy, cy = K[0, 0], K[0, 2], K[1, 1], K[1, 2]
    pts = []
    for i in range(count):
        which = i % 3
        z = F(dmin) if which == 1 else F(dmax) if which == 2 else F(rng.uniform(dmin, dmax))
        v = rng.uniform(0, rows - 1)
        y = F((v - cy) / fy * z)
        if which == 0:  # search the float32 x whose projection gives exactly u + 0.5 == cols
            x = F((cols - 0.5 - cx) / fx * z)
            for _ in range(64):
                uf = (fx * x) / z + cx + F(0.5)
                if uf == F(cols):
                    break
                x = np.nextafter(x, F(np.inf) if uf < F(cols) else F(-np.inf))
        else:
            x = F((rng.uniform(0, cols - 1) - cx) / fx * z)
        pts.append([x, y, z])
    return np.array(pts, np.float32)


# ---- the configurations the CPU and GPU edge tests share ----------------------------------------------------------
KINDS = (abi.SE3_QUAT_RIGHT, abi.SE3_EULER_RIGHT)
ROBUST = (abi.ROBUST_NONE, abi.ROBUST_CLAMP, abi.ROBUST_SATURATED, abi.ROBUST_CAUCHY)
SHAPES = ((1, 97), (97, 1), (7, 13), (257, 3), (3, 257), (120, 160), (33, 47), (60, 80))


def random_config(seed):
    """one seeded configuration: generator arguments, slice parameters, guess and sensor offset"""
    rng = np.random.default_rng(1000 + seed)
    rows, cols = SHAPES[seed % len(SHAPES)]
    fx = float(rng.choice([60.0, 150.0, 400.0, 1200.0]))
    dmin = float(rng.choice([0.05, 0.3, 0.5]))
    gen = dict(rows=rows, cols=cols, fx=fx, fy=fx * float(rng.choice([1.0, 0.7, 1.4])),
               cx=float(rng.choice([(cols - 1) / 2.0, -0.5, cols - 0.5, -3.0 * cols, 2.5 * cols, rng.uniform(0, cols)])),
               cy=float(rng.choice([(rows - 1) / 2.0, -0.5, rows - 0.5, -2.0 * rows, rng.uniform(0, rows)])),
               depth_min=dmin, depth_max=float(rng.choice([3.0, 8.0])), holes=float(rng.choice([0.0, 0.05])),
               nan_normals=float(rng.choice([0.0, 0.05])), density=float(rng.choice([0.5, 1.0, 3.0])),
               duplicates=float(rng.choice([0.0, 0.05])), equal_depth=float(rng.choice([0.0, 0.05])),
               behind=float(rng.choice([0.0, 0.02])), nonfinite=float(rng.choice([0.0, 0.01])),
               on_bounds=int(rng.choice([0, 12])), moving_normals=bool(rng.integers(0, 4) > 0))
    gen["depth_range"] = (dmin, min(dmin + float(rng.choice([0.2, 2.0])), gen["depth_max"]))
    par = dict(kind=KINDS[seed % 2], slice_kind=(abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION)[(seed // 2) % 2],
               robust=ROBUST[(seed // 4) % 4], gate=float(rng.choice([0.02, 0.05, 0.2])),
               normal_cos=float(rng.choice([-2.0, 0.5, 0.9])), sensor=bool(rng.integers(0, 3) == 0),
               guess=str(rng.choice(["gt", "identity", "perturbed"])))
    par["thr"] = 0.5 if par["slice_kind"] == abi.SLICE_REPROJECTION else 1e-5
    if gen["on_bounds"]:
        par["guess"], par["sensor"] = "identity", False  # (exact bound hits need the identity transform)
        gen["motion"] = (0.0, 0.0)
    return gen, par


def sensor_offset(seed):
    return _se3(np.array([0.05, -0.02, 0.1]), np.deg2rad([1.0, -2.0, 0.5]) * (1 + seed % 3)).astype(np.float32)


def make_case(gen, par, seed):
    """(data, guess, sensor_in_robot or None) for one configuration"""
    d = rgbd_case(seed, **gen)
    S = sensor_offset(seed) if par.get("sensor") else None
    X_cam = np.asarray(d["X_gt"], np.float64)
    if par["guess"] == "identity":
        X_cam = np.eye(4)[:3]
    elif par["guess"] == "perturbed":
        P = _se3(np.array([0.004, -0.003, 0.002]), np.deg2rad([0.2, -0.1, 0.15]))
        X_cam = np.concatenate([X_cam[:, :3] @ P[:, :3], (X_cam[:, :3] @ P[:, 3] + X_cam[:, 3])[:, None]], 1)
    if S is None:
        return d, X_cam.astype(np.float32), None
    S64 = S.astype(np.float64)  # robot guess X with S^-1 X = X_cam
    X = np.concatenate([S64[:, :3] @ X_cam[:, :3], (S64[:, :3] @ X_cam[:, 3] + S64[:, 3])[:, None]], 1)
    return d, X.astype(np.float32), S


def expected(d, X, par, S=None, moving_normals=True):
    """the restatement's association and first linearisation of one configuration"""
    fi, mi, resp = associate(d, X, par["gate"], par["normal_cos"], S, moving_normals)
    lin = linearize(d, X, fi, mi, par["slice_kind"], par["kind"], par["robust"], par["thr"], par["gate"], S)
    return fi, mi, resp, lin
