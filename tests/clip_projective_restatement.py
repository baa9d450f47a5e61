"""Independent numpy restatement of the projective clipper's contract (DESIGN.md section 4 "Projective clipping"): float32 in the
written operation order, whole arrays with float32 scalars, ``np.minimum.at`` for the per-pixel depth minimum.  It knows
nothing of the library: the GPU tests compare srrg2_scene_clip_projective against it bit for bit."""
import numpy as np

F = np.float32
CLIPPER_SUCCESSFUL, CLIPPER_READY = 1, 2


def se3_inverse(T):
    """[R|t] -> [R^T | -(R^T t)]: the translation summed in float64 as ((a + b) + c), rounded once"""
    T = np.asarray(T, F).reshape(3, 4)
    out = np.zeros((3, 4), F)
    out[:, :3] = T[:, :3].T
    D = T.astype(np.float64)
    for i in range(3):
        out[i, 3] = F(-((D[0, i] * D[0, 3] + D[1, i] * D[1, 3]) + D[2, i] * D[2, 3]))
    return out


def xform(M, P):
    """rows of [R|t] applied as ((m0*x + m1*y) + m2*z) + m3, float32 throughout"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1).astype(F)


def rotate(M, N):
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.stack([(M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z for r in range(3)], axis=1).astype(F)


def clip_projective(points, robot_in_local_map, K, rows, cols, depth_min=0.4, depth_max=8.0, sensor_in_robot=None,
                    occlusion_margin=-1.0, normals=None, descriptors=None, intensity=None):
    """-> dict: points / normals (robot frame; normals None when the scene has none), global_indices, descriptors, intensity,
    num_valid, num_in_view, num_kept, status, and per scene point: pix (-1 = not in view) and depth (camera z)"""
    P = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = P.shape[0]
    K = np.asarray(K, F).reshape(3, 3)
    L = se3_inverse(robot_in_local_map)
    S = se3_inverse(np.eye(3, 4, dtype=F) if sensor_in_robot is None else sensor_in_robot)
    margin = F(occlusion_margin)
    with np.errstate(all="ignore"):
        valid = np.isfinite(P).all(axis=1)
        R = xform(L, P)
        Cm = xform(S, R)
        cx, cy, cz = Cm[:, 0], Cm[:, 1], Cm[:, 2]
        ok = valid & np.isfinite(Cm).all(axis=1) & (cz >= F(depth_min)) & (cz <= F(depth_max))
        u = (K[0, 0] * cx) / cz + K[0, 2]
        v = (K[1, 1] * cy) / cz + K[1, 2]
        uf, vf = u + F(0.5), v + F(0.5)
        in_view = ok & (uf >= F(0)) & (uf < F(cols)) & (vf >= F(0)) & (vf < F(rows))
        pix = np.full(n, -1, np.int64)
        pix[in_view] = np.floor(vf[in_view]).astype(np.int64) * cols + np.floor(uf[in_view]).astype(np.int64)
        keep = in_view.copy()
        if margin >= 0:
            zmin = np.full(rows * cols, np.inf, F)
            np.minimum.at(zmin, pix[in_view], cz[in_view])
            keep[in_view] = cz[in_view] <= zmin[pix[in_view]] + margin
        g = np.flatnonzero(keep).astype(np.int32)
        out_n = None if normals is None else rotate(L, np.ascontiguousarray(normals, F).reshape(-1, 3)[g])
    return {"points": R[g], "normals": out_n, "global_indices": g,
            "descriptors": None if descriptors is None else np.ascontiguousarray(descriptors, np.uint8)[g],
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F)[g],
            "num_valid": int(valid.sum()), "num_in_view": int(in_view.sum()), "num_kept": int(len(g)),
            "status": CLIPPER_READY if n == 0 else CLIPPER_SUCCESSFUL, "pix": pix, "depth": cz}


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN == NaN whatever the payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
