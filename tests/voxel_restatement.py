"""numpy restatement of srrg2_scene_voxelize: the executable form of DESIGN.md section 4 "Voxel-grid decimation".  A plain loop
over the occupied cells; every value goes through exactly the operations of the contract, in its order, so the device's points,
normals, counts and indices equal these bit for bit.

How the cells are FOUND is not part of the contract (np.unique here, a radix sort of 64-bit keys on the device); which extents
the device's key can hold is (``key_layout``).
"""
import numpy as np

from normals_restatement import exponents, same_bits  # noqa: F401  (same_bits: re-exported for the tests)

F32, F64, I64 = np.float32, np.float64, np.int64
CENTROID, FIRST = 0, 1
AXIS_BITS, KEY_BITS = 30, 63


def _rows(a, dtype):
    """a as a 2-D array of rows (an empty cloud keeps its width)"""
    a = np.ascontiguousarray(a, dtype)
    return a if a.ndim == 2 else a.reshape(len(a), -1)


def cells_of(points, leaf_size, origin, dim):
    """(participating (n,) bool, cells (n, dim) float64 whole numbers -- rows of non-participating points are meaningless)"""
    P = _rows(points, F32)[:, :dim]
    part = np.isfinite(P).all(1)
    org = np.asarray(origin, F32)[:dim].astype(F64)
    with np.errstate(all="ignore"):
        c = np.floor((P.astype(F64) - org[None, :]) / F64(F32(leaf_size)))
    return part, c


def key_layout(points, leaf_size, origin, dim):
    """None when the device's 64-bit cell key cannot hold the extent (SRRG2_E_UNSUPPORTED), else the bits per axis: cell
    coordinates relative to the lowest occupied cell per axis, at most 2^30 cells per axis, 63 bits over the axes"""
    part, c = cells_of(points, leaf_size, origin, dim)
    if not part.any():
        return [0] * dim
    span = c[part].max(0) - c[part].min(0)
    if not (span < F64(1 << AXIS_BITS)).all():
        return None
    bits = [int(s).bit_length() for s in span]
    return bits if sum(bits) <= KEY_BITS else None


def voxelize(points, leaf_size, dim=None, origin=(0.0, 0.0, 0.0), mode=CENTROID, min_points=1, normals=None, descriptors=None,
             intensity=None):
    """the whole call.  Returns a dict: points / normals (m, dim) float32 (normals None without input normals), descriptors /
    intensity (None when absent), global_indices (m,) int32, counts (m,) int32, result (the srrg2_voxel_result fields)."""
    P = _rows(points, F32)
    dim = P.shape[1] if dim is None else dim
    P = P[:, :dim]
    n = len(P)
    N = None if normals is None else _rows(normals, F32)[:, :dim]
    leaf = F64(F32(leaf_size))
    org = np.asarray(tuple(origin) + (0.0,) * (3 - len(origin)), F32)[:dim].astype(F64)
    e = exponents(leaf_size, n)[0]
    en = exponents(1.0, n)[0]
    part, cell = cells_of(P, leaf_size, org.astype(F32), dim)
    idx = np.flatnonzero(part)
    # the occupied cells, each with its members in ascending scene index
    members = {}
    for i in idx.tolist():
        members.setdefault(tuple(cell[i].tolist()), []).append(i)
    out_p, out_n, reps, counts = [], [], [], []
    occupied, most, with_normal = len(members), 0, 0
    for c, mem in sorted(members.items(), key=lambda kv: kv[1][0]):  # ascending representative
        k = len(mem)
        most = max(most, k)
        if k < min_points:
            continue
        rep = mem[0]
        p = P[rep].copy()
        nv = None if N is None else N[rep].copy()
        if mode == CENTROID:
            if k > 1:
                corner = org + np.asarray(c, F64) * leaf  # one multiply, one add
                q = np.rint((P[mem].astype(F64) - corner[None, :]) * F64(2.0) ** e).astype(I64)
                S = q.sum(0, dtype=I64)
                p = (corner + (S.astype(F64) * F64(2.0) ** -e) / F64(k)).astype(F32)
            if N is not None:
                M = N[mem]
                with np.errstate(invalid="ignore"):
                    ok = (np.abs(M) < F32(2.0)).all(1)  # (finite and below 2 in magnitude: NaN and inf compare false)
                v = np.rint(M[ok].astype(F64) * F64(2.0) ** en).astype(I64).sum(0, dtype=I64).astype(F64)
                ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) if dim == 3 else np.sqrt(v[0] * v[0] + v[1] * v[1])
                if ok.any() and ln > 0.0:
                    nv = (v / ln).astype(F32)
                else:
                    nv = np.full(dim, np.nan, F32)
        if nv is not None and not np.isnan(nv).any():
            with_normal += 1
        out_p.append(p)
        out_n.append(nv)
        reps.append(rep)
        counts.append(k)
    m = len(reps)
    g = np.asarray(reps, np.int32).reshape(m)
    res = {"num_points": n, "num_finite": int(part.sum()), "num_occupied": occupied, "num_voxels": m,
           "num_with_normal": with_normal, "max_points_per_voxel": most}
    return {"points": np.asarray(out_p, F32).reshape(m, dim),
            "normals": None if N is None else np.asarray(out_n, F32).reshape(m, dim),
            "descriptors": None if descriptors is None else np.ascontiguousarray(descriptors)[g],
            "intensity": None if intensity is None else np.ascontiguousarray(intensity, F32)[g],
            "global_indices": g, "counts": np.asarray(counts, np.int32).reshape(m), "result": res}
