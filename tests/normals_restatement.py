"""numpy restatement of srrg2_scene_estimate_normals: the executable form of DESIGN.md section 4 "Normals of unorganised
scenes".  Vectorised over points and pairs, but every value goes through exactly the operations of the contract, in its order,
so the device's normals, curvatures and counts equal these bit for bit.

How the candidate pairs are FOUND is not part of the contract (membership is decided by the float32 distance alone, and the
integer moment sums do not depend on order): here a hashed grid of cells a little larger than the radius, 3^dim cells per query.
"""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
SWEEPS = 6  # cyclic Jacobi sweeps over (0,1), (0,2), (1,2)
CLS_NORMAL, CLS_NOT_FINITE, CLS_TOO_FEW, CLS_DEGENERATE, CLS_TOO_CURVED = 0, 1, 2, 3, 4
PAIRS_PER_CHUNK = 1 << 21


def exponents(radius, n):
    """(e1, e2): first-moment terms are scaled by 2^e1, second-moment terms by 2^e2.  radius < 2^E (frexp), n <= 2^L:
    n terms of magnitude <= radius * (1 + 2^-22) (resp. its square) stay below 2^62, and one term below 2^51."""
    E = int(np.frexp(F32(radius))[1])
    L = 0 if n <= 1 else int(n - 1).bit_length()
    return min(61 - L - E, 50 - E), min(61 - L - 2 * E, 50 - 2 * E)


def second_moment_pairs(dim):
    return [(a, b) for a in range(dim) for b in range(a, dim)]  # xx xy xz yy yz zz / xx xy yy


def member_pairs(points, radius, dim):
    """yields (qi, cj, d): for chunks of queries, every (query, member) pair with d = p_c - p_q in float32; qi ascending."""
    P = np.ascontiguousarray(points, F32)[:, :dim]
    finite = np.flatnonzero(np.isfinite(P).all(1))
    if finite.size == 0:
        return
    Q = P[finite]
    r2 = F32(radius) * F32(radius)
    h = F64(F32(radius)) * (1.0 + 2.0 ** -16)
    cells = np.floor((Q.astype(F64) - Q.min(0).astype(F64)) / h).astype(I64)
    uc, inv = np.unique(cells, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(inv, kind="stable")
    start = np.searchsorted(inv[order], np.arange(len(uc) + 1))
    table = {tuple(c): k for k, c in enumerate(uc.tolist())}
    offsets = np.stack(np.meshgrid(*([[-1, 0, 1]] * dim), indexing="ij"), -1).reshape(-1, dim)
    # per query (in cell order) and offset: the candidate cell's range
    qcell = inv[order]
    for off in offsets.tolist():
        nb = np.array([table.get(tuple(np.add(c, off)), -1) for c in uc.tolist()], I64)
        cb = nb[qcell]
        has = cb >= 0
        qpos = np.flatnonzero(has)
        if qpos.size == 0:
            continue
        cstart = start[cb[qpos]]
        clen = start[cb[qpos] + 1] - cstart
        csum = np.cumsum(clen)
        lo = 0
        while lo < qpos.size:
            hi = int(np.searchsorted(csum, (csum[lo - 1] if lo else 0) + PAIRS_PER_CHUNK, side="right"))
            hi = max(hi, lo + 1)
            ln = clen[lo:hi]
            tot = int(ln.sum())
            rep = np.repeat(np.arange(lo, hi), ln)
            within = np.arange(tot) - np.repeat(np.cumsum(ln) - ln, ln)
            qloc = order[qpos[rep]]
            cloc = order[np.repeat(cstart[lo:hi], ln) + within]
            d = (Q[cloc] - Q[qloc]).astype(F32)
            if dim == 3:
                d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32) + d[:, 2] * d[:, 2]).astype(F32)
            else:
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F32)
            m = d2 <= r2
            qi, cj, d = finite[qloc[m]], finite[cloc[m]], d[m]
            o = np.argsort(qi, kind="stable")
            yield qi[o], cj[o], d[o]
            lo = hi


def moments(points, radius, dim, n=None):
    """neighbour counts and the fixed-point sums: count (n,), S1 (n, dim) int64, S2 (n, dim(dim+1)/2) int64, and (e1, e2)."""
    npts = len(points)
    e1, e2 = exponents(radius, npts if n is None else n)
    s1, s2 = F64(2.0) ** e1, F64(2.0) ** e2
    pairs = second_moment_pairs(dim)
    count = np.zeros(npts, I64)
    S1 = np.zeros((npts, dim), I64)
    S2 = np.zeros((npts, len(pairs)), I64)
    for qi, _, d in member_pairs(points, radius, dim):
        if qi.size == 0:
            continue
        d64 = d.astype(F64)
        t1 = np.rint(d64 * s1).astype(I64)
        t2 = np.stack([np.rint((d64[:, a] * d64[:, b]) * s2) for a, b in pairs], 1).astype(I64)
        first = np.flatnonzero(np.r_[True, qi[1:] != qi[:-1]])
        uq = qi[first]
        count[uq] += np.diff(np.r_[first, qi.size])
        S1[uq] += np.add.reduceat(t1, first, axis=0)
        S2[uq] += np.add.reduceat(t2, first, axis=0)
    return count, S1, S2, (e1, e2)


def covariance(count, S1, S2, e1, e2, dim):
    """C_ab = (S_ab 2^-e2) / k - ((S_a 2^-e1) / k) ((S_b 2^-e1) / k), float64, about the query point; (n, dim, dim)"""
    k = count.astype(F64)
    with np.errstate(all="ignore"):
        mean = (S1.astype(F64) * F64(2.0) ** -e1) / k[:, None]
        E = (S2.astype(F64) * F64(2.0) ** -e2) / k[:, None]
        C = np.zeros((len(count), dim, dim), F64)
        for c, (a, b) in enumerate(second_moment_pairs(dim)):
            C[:, a, b] = C[:, b, a] = E[:, c] - mean[:, a] * mean[:, b]
    return C


def _rotate(A, V, p, q, dim):
    apq = A[:, p, q].copy()
    go = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
        at = np.abs(theta) + np.sqrt(theta * theta + 1.0)
        t = np.where(theta >= 0.0, 1.0, -1.0) / at
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        tap = t * apq
        new = {}
        new["pp"] = A[:, p, p] - tap
        new["qq"] = A[:, q, q] + tap
        rs = [r for r in range(dim) if r not in (p, q)]
        for r in rs:
            a, b = A[:, r, p].copy(), A[:, r, q].copy()
            new[("a", r)] = (c * a - s * b, s * a + c * b)
        for k in range(dim):
            a, b = V[:, k, p].copy(), V[:, k, q].copy()
            new[("v", k)] = (c * a - s * b, s * a + c * b)
    A[go, p, p] = new["pp"][go]
    A[go, q, q] = new["qq"][go]
    A[go, p, q] = A[go, q, p] = 0.0
    for r in rs:
        x, y = new[("a", r)]
        A[go, r, p] = A[go, p, r] = x[go]
        A[go, r, q] = A[go, q, r] = y[go]
    for k in range(dim):
        x, y = new[("v", k)]
        V[go, k, p] = x[go]
        V[go, k, q] = y[go]


def jacobi(C, dim):
    """(diagonal (m, dim), V (m, dim, dim)) after the fixed sweeps; only + - * / sqrt, a rotation skipped on an exact 0"""
    A = np.array(C, F64, copy=True)
    V = np.tile(np.eye(dim, dtype=F64), (len(A), 1, 1))
    if dim == 2:
        _rotate(A, V, 0, 1, 2)  # (one rotation diagonalises a 2x2)
    else:
        for _ in range(SWEEPS):
            _rotate(A, V, 0, 1, 3)
            _rotate(A, V, 0, 2, 3)
            _rotate(A, V, 1, 2, 3)
    return np.stack([A[:, d, d] for d in range(dim)], 1), V


def smallest(diag, V, dim):
    """(lambda0, its eigenvector column, trace): the smallest diagonal entry, the lowest column on an exact tie"""
    m = len(diag)
    col = np.zeros(m, I64)
    l0 = diag[:, 0].copy()
    for d in range(1, dim):
        better = diag[:, d] < l0
        col[better] = d
        l0 = np.where(better, diag[:, d], l0)
    trace = (diag[:, 0] + diag[:, 1]) + diag[:, 2] if dim == 3 else diag[:, 0] + diag[:, 1]
    return l0, V[np.arange(m), :, col], trace


def estimate_normals(points, radius, dim=None, min_neighbours=None, max_curvature=1.0, viewpoint=(0.0, 0.0, 0.0), drop=True):
    """the whole call.  viewpoint None (or with a NaN in any component) = no viewpoint."""
    P = np.ascontiguousarray(points, F32)
    dim = P.shape[1] if dim is None else dim
    P = P[:, :dim]
    n = len(P)
    if min_neighbours is None:
        min_neighbours = 5 if dim == 3 else 3
    count, S1, S2, (e1, e2) = moments(P, radius, dim)
    finite = np.isfinite(P).all(1)
    cls = np.full(n, CLS_NOT_FINITE, I64)
    cls[finite] = CLS_TOO_FEW
    formed = finite & (count >= min_neighbours)
    cov = np.full((n, dim, dim), np.nan, F64)
    normals = np.full((n, dim), np.nan, F32)
    curvature = np.full(n, np.nan, F32)
    f = np.flatnonzero(formed)
    if f.size:
        C = covariance(count[f], S1[f], S2[f], e1, e2, dim)
        cov[f] = C
        diag, V = jacobi(C, dim)
        l0, vec, trace = smallest(diag, V, dim)
        ok = (trace > 0.0) & np.isfinite(trace)
        cls[f] = np.where(ok, CLS_TOO_CURVED, CLS_DEGENERATE)
        with np.errstate(all="ignore"):
            curv = (l0 / trace).astype(F32)
        curvature[f[ok]] = curv[ok]
        good = ok & ~(curv > F32(max_curvature))
        cls[f[good]] = CLS_NORMAL
        g = f[good]
        e = vec[good]
        if dim == 3:
            ln = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        else:
            ln = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        e = e / ln[:, None]
        vp = None if viewpoint is None else np.asarray(viewpoint, F32)
        if vp is not None and not np.isnan(vp).any():  # (any component given, also a third one for dim 2)
            w = vp[:dim].astype(F64)[None, :] - P[g].astype(F64)
            dot = (e[:, 0] * w[:, 0] + e[:, 1] * w[:, 1]) + e[:, 2] * w[:, 2] if dim == 3 else e[:, 0] * w[:, 0] + e[:, 1] * w[:, 1]
            flip = dot < 0.0
        else:
            big = e[:, 0].copy()
            for d in range(1, dim):
                big = np.where(np.abs(e[:, d]) > np.abs(big), e[:, d], big)
            flip = big < 0.0
        e[flip] = -e[flip]
        normals[g] = e.astype(F32)
    kept = np.flatnonzero(cls == CLS_NORMAL) if drop else np.arange(n)
    result = {"num_points": n, "num_finite": int(finite.sum()), "num_with_normal": int((cls == CLS_NORMAL).sum()),
              "num_too_few": int((cls == CLS_TOO_FEW).sum()), "num_degenerate": int((cls == CLS_DEGENERATE).sum()),
              "num_too_curved": int((cls == CLS_TOO_CURVED).sum()), "scene_size": int(len(kept))}
    return {"normals": normals, "curvature": curvature, "cls": cls, "cov": cov, "count": count, "result": result, "kept": kept,
            "points_out": P[kept], "normals_out": normals[kept], "S1": S1, "S2": S2, "exponents": (e1, e2)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the surfaces the tests sample (seeded; dim 3: plane, sphere, cylinder, two crossing planes; dim 2: line, circle, crossing lines)
def surface(kind, n, seed, radius, dim=3):
    rng = np.random.default_rng(seed)
    sigma = 0.01 * radius
    if dim == 3:
        if kind == "plane":
            uv = rng.uniform(-1, 1, (n, 2))
            P = np.stack([uv[:, 0], uv[:, 1], 0.3 * uv[:, 0] - 0.2 * uv[:, 1]], 1)
        elif kind == "sphere":
            v = rng.normal(size=(n, 3))
            P = v / np.linalg.norm(v, axis=1, keepdims=True)
        elif kind == "cylinder":
            a, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n)
            P = np.stack([0.7 * np.cos(a), 0.7 * np.sin(a), z], 1)
        elif kind == "crossing":
            uv = rng.uniform(-1, 1, (n, 2))
            P = np.stack([uv[:, 0], uv[:, 1], np.zeros(n)], 1)
            P[n // 2:] = P[n // 2:, [0, 2, 1]]
        else:
            raise ValueError(kind)
    else:
        if kind == "line":
            u = rng.uniform(-1, 1, n)
            P = np.stack([u, 0.4 * u + 0.1], 1)
        elif kind == "circle":
            a = rng.uniform(0, 2 * np.pi, n)
            P = np.stack([np.cos(a), np.sin(a)], 1)
        elif kind == "crossing":
            u = rng.uniform(-1, 1, n)
            P = np.stack([u, np.zeros(n)], 1)
            P[n // 2:] = P[n // 2:, ::-1]
        else:
            raise ValueError(kind)
    return (P + rng.normal(scale=sigma, size=P.shape)).astype(F32)
