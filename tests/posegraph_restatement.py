"""One Gauss-Newton step of the pose graph in plain float64 numpy, independent of the product and of the oracle.

The residual is the one of tests/golden/make_posegraph_golden.py / make_posegraph_golden_se2.py: e = t2v(Z^-1 Xi^-1 Xj), with
t2v = (t, quaternion vector) for SE3_QUAT_RIGHT and (tx, ty, atan2) for SE2_RIGHT.  Jacobians are central differences of that
residual under the right perturbation X <- X v2t(d), vectorised over the factors.  H and b carry the per-factor information
matrices, skip disabled factors, replace fixed poses by an identity row with a zero right-hand side and add `damping` to the free
diagonal (k_pg_vertices in csrc/posegraph.hip, oracle_posegraph_solve in oracle/o_posegraph.c).  H dx = -b is solved densely,
or block-banded when every factor joins poses at most BANDED_WIDTH apart (odometry chains with short closures, at any size).  Used by
tests/test_posegraph_restatement.py (CPU) and tests/test_gpu_posegraph_cycles.py."""
import numpy as np

from srrg2_slam_interfaces_amd import _abi as abi

EPS = 1e-6          # central-difference step (the golden generators' step)
DENSE_LIMIT = 4608  # unknowns of the largest dense solve
BANDED_WIDTH = 8    # graphs whose factors all join poses at most this far apart take the banded solve


def dim(kind):
    return 3 if kind == abi.SE2_RIGHT else 6


# ---- group operations, vectorised over leading axes ------------------------------------------------------------------------
def _mul(kind, A, B):
    if kind == abi.SE2_RIGHT:
        return A @ B
    C = np.empty(np.broadcast_shapes(A.shape, B.shape))
    C[..., :3] = A[..., :3] @ B[..., :3]
    C[..., 3] = np.einsum("...ab,...b->...a", A[..., :3], B[..., 3]) + A[..., 3]
    return C


def _inv(kind, A):
    if kind == abi.SE2_RIGHT:
        out = np.zeros_like(A)
        R = A[..., :2, :2]
        Rt = np.swapaxes(R, -1, -2)
        out[..., :2, :2] = Rt
        out[..., :2, 2] = -np.einsum("...ab,...b->...a", Rt, A[..., :2, 2])
        out[..., 2, 2] = 1.0
        return out
    out = np.empty_like(A)
    Rt = np.swapaxes(A[..., :3], -1, -2)
    out[..., :3] = Rt
    out[..., 3] = -np.einsum("...ab,...b->...a", Rt, A[..., 3])
    return out


def v2t(kind, d):
    """the increment's transform: se2(tx, ty, theta), or synthetic._quat_v2t (t, quaternion vector) for SE(3)"""
    d = np.asarray(d, np.float64)
    if kind == abi.SE2_RIGHT:
        c, s = np.cos(d[..., 2]), np.sin(d[..., 2])
        T = np.zeros(d.shape[:-1] + (3, 3))
        T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = c, -s, d[..., 0]
        T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = s, c, d[..., 1]
        T[..., 2, 2] = 1.0
        return T
    x, y, z = d[..., 3], d[..., 4], d[..., 5]
    w = np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y - z * z))
    T = np.zeros(d.shape[:-1] + (3, 4))
    T[..., 0, 0], T[..., 0, 1], T[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    T[..., 1, 0], T[..., 1, 1], T[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    T[..., 2, 0], T[..., 2, 1], T[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    T[..., 3] = d[..., :3]
    return T


def t2v(kind, T):
    if kind == abi.SE2_RIGHT:
        return np.stack([T[..., 0, 2], T[..., 1, 2], np.arctan2(T[..., 1, 0], T[..., 0, 0])], -1)
    R = T[..., :3]
    w = np.sqrt(np.maximum(1e-30, 1.0 + R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2])) / 2
    q = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / (4 * w[..., None])
    return np.concatenate([T[..., 3], q], -1)


def residual(kind, Xi, Xj, Z):
    return t2v(kind, _mul(kind, _inv(kind, Z), _mul(kind, _inv(kind, Xi), Xj)))


def box_plus(kind, X, dx):
    return _mul(kind, X, v2t(kind, dx))


# ---- the linear system ------------------------------------------------------------------------------------------------------
def linearise(kind, poses, ij, Z, omega=None, enabled=None):
    """per enabled factor: r (E, D), Ji, Jj (E, D, D) and Omega (E, D, D); plus the factor indices kept"""
    D = dim(kind)
    X = np.asarray(poses, np.float64)
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    keep = np.ones(ij.shape[0], bool) if enabled is None else np.asarray(enabled).astype(bool)
    idx = np.flatnonzero(keep)
    i, j = ij[idx, 0], ij[idx, 1]
    Zk = np.asarray(Z, np.float64)[idx]
    Om = np.tile(np.eye(D), (idx.size, 1, 1)) if omega is None else np.asarray(omega, np.float64).reshape(-1, D, D)[idx]
    Xi, Xj = X[i], X[j]
    r = residual(kind, Xi, Xj, Zk)
    Ji, Jj = np.empty((idx.size, D, D)), np.empty((idx.size, D, D))
    for a in range(D):
        d = np.zeros(D)
        d[a] = EPS
        Tp, Tm = v2t(kind, d), v2t(kind, -d)
        Ji[:, :, a] = (residual(kind, _mul(kind, Xi, Tp), Xj, Zk) - residual(kind, _mul(kind, Xi, Tm), Xj, Zk)) / (2 * EPS)
        Jj[:, :, a] = (residual(kind, Xi, _mul(kind, Xj, Tp), Zk) - residual(kind, Xi, _mul(kind, Xj, Tm), Zk)) / (2 * EPS)
    return r, Ji, Jj, Om, i, j


def chi(kind, poses, ij, Z, omega=None, enabled=None):
    """sum of e^T Omega e over the enabled factors"""
    r, _, _, Om, _, _ = linearise(kind, poses, ij, Z, omega, enabled)
    return float(np.einsum("ea,eab,eb->", r, Om, r))


def _blocks(kind, V, r, Ji, Jj, Om, i, j):
    tJiO = np.einsum("eba,ebc->eac", Ji, Om)  # Ji^T Omega
    tJjO = np.einsum("eba,ebc->eac", Jj, Om)
    Hii, Hjj, Hij = tJiO @ Ji, tJjO @ Jj, tJiO @ Jj
    D = dim(kind)
    b = np.zeros((V, D))
    np.add.at(b, i, np.einsum("eab,eb->ea", tJiO, r))
    np.add.at(b, j, np.einsum("eab,eb->ea", tJjO, r))
    return Hii, Hjj, Hij, b


def _solve_dense(V, D, Hii, Hjj, Hij, i, j, b, fixed, damping):
    H4 = np.zeros((V, V, D, D))
    np.add.at(H4, (i, i), Hii)
    np.add.at(H4, (j, j), Hjj)
    np.add.at(H4, (i, j), Hij)
    np.add.at(H4, (j, i), np.swapaxes(Hij, 1, 2))
    free = ~fixed
    H4[free, free] += damping * np.eye(D)
    H4[fixed, :] = 0.0
    H4[:, fixed] = 0.0
    H4[fixed, fixed] = np.eye(D)
    H = H4.transpose(0, 2, 1, 3).reshape(V * D, V * D)
    return np.linalg.solve(H, -b.reshape(-1)).reshape(V, D)


def _solve_banded(V, D, Hii, Hjj, Hij, i, j, b, fixed, damping):
    """H of block bandwidth w = max |i - j| (odometry chains with short closures): w consecutive poses form one super-node of
    w D unknowns, which makes H block-tridiagonal; a block LDL^T sweep over the super-nodes solves it"""
    w = int(np.max(np.abs(i - j)))
    Vs = -(-V // w)
    Hd = np.zeros((Vs * w, D, D))
    np.add.at(Hd, i, Hii)
    np.add.at(Hd, j, Hjj)
    Hd[:V][~fixed] += damping * np.eye(D)
    Hd[:V][fixed] = np.eye(D)
    Hd[V:] = np.eye(D)  # (padding of the last super-node)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    C = np.where((i < j)[:, None, None], Hij, np.swapaxes(Hij, 1, 2))  # H[lo, hi]
    live = ~(fixed[lo] | fixed[hi])
    lo, hi, C = lo[live], hi[live], C[live]
    S = np.zeros((Vs, w, w, D, D))  # super-diagonal blocks
    U = np.zeros((max(Vs - 1, 0), w, w, D, D))  # U[s] = H[super s, super s + 1]
    S[np.arange(Vs * w) // w, np.arange(Vs * w) % w, np.arange(Vs * w) % w] = Hd
    same = lo // w == hi // w
    np.add.at(S, (lo[same] // w, lo[same] % w, hi[same] % w), C[same])
    np.add.at(S, (lo[same] // w, hi[same] % w, lo[same] % w), np.swapaxes(C[same], 1, 2))
    nxt = ~same
    np.add.at(U, (lo[nxt] // w, lo[nxt] % w, hi[nxt] % w), C[nxt])
    n = w * D
    S = S.transpose(0, 1, 3, 2, 4).reshape(Vs, n, n)
    U = U.transpose(0, 1, 3, 2, 4).reshape(-1, n, n)
    rhs = np.zeros((Vs * w, D))
    rhs[:V] = -b
    rhs = rhs.reshape(Vs, n)
    y = np.empty_like(rhs)
    y[0] = rhs[0]
    for v in range(1, Vs):
        L = np.linalg.solve(S[v - 1], U[v - 1]).T  # U^T S^-1
        S[v] = S[v] - L @ U[v - 1]
        y[v] = rhs[v] - L @ y[v - 1]
    x = np.empty_like(rhs)
    x[Vs - 1] = np.linalg.solve(S[Vs - 1], y[Vs - 1])
    for v in range(Vs - 2, -1, -1):
        x[v] = np.linalg.solve(S[v], y[v] - U[v] @ x[v + 1])
    return x.reshape(Vs * w, D)[:V]


def gn_step(kind, poses, ij, Z, omega=None, enabled=None, fixed_mask=None, damping=0.0):
    """one Gauss-Newton step at `poses` (float32 or float64).  fixed_mask None = pose 0 fixed (the solvers' default).
    Returns (chi at the linearisation point, dx (V, D), poses after the step (float64))"""
    D = dim(kind)
    X = np.asarray(poses, np.float64)
    V = X.shape[0]
    fixed = np.zeros(V, bool)
    if fixed_mask is None:
        fixed[0] = True
    else:
        fixed[:] = np.asarray(fixed_mask).astype(bool)
    r, Ji, Jj, Om, i, j = linearise(kind, X, ij, Z, omega, enabled)
    chi0 = float(np.einsum("ea,eab,eb->", r, Om, r))
    Hii, Hjj, Hij, b = _blocks(kind, V, r, Ji, Jj, Om, i, j)
    b[fixed] = 0.0
    if V > 1 and i.size and np.max(np.abs(i - j)) <= BANDED_WIDTH:
        dx = _solve_banded(V, D, Hii, Hjj, Hij, i, j, b, fixed, float(damping))
    else:
        assert V * D <= DENSE_LIMIT, "dense restatement capped at %d unknowns (got %d)" % (DENSE_LIMIT, V * D)
        dx = _solve_dense(V, D, Hii, Hjj, Hij, i, j, b, fixed, float(damping))
    dx[fixed] = 0.0
    after = X.copy()
    free = ~fixed
    after[free] = box_plus(kind, X[free], dx[free])
    return chi0, dx, after


def gauss_newton(kind, poses, ij, Z, iterations, **kw):
    """`iterations` steps, each from the FLOAT32 poses of the previous one (as a solver that keeps float32 poses does).
    Returns (chi per iteration, poses after the last step as float32)"""
    P = np.asarray(poses, np.float32)
    chis = []
    for _ in range(iterations):
        c, _, after = gn_step(kind, P, ij, Z, **kw)
        chis.append(c)
        P = after.astype(np.float32)
    return chis, P
