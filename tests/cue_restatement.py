"""Independent numpy restatement of the gated nearest-neighbour and given-correspondence cue slices.

The finder transform, the query and a brute-force gated search in float32 in the documented operation order: they must give
the library's correspondences bit for bit.  Rows, chi and the robustifier in float32 as specified; H, b and the chi sums in
float64; the fixed-point exponent by DESIGN.md's formula, with the largest scaled term and the largest scaled sum of
magnitudes -- the range contract that the bit-for-bit tests cannot see, because the oracle and the device share the
fixed-point arithmetic and would be wrong together.  SE(3) quaternion and Euler, SE(2); point-to-point and point-to-plane.
Also the cases the CPU and GPU edge tests share.
"""
import math

import numpy as np

from projective_restatement import _inv, _robust, _se3, finder_transform as _finder_transform3
from projective_restatement import fixed_point_exponent, gauss_newton_step as _gauss_newton_step3
from srrg2_slam_interfaces_amd import _abi as abi

F = np.float32
SQRT3 = 1.7320508075688772
NN, PAIRS = abi.FINDER_NN_GATED, abi.FINDER_CORRESPONDENCES
P2P, PLANE = abi.SLICE_P2P, abi.SLICE_P2PLANE
QUAT, EULER, SE2 = abi.SE3_QUAT_RIGHT, abi.SE3_EULER_RIGHT, abi.SE2_RIGHT
KINDS = (QUAT, EULER, SE2)
ROBUST = (abi.ROBUST_NONE, abi.ROBUST_CLAMP, abi.ROBUST_SATURATED, abi.ROBUST_CAUCHY)
CORR = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])


def dim_of(kind):
    return 2 if kind == SE2 else 3


def identity(kind):
    return np.eye(3, dtype=F) if kind == SE2 else np.eye(4, dtype=F)[:3]


# ---- float32 transforms ---------------------------------------------------------------------------------------------
def se2_inverse32(A):
    """R^T, -R^T t (translation in float64, rounded once)"""
    A = np.asarray(A, F).reshape(3, 3)
    a = A.astype(np.float64)
    out = np.eye(3, dtype=F)
    out[0, 0], out[0, 1], out[1, 0], out[1, 1] = A[0, 0], A[1, 0], A[0, 1], A[1, 1]
    out[0, 2] = F(-(a[0, 0] * a[0, 2] + a[1, 0] * a[1, 2]))
    out[1, 2] = F(-(a[0, 1] * a[0, 2] + a[1, 1] * a[1, 2]))
    return out


def se2_compose32(A, B):
    """A*B, every entry a float64 dot product rounded once to float32"""
    a, b = np.asarray(A, F).reshape(3, 3).astype(np.float64), np.asarray(B, F).reshape(3, 3).astype(np.float64)
    out = np.eye(3, dtype=F)
    for i in range(2):
        for j in range(2):
            out[i, j] = F(a[i, 0] * b[0, j] + a[i, 1] * b[1, j])
        out[i, 2] = F((a[i, 0] * b[0, 2] + a[i, 1] * b[1, 2]) + a[i, 2])
    return out


def finder_transform(kind, X, sensor_in_robot=None):
    """T = fl32(robot_in_sensor * X), rows of [R | t]: (2, 3) for SE(2), (3, 4) for SE(3)"""
    if kind != SE2:
        return _finder_transform3(X, sensor_in_robot)
    S = np.eye(3, dtype=F) if sensor_in_robot is None else sensor_in_robot
    return se2_compose32(se2_inverse32(S), X)[:2]


def _xform(T, P):
    d = P.shape[1]
    if d == 2:
        return np.stack([(T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] for i in range(2)], 1)
    return np.stack([((T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2]) + T[i, 3] for i in range(3)], 1)


def _rot(T, P):
    d = P.shape[1]
    if d == 2:
        return np.stack([T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1] for i in range(2)], 1)
    return np.stack([(T[i, 0] * P[:, 0] + T[i, 1] * P[:, 1]) + T[i, 2] * P[:, 2] for i in range(3)], 1)


def _dot(a, b):
    d = a.shape[1]
    s = a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]
    return s if d == 2 else s + a[:, 2] * b[:, 2]


# ---- the gated nearest-neighbour finder, brute force ---------------------------------------------------------------
def dist2_matrix(fixed, q):
    """d2[i, j] of query i and fixed point j: dx = f - q, ((dx dx + dy dy) + dz dz), float32"""
    d = fixed[None, :, :] - q[:, None, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    return d2 if fixed.shape[1] == 2 else d2 + d[..., 2] * d[..., 2]


def associate(case, chunk=512):
    """(fixed_idx, moving_idx, response) ascending in moving_idx: over the finite fixed points with d2 <= gate2 the minimum
    of the key (d2, fixed_idx); non-finite points on either side never match; the optional normal gate after the search"""
    kind = case["kind"]
    T = finder_transform(kind, case["X"], case.get("S"))
    P, Fx = np.asarray(case["moving"], F), np.asarray(case["fixed"], F)
    g = F(case["gate"])
    gate2 = g * g
    fin_f = np.isfinite(Fx).all(1)
    cand = np.nonzero(fin_f)[0]
    mov = np.nonzero(np.isfinite(P).all(1))[0]
    fi, mi, resp = [], [], []
    with np.errstate(all="ignore"):
        for s in range(0, mov.size, chunk):
            m = mov[s:s + chunk]
            q = _xform(T, P[m])
            if cand.size == 0:
                continue
            d2 = dist2_matrix(Fx[cand], q)
            d2 = np.where(np.isnan(d2), F(np.inf), d2)
            best = d2.min(1)
            j = np.argmax(d2 == best[:, None], 1)  # first = smallest fixed index among the equal minima
            keep = best <= gate2
            fi.append(cand[j][keep]), mi.append(m[keep]), resp.append(best[keep])
    if not fi:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, F)
    fi, mi, resp = np.concatenate(fi), np.concatenate(mi), np.concatenate(resp)
    nf, nm = case.get("fixed_normals"), case.get("moving_normals")
    if case.get("normal_cos", -2.0) > -1.0 and nf is not None and nm is not None:
        with np.errstate(all="ignore"):
            dot = _dot(np.asarray(nf, F)[fi], _rot(T, np.asarray(nm, F)[mi]))
            keep = dot > F(case["normal_cos"])
        fi, mi, resp = fi[keep], mi[keep], resp[keep]
    return fi.astype(np.int32), mi.astype(np.int32), resp.astype(F)


def correspondences(case):
    if case["finder"] == PAIRS:
        c = case["corr"]
        return c["fixed_idx"].astype(np.int32), c["moving_idx"].astype(np.int32), c["response"].astype(F)
    return associate(case)


# ---- rows in float32, sums in float64 ----------------------------------------------------------------------------------
def factor_rows(case, fi, mi):
    """(J [C, rows, D], e [C, rows], chi [C]) in float32, in the specified operation order"""
    kind, plane = case["kind"], case["slice_kind"] == PLANE
    d = dim_of(kind)
    T = finder_transform(kind, case["X"], case.get("S"))
    p, f = np.asarray(case["moving"], F)[mi], np.asarray(case["fixed"], F)[fi]
    kk = F(2) if kind == QUAT else F(1)
    with np.errstate(all="ignore"):
        q = _xform(T, p)
        if plane:
            n = np.asarray(case["fixed_normals"], F)[fi]
            e = _dot(n, q - f)[:, None]
            # m = T_R^T n
            if d == 3:
                m = np.stack([(T[0, a] * n[:, 0] + T[1, a] * n[:, 1]) + T[2, a] * n[:, 2] for a in range(3)], 1)[:, None, :]
            else:
                m = np.stack([T[0, a] * n[:, 0] + T[1, a] * n[:, 1] for a in range(2)], 1)[:, None, :]
        else:
            e = q - f
            m = np.broadcast_to(T[None, :, :d], (len(fi), d, d)).astype(F)
        pp = p[:, None, :]
        if d == 3:
            J = np.concatenate([m, np.stack([kk * (pp[..., 1] * m[..., 2] - pp[..., 2] * m[..., 1]),
                                             kk * (pp[..., 2] * m[..., 0] - pp[..., 0] * m[..., 2]),
                                             kk * (pp[..., 0] * m[..., 1] - pp[..., 1] * m[..., 0])], 2)], 2)
        else:
            J = np.concatenate([m, (m[..., 1] * pp[..., 0] - m[..., 0] * pp[..., 1])[..., None]], 2)
        chi = e[:, 0] * e[:, 0]
        for r in range(1, e.shape[1]):
            chi = chi + e[:, r] * e[:, r]
    return J.astype(F), e.astype(F), chi.astype(F)


def _max_abs_finite(a, per_point):
    a = np.abs(np.asarray(a, F))
    if a.size == 0:
        return 0.0
    # points: the coordinates of the points with finite coordinates; normals: every finite component
    ok = np.broadcast_to(np.isfinite(a).all(1)[:, None], a.shape) if per_point else np.isfinite(a)
    return float(a[ok].max()) if ok.any() else 0.0


def slice_exponent(case):
    """k = min(62 - ceil(log2 N) - ceil(log2 B), 50 - ceil(log2 B), 50), B = rows max(J_b, e_b)^2.
    Gated slices: e_b = 1.01 m_b gate, N = moving points.  Given pairs: no gate, e_b = 1.01 m_b sqrt3 (sqrt3 P + |t| + F)
    with t the translation of the finder transform T the residual is formed with, N = pairs.  Returns (k, k_H)."""
    kind, plane = case["kind"], case["slice_kind"] == PLANE
    d = dim_of(kind)
    kk = 2.0 if kind == QUAT else 1.0
    pinf = _max_abs_finite(case["moving"], True)
    mb = (SQRT3 * _max_abs_finite(case["fixed_normals"], False)) * 1.01 if plane else 1.01
    pf = (2.0 * kk) * pinf
    jb = mb * (pf if pf > 1.0 else 1.0)
    eb = (mb * float(F(case["gate"]))) * 1.01
    n_terms = np.asarray(case["moving"]).shape[0]
    if case["finder"] == PAIRS:
        T = finder_transform(kind, case["X"], case.get("S"))
        tmax = float(np.abs(T[:, d].astype(np.float64)).max())
        finf = _max_abs_finite(case["fixed"], True)
        eb = ((mb * SQRT3) * ((SQRT3 * pinf + tmax) + finf)) * 1.01
        n_terms = max(len(case["corr"]), 1)
    mx = jb if jb > eb else eb
    rows = 1 if plane else d
    k = fixed_point_exponent(n_terms, rows * (mx * mx))
    # the H terms of a given-pair slice have their own exponent, from rows J_b^2: no gate bounds e_b there
    return k, (fixed_point_exponent(n_terms, rows * (jb * jb)) if case["finder"] == PAIRS else k)


def linearize(case, fi, mi):
    """float64 H, b, chi sums, counts, and the range of the fixed-point terms of one slice"""
    J32, e32, chi32 = factor_rows(case, fi, mi)
    supp = ~np.isfinite(chi32)
    w, kern = _robust(case["robust"], case["thr"], np.where(supp, F(0), chi32))
    ok = ~supp
    w64 = np.where(ok, w.astype(np.float64), 0.0)
    J = np.where(ok[:, None, None], J32.astype(np.float64), 0.0)
    e = np.where(ok[:, None], e32.astype(np.float64), 0.0)
    Hc = np.einsum("c,cra,crb->cab", w64, J, J)
    bc = np.einsum("c,cra,cr->ca", w64, J, e)
    D = J.shape[2]
    k, kh = slice_exponent(case)
    iu = np.triu_indices(D)
    chi_ok = np.where(ok, chi32.astype(np.float64), 0.0)
    terms = np.concatenate([np.abs(Hc[:, iu[0], iu[1]]) * 2.0 ** kh, np.abs(bc) * 2.0 ** k, chi_ok[:, None] * 2.0 ** k], 1)
    inl, out = ok & ~kern, ok & kern
    return {
        "H": Hc.sum(0), "b": bc.sum(0),
        "b_bound": float(np.abs(bc).sum(0).max()) if len(fi) else 0.0,  # sum of the term magnitudes, largest component
        "chi_inliers": float(chi_ok[inl].sum()), "chi_outliers": float(chi_ok[out].sum()),
        "num_inliers": int(inl.sum()), "num_outliers": int(out.sum()), "num_suppressed": int(supp.sum()),
        "num_correspondences": len(fi),
        "status": np.where(supp, abi.FACTOR_SUPPRESSED, np.where(kern, abi.FACTOR_KERNELIZED, abi.FACTOR_INLIER)),
        "k": k, "k_H": kh,
        "max_scaled_term": float(terms.max()) if terms.size else 0.0,
        # any order of the integer sums: bounded by the sum of the magnitudes
        "max_scaled_sum": float(terms.sum(0).max()) if terms.size else 0.0,
    }


def gauss_newton_step(kind, X, H, b):
    """X * v2t(-H^-1 b) in float64"""
    if kind != SE2:
        return _gauss_newton_step3(X, H, b, kind)
    dx = -np.linalg.solve(H, b)
    X = np.asarray(X, np.float64).reshape(3, 3)
    D = np.array([[math.cos(dx[2]), -math.sin(dx[2]), dx[0]], [math.sin(dx[2]), math.cos(dx[2]), dx[1]], [0, 0, 1]])
    return X @ D


def expected(case):
    fi, mi, resp = correspondences(case)
    return fi, mi, resp, linearize(case, fi, mi)


# ---- the cases the CPU and GPU edge tests share --------------------------------------------------------------------------
def se2(tx, ty, th):
    return np.array([[math.cos(th), -math.sin(th), tx], [math.sin(th), math.cos(th), ty], [0, 0, 1]])


def _pose(kind, t, angle):
    """a pose with translation t (first dim entries) and a rotation of `angle` radians scale"""
    if kind == SE2:
        return se2(t[0], t[1], angle)
    return _se3(np.asarray(t, np.float64), np.array([angle, -0.7 * angle, 0.5 * angle]))


def _inv_pose(kind, T):
    return np.linalg.inv(T) if kind == SE2 else _inv(T)


def _mul(kind, A, B):
    if kind == SE2:
        return A @ B
    out = np.zeros((3, 4))
    out[:, :3], out[:, 3] = A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3] + A[:, 3]
    return out


def _apply(kind, T, P):
    d = dim_of(kind)
    return P @ T[:d, :d].T + T[:d, d]


def _unit(rng, n, d):
    v = rng.normal(size=(n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(kind, slice_kind, finder, fixed, moving, X, fixed_normals=None, moving_normals=None, S=None, corr=None,
          robust=abi.ROBUST_NONE, thr=1.0, gate=1.0, normal_cos=-2.0):
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F)
    if slice_kind == PLANE:
        assert fixed_normals is not None
    c = dict(kind=kind, slice_kind=slice_kind, finder=finder, fixed=f32(fixed), moving=f32(moving), X=f32(X),
             fixed_normals=f32(fixed_normals), moving_normals=f32(moving_normals), S=f32(S), robust=robust, thr=thr,
             gate=float(gate), normal_cos=float(normal_cos))
    if finder == PAIRS:
        c["corr"] = np.ascontiguousarray(corr, dtype=CORR)
    return c


def _pairs(fixed_idx, moving_idx, rng=None):
    c = np.zeros(len(fixed_idx), CORR)
    c["fixed_idx"], c["moving_idx"] = fixed_idx, moving_idx
    c["response"] = 1.0 if rng is None else rng.uniform(0, 25, len(fixed_idx))
    return c


def sensor_offset(kind, L=0.3, angle=0.02):
    """sensor_in_robot translated by L along x (and a little along the other axes), rotated by `angle`"""
    t = [L, -0.2 * min(L, 1.0), 0.1 * min(L, 1.0)]
    return _pose(kind, t, angle)


def cloud_pair(kind, seed, n=600, scale=1.0, noise=0.01, outside=0.3, nonfinite=0, motion=(0.05, 0.03)):
    """fixed points uniform in [-scale, scale]^dim with unit normals; moving = a share of them (plus `outside` points that have
    no partner) seen from a frame X_gt away, with noise; `nonfinite` NaN / inf points on each side"""
    rng = np.random.default_rng(seed)
    d = dim_of(kind)
    Pf = rng.uniform(-scale, scale, (n, d))
    Nf = _unit(rng, n, d)
    sel = rng.permutation(n)[: max(int(n * (1.0 - outside)), 1)]
    extra = rng.uniform(-scale, scale, (n - sel.size, d)) + 3.0 * scale
    Q = np.concatenate([Pf[sel] + rng.normal(0, noise * scale, (sel.size, d)), extra])
    Nq = np.concatenate([Nf[sel], _unit(rng, extra.shape[0], d)])
    Nq[::5] = -Nq[::5]  # a fifth face away: the normal gate drops them
    X_gt = _pose(kind, rng.normal(0, motion[0], 3) * scale, float(rng.normal(0, motion[1])))
    Xi = _inv_pose(kind, X_gt)
    Pm, Nm = _apply(kind, Xi, Q), Nq @ Xi[:d, :d].T
    perm = rng.permutation(Pm.shape[0])
    Pm, Nm = Pm[perm], Nm[perm]
    partner = np.concatenate([sel, -np.ones(extra.shape[0], int)])[perm]  # the fixed point a moving point came from
    Pf, Nf, Pm, Nm = (a.astype(F) for a in (Pf, Nf, Pm, Nm))
    if nonfinite:
        bad = np.array([np.nan, np.inf, -np.inf], F)
        for A in (Pf, Pm):
            rows = rng.choice(A.shape[0], min(nonfinite, A.shape[0]), replace=False)
            A[rows, rng.integers(0, d, rows.size)] = rng.choice(bad, rows.size)
        Nf[rng.choice(n, min(nonfinite, n), replace=False)] = np.nan
    return dict(fixed=Pf, fixed_normals=Nf, moving=Pm, moving_normals=Nm, X_gt=X_gt, partner=partner)


def _robot_guess(kind, X_cam, S):
    """the robot-frame guess X with robot_in_sensor * X = X_cam"""
    return X_cam if S is None else _mul(kind, S, X_cam)


def random_case(seed):
    """one seeded configuration over kind, slice kind, finder, robustifier, normal gate, sensor offset, overlap, NaN / inf"""
    rng = np.random.default_rng(5000 + seed)
    kind, slice_kind = KINDS[seed % 3], (P2P, PLANE)[(seed // 3) % 2]
    finder = (NN, PAIRS)[(seed // 6) % 2]
    robust = ROBUST[(seed + seed // 12) % 4]
    d = cloud_pair(kind, 100 + seed, n=int(rng.integers(200, 1500)), scale=float(rng.choice([0.5, 2.0, 10.0])),
                   noise=0.01, outside=float(rng.choice([0.0, 0.3, 0.6])), nonfinite=int(rng.choice([0, 3])))
    scale = float(np.abs(d["fixed"][np.isfinite(d["fixed"])]).max())
    S = sensor_offset(kind, 0.3, 0.02 * (1 + seed % 3)) if rng.integers(0, 2) else None
    guess = _mul(kind, d["X_gt"], _pose(kind, [0.004 * scale, -0.003 * scale, 0.002 * scale], 0.003))
    X = _robot_guess(kind, guess, S)
    with_moving_normals = bool(rng.integers(0, 3) > 0)
    corr = None
    if finder == PAIRS:
        mi = np.nonzero(d["partner"] >= 0)[0]
        fi = d["partner"][mi].copy()
        wrong = rng.random(mi.size) < 0.2
        fi[wrong] = rng.integers(0, d["fixed"].shape[0], int(wrong.sum()))
        corr = _pairs(fi, mi, rng)
    chi = (0.01 * scale) ** 2 * (1 if slice_kind == PLANE else dim_of(kind))  # the noise's share of chi
    return _case(kind, slice_kind, finder, d["fixed"], d["moving"], X, d["fixed_normals"],
                 d["moving_normals"] if with_moving_normals else None, S, corr, robust, thr=2.0 * chi,
                 gate=float(rng.choice([0.03, 0.08, 0.25])) * scale,
                 normal_cos=float(rng.choice([-2.0, 0.5, 0.9])))


SIZES = (1, 63, 64, 65, 257)


def size_case(kind, n, finder):
    d = cloud_pair(kind, 300 + n, n=n, scale=1.0, noise=0.005, outside=0.0, motion=(0.01, 0.01))
    slice_kind = (P2P, PLANE)[n % 2]
    corr = _pairs(d["partner"], np.arange(n)) if finder == PAIRS else None
    return _case(kind, slice_kind, finder, d["fixed"], d["moving"], d["X_gt"], d["fixed_normals"], None, None, corr,
                 abi.ROBUST_CAUCHY, thr=1e-4, gate=0.2)


# ---- ties and the gate -----------------------------------------------------------------------------------------------
def lattice_case(kind, seed=0):
    """fixed points on the integer lattice in shuffled order; moving points at cell, face and edge centres: 2^dim, 4 and 2
    fixed points exactly equidistant (d2 = 0.75, 0.5, 0.25: exact in float32)"""
    rng = np.random.default_rng(seed)
    d = dim_of(kind)
    g = np.stack(np.meshgrid(*([np.arange(5.0)] * d), indexing="ij"), -1).reshape(-1, d)
    fixed = g[rng.permutation(g.shape[0])]
    cells = g[(g < 4).all(1)]
    offsets = np.stack(np.meshgrid(*([np.array([0.0, 0.5])] * d), indexing="ij"), -1).reshape(-1, d)[1:]
    moving = np.concatenate([cells + off for off in offsets])
    return _case(kind, P2P, NN, fixed, moving[rng.permutation(moving.shape[0])], identity(kind), gate=1.0)


def gate_edge_case(kind, gate=0.5):
    """moving point i sits off fixed point i along y by exactly the gate (even i: kept, d2 == gate2) or by one ulp more (odd i:
    dropped); the fixed points are 4 apart along x"""
    d = dim_of(kind)
    n = 40
    fixed, moving = np.zeros((n, d), F), np.zeros((n, d), F)
    fixed[:, 0] = moving[:, 0] = 4.0 * np.arange(n)
    g = F(gate)
    moving[0::2, 1] = g
    moving[1::2, 1] = np.nextafter(g, F(np.inf))
    return _case(kind, P2P, NN, fixed, moving, identity(kind), gate=gate)


def duplicate_fixed_case(kind):
    """every third fixed point appears twice: the smaller index of the two wins"""
    d = cloud_pair(kind, 77, n=300, scale=1.0, noise=0.005, outside=0.1)
    fixed = np.concatenate([d["fixed"], d["fixed"][::3]])
    normals = np.concatenate([d["fixed_normals"], d["fixed_normals"][::3]])
    perm = np.random.default_rng(78).permutation(fixed.shape[0])
    return _case(kind, PLANE, NN, fixed[perm], d["moving"], d["X_gt"], normals[perm], gate=0.2)


def duplicate_pairs_case(kind):
    d = cloud_pair(kind, 79, n=200, scale=1.0, noise=0.005, outside=0.0)
    corr = _pairs(d["partner"], np.arange(200))
    corr = np.concatenate([corr, corr, corr[:17]])
    return _case(kind, P2P, PAIRS, d["fixed"], d["moving"], d["X_gt"], corr=corr, robust=abi.ROBUST_CAUCHY, thr=1e-4)


TIE_CASES = {"lattice": lattice_case, "gate_edge": gate_edge_case, "duplicate_fixed": duplicate_fixed_case,
             "duplicate_pairs": duplicate_pairs_case}


# ---- range cases: ROBUST_NONE, the farthest admissible match enters at full weight -----------------------------------------
def magnitude_case(kind, slice_kind, pinf):
    """a cloud of magnitude P, gate 0.05 P, noise of the gate's order"""
    d = cloud_pair(kind, 400, n=300, scale=pinf, noise=0.02, outside=0.2, motion=(0.02, 0.01))
    return _case(kind, slice_kind, NN, d["fixed"], d["moving"], d["X_gt"], d["fixed_normals"], gate=0.05 * pinf)


def near_gate_case(kind, slice_kind, gate):
    """fixed points on a jittered lattice of spacing 4 gate; every moving point sits 0.9 ... 0.9999 gate off its partner"""
    rng = np.random.default_rng(410)
    d = dim_of(kind)
    side = 6 if d == 3 else 15
    g = np.stack(np.meshgrid(*([np.arange(float(side))] * d), indexing="ij"), -1).reshape(-1, d) - (side - 1) / 2.0
    fixed = (g * 4.0 + rng.uniform(-0.3, 0.3, g.shape)) * gate
    moving = fixed + _unit(rng, g.shape[0], d) * rng.uniform(0.9, 0.9999, (g.shape[0], 1)) * gate
    return _case(kind, slice_kind, NN, fixed, moving[rng.permutation(g.shape[0])], identity(kind), _unit(rng, g.shape[0], d),
                 gate=gate)


def normal_length_case(kind, length):
    d = cloud_pair(kind, 420, n=300, scale=1.0, noise=0.02, outside=0.2)
    return _case(kind, PLANE, NN, d["fixed"], d["moving"], d["X_gt"], d["fixed_normals"] * F(length), gate=0.1)


def opposite_corners_case(kind, slice_kind):
    """given pairs that join opposite corners of the two clouds"""
    rng = np.random.default_rng(430)
    d = dim_of(kind)
    fixed, moving = rng.uniform(-1, 1, (250, d)), rng.uniform(-1, 1, (250, d))
    corr = _pairs(np.argsort(-fixed.sum(1)), np.argsort(moving.sum(1)))
    return _case(kind, slice_kind, PAIRS, fixed, moving, identity(kind), _unit(rng, 250, d), corr=corr)


def far_estimate_case(kind, slice_kind, t, rotated=False):
    """given pairs of two overlapping clouds, linearised at an estimate that is a translation by t: every residual is ~t.
    rotated: the clouds' frames also differ by a small rotation, so the rows of T_R are no longer exact unit vectors"""
    d = cloud_pair(kind, 440, n=250, scale=1.0, noise=0.005, outside=0.0, motion=(0.05, 0.03) if rotated else (0.0, 0.0))
    X = _mul(kind, _pose(kind, [t, -0.5 * t, 0.25 * t], 0.0), d["X_gt"])
    return _case(kind, slice_kind, PAIRS, d["fixed"], d["moving"], X, d["fixed_normals"], corr=_pairs(d["partner"], np.arange(250)))


def sensor_offset_case(kind, slice_kind, L):
    """given identity pairs, X = I, sensor_in_robot translated by L along x: the residual is formed with T = S^-1 X, |t| = L"""
    rng = np.random.default_rng(450)
    d = dim_of(kind)
    P = rng.uniform(-1, 1, (200, d))
    S = _pose(kind, [L, 0.0, 0.0], 0.0)
    return _case(kind, slice_kind, PAIRS, P, P, identity(kind), _unit(rng, 200, d), S=S, corr=_pairs(np.arange(200), np.arange(200)))


def _range_cases():
    out = {}
    for z, pinf in enumerate((1e-3, 1.0, 1e3, 1e5)):
        for kind in KINDS:
            out["magnitude_%g_%d_p2p" % (pinf, kind)] = (magnitude_case, (kind, P2P, pinf))
        out["magnitude_%g_%d_plane" % (pinf, KINDS[z % 3])] = (magnitude_case, (KINDS[z % 3], PLANE, pinf))
    for z, gate in enumerate((1e-3, 0.05, 10.0, 1e3)):
        for sk, name in ((P2P, "p2p"), (PLANE, "plane")):
            kind = KINDS[(z + (sk == PLANE)) % 3]
            out["near_gate_%g_%d_%s" % (gate, kind, name)] = (near_gate_case, (kind, sk, gate))
    for length in (0.01, 100.0):
        for kind in KINDS:
            out["normal_length_%g_%d" % (length, kind)] = (normal_length_case, (kind, length))
    for kind in KINDS:
        out["opposite_corners_%d_p2p" % kind] = (opposite_corners_case, (kind, P2P))
    out["opposite_corners_%d_plane" % QUAT] = (opposite_corners_case, (QUAT, PLANE))
    for t in (30.0, 3e4):
        for kind in KINDS:
            out["far_estimate_%g_%d_p2p" % (t, kind)] = (far_estimate_case, (kind, P2P, t))
        out["far_estimate_%g_%d_plane" % (t, EULER)] = (far_estimate_case, (EULER, PLANE, t))
    for kind in KINDS:
        # with one exponent for H, b and chi the rows of a rotated T_R, the same in every point-to-point factor, rounded alike
        # in all of them on the coarse grid that the 3e4 residuals force: H was 7.6e-6 max|H| off, the step 4e-3
        out["far_rotated_estimate_%d_p2p" % kind] = (far_estimate_case, (kind, P2P, 3e4, True))
    for L in (0.5, 10.0, 1e3):
        for kind in KINDS:
            out["sensor_offset_%g_%d_p2p" % (L, kind)] = (sensor_offset_case, (kind, P2P, L))
        out["sensor_offset_%g_%d_plane" % (L, QUAT)] = (sensor_offset_case, (QUAT, PLANE, L))
        out["sensor_offset_%g_%d_plane" % (L, SE2)] = (sensor_offset_case, (SE2, PLANE, L))
    return out


RANGE_CASES = _range_cases()


def range_case(name):
    fn, args = RANGE_CASES[name]
    return fn(*args)
