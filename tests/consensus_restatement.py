"""Executable restatement of DESIGN.md section 4 "Consensus pose" (srrg2_consensus_compute), vectorised numpy.

Every operation is written out scalar-wise in the contract's order (no np.cross, no np.linalg, no matmul): numpy never fuses
a multiply and an add, so float64 / float32 arrays give the bits of the library (-ffp-contract=off).  ``consensus`` returns what
the C call returns per candidate, plus the per-hypothesis arrays the bit checks read.
"""
import numpy as np

F32, F64 = np.float32, np.float64
CORR_DTYPE = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
FOUND, NO_HYPOTHESIS, TOO_FEW_INLIERS = 0, 1, 2
HYP_SCORED, HYP_DEGENERATE, HYP_REJECTED = 0, 1, 2
DEFAULTS = dict(num_hypotheses=256, inlier_distance=0.05, min_sample_distance=0.1, min_inliers=0, seed=0, length_check=1)
_M = np.uint64(0xffffffff)


def mix32(x):
    """x: uint64 array holding uint32 values"""
    x = np.asarray(x, np.uint64) & _M
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M
    x = x ^ (x >> np.uint64(16))
    return x


def _ceil_log2(v):
    u = int(np.array([v], np.float64).view(np.uint64)[0])
    e = ((u >> 52) & 0x7ff) - 1023
    return e + 1 if (u & 0xfffffffffffff) else e


def fixed_point_exponent(n_terms, bound):
    """dm::fixed_point_exponent (csrc/det_math.h)"""
    n_terms = max(int(n_terms), 1)
    bound = bound if bound > 1e-30 else 1e-30
    lb = _ceil_log2(bound)
    k = min(62 - _ceil_log2(float(n_terms)) - lb, 50 - lb, 50)
    return max(k, -64)


def sample(seed, H, N, s):
    """idx (H, s) int64, ok (H,) bool"""
    h = np.arange(H, dtype=np.uint64)
    base = mix32(mix32(np.array([seed], np.uint64)) + h)
    idx = np.zeros((H, s), np.int64)
    ok = np.full(H, N >= s)
    for j in range(s):
        found = np.zeros(H, bool)
        for a in range(4):
            r = mix32(base + np.uint64(4 * j + a))
            i = ((r * np.uint64(max(N, 0))) >> np.uint64(32)).astype(np.int64)
            fresh = np.ones(H, bool)
            for e in range(j):
                fresh &= idx[:, e] != i
            take = fresh & ~found
            idx[take, j] = i[take]
            found |= take
        ok &= found
    return idx, ok


def _fin(x):
    return (x - x) == 0.0


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sq3(a):
    return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]


def _frame3(p0, p1, p2, msd2):
    """p*: (H, 3) float32 -> ok, e1, e2, e3, c, (d01, d02, d12)"""
    P0, P1, P2 = [[p[:, i].astype(F64) for i in range(3)] for p in (p0, p1, p2)]
    a = [P1[i] - P0[i] for i in range(3)]
    b = [P2[i] - P0[i] for i in range(3)]
    c = [P2[i] - P1[i] for i in range(3)]
    n = _cross(a, b)
    la, ln = _sq3(a), _sq3(n)
    ok = _fin(la) & _fin(ln) & ~(la < msd2) & ~(ln < msd2 * la)
    ra, rn = np.sqrt(la), np.sqrt(ln)
    e1 = [a[i] / ra for i in range(3)]
    e3 = [n[i] / rn for i in range(3)]
    e2 = _cross(e3, e1)
    cen = [((P0[i] + P1[i]) + P2[i]) / 3.0 for i in range(3)]
    return ok, e1, e2, e3, cen, (la, _sq3(b), _sq3(c))


def _length_differs(d2m, d2f, tau):
    return np.abs(np.sqrt(d2m) - np.sqrt(d2f)) > 2.0 * tau


def solve3(m, f, msd2, tau, length_check):
    """m, f: (H, 3 points, 3) float32 -> status (H,), X (H, 12) float64"""
    okm, m1, m2, m3, cm, dm = _frame3(m[:, 0], m[:, 1], m[:, 2], msd2)
    okf, f1, f2, f3, cf, df = _frame3(f[:, 0], f[:, 1], f[:, 2], msd2)
    H = len(m)
    status = np.full(H, HYP_SCORED)
    rej = np.zeros(H, bool)
    if length_check:
        for q in range(3):
            rej |= _length_differs(dm[q], df[q], tau)
    X = np.zeros((H, 12), F64)
    finite = np.ones(H, bool)
    for i in range(3):
        for j in range(3):
            X[:, i * 4 + j] = (f1[i] * m1[j] + f2[i] * m2[j]) + f3[i] * m3[j]
        X[:, i * 4 + 3] = cf[i] - ((X[:, i * 4 + 0] * cm[0] + X[:, i * 4 + 1] * cm[1]) + X[:, i * 4 + 2] * cm[2])
        for j in range(4):
            finite &= _fin(X[:, i * 4 + j])
    status[~finite] = HYP_DEGENERATE
    status[rej] = HYP_REJECTED
    status[~(okm & okf)] = HYP_DEGENERATE
    return status, X


def solve2(m, f, msd2, tau, length_check):
    """m, f: (H, 2 points, 2) float32 -> status (H,), X (H, 9) float64"""
    a0 = m[:, 1, 0].astype(F64) - m[:, 0, 0].astype(F64)
    a1 = m[:, 1, 1].astype(F64) - m[:, 0, 1].astype(F64)
    A0 = f[:, 1, 0].astype(F64) - f[:, 0, 0].astype(F64)
    A1 = f[:, 1, 1].astype(F64) - f[:, 0, 1].astype(F64)
    la, lA = a0 * a0 + a1 * a1, A0 * A0 + A1 * A1
    ok = _fin(la) & _fin(lA) & ~(la < msd2) & ~(lA < msd2)
    H = len(m)
    rej = _length_differs(la, lA, tau) if length_check else np.zeros(H, bool)
    den = np.sqrt(la) * np.sqrt(lA)
    c, s = (a0 * A0 + a1 * A1) / den, (a0 * A1 - a1 * A0) / den
    cm0 = (m[:, 0, 0].astype(F64) + m[:, 1, 0].astype(F64)) * 0.5
    cm1 = (m[:, 0, 1].astype(F64) + m[:, 1, 1].astype(F64)) * 0.5
    cf0 = (f[:, 0, 0].astype(F64) + f[:, 1, 0].astype(F64)) * 0.5
    cf1 = (f[:, 0, 1].astype(F64) + f[:, 1, 1].astype(F64)) * 0.5
    X = np.zeros((H, 9), F64)
    X[:, 0], X[:, 1], X[:, 3], X[:, 4] = c, -s, s, c
    X[:, 2] = cf0 - (X[:, 0] * cm0 + X[:, 1] * cm1)
    X[:, 5] = cf1 - (X[:, 3] * cm0 + X[:, 4] * cm1)
    X[:, 8] = 1.0
    finite = np.ones(H, bool)
    for i in range(6):
        finite &= _fin(X[:, i])
    status = np.full(H, HYP_SCORED)
    status[~finite] = HYP_DEGENERATE
    status[rej] = HYP_REJECTED
    status[~ok] = HYP_DEGENERATE
    return status, X


def gather_pairs(dim, fixed, moving, corr):
    """the candidate's pairs: pf, pm (N, dim) float32 (zeros where invalid), valid (N,) bool"""
    fixed, moving = np.asarray(fixed, F32), np.asarray(moving, F32)
    fixed = (fixed if fixed.ndim == 2 else fixed.reshape(-1, dim))[:, :dim]
    moving = (moving if moving.ndim == 2 else moving.reshape(-1, dim))[:, :dim]
    fi, mi = corr["fixed_idx"].astype(np.int64), corr["moving_idx"].astype(np.int64)
    valid = (fi >= 0) & (fi < len(fixed)) & (mi >= 0) & (mi < len(moving))
    N = len(corr)
    pf, pm = np.zeros((N, dim), F32), np.zeros((N, dim), F32)
    if valid.any():
        pf[valid] = fixed[fi[valid]]
        pm[valid] = moving[mi[valid]]
    with np.errstate(all="ignore"):
        valid &= np.isfinite(pf).all(1) & np.isfinite(pm).all(1)
    pf[~valid] = 0
    pm[~valid] = 0
    return pf, pm, valid


def errors(dim, X32, pm, pf):
    """e (S, N) float32 of the float32 poses X32 (S, 12 | 9) on the pairs"""
    x, y = pm[None, :, 0], pm[None, :, 1]
    if dim == 3:
        z = pm[None, :, 2]
        r = [(((X32[:, i * 4 + 0, None] * x + X32[:, i * 4 + 1, None] * y) + X32[:, i * 4 + 2, None] * z) + X32[:, i * 4 + 3, None])
             - pf[None, :, i] for i in range(3)]
        return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
    r = [((X32[:, i * 3 + 0, None] * x + X32[:, i * 3 + 1, None] * y) + X32[:, i * 3 + 2, None]) - pf[None, :, i] for i in range(2)]
    return r[0] * r[0] + r[1] * r[1]


def consensus_one(dim, fixed, moving, corr, **params):
    p = dict(DEFAULTS)
    p.update(params)
    H, s = int(p["num_hypotheses"]), (3 if dim == 3 else 2)
    tau32 = F32(p["inlier_distance"])
    tau = float(tau32)
    msd = float(F32(p["min_sample_distance"]))
    msd2 = msd * msd
    corr = np.asarray(corr, CORR_DTYPE)
    N = len(corr)
    pf, pm, valid = gather_pairs(dim, fixed, moving, corr)
    tsize = 12 if dim == 3 else 9
    with np.errstate(all="ignore"):
        idx, ok = sample(int(p["seed"]), H, N, s)
        if N > 0:
            ok &= valid[idx].all(1)
            m, f = pm[idx], pf[idx]
        else:
            m, f = np.zeros((H, s, dim), F32), np.zeros((H, s, dim), F32)
        status, X = (solve3 if dim == 3 else solve2)(m, f, msd2, tau, int(p["length_check"]))
        status[~ok] = HYP_DEGENERATE
        X32 = X.astype(F32)
        scored = np.flatnonzero(status == HYP_SCORED)
        k = fixed_point_exponent(N, tau * tau)
        counts, costs = np.zeros(H, np.int64), np.zeros(H, np.int64)
        inl = np.zeros((len(scored), N), bool)
        if len(scored) and N:
            e = errors(dim, X32[scored], pm, pf)
            inl = valid[None, :] & (e <= tau32 * tau32)
            term = np.trunc(e.astype(F64) * 2.0 ** k)
            costs[scored] = np.where(inl, term, 0.0).astype(np.int64).sum(1)
            counts[scored] = inl.sum(1)
    res = {"status": NO_HYPOTHESIS, "best_hypothesis": -1, "num_inliers": 0, "num_pairs": N, "num_valid_pairs": int(valid.sum()),
           "num_degenerate": int((status == HYP_DEGENERATE).sum()), "num_rejected": int((status == HYP_REJECTED).sum()),
           "num_scored": len(scored), "cost_exponent": k, "cost": 0, "moving_in_fixed": np.zeros(tsize, F32),
           "inliers": np.zeros(0, CORR_DTYPE), "flags": np.zeros(N, bool),
           "hyp_status": status, "hyp_idx": idx, "hyp_pose64": X, "hyp_pose32": X32, "hyp_count": counts, "hyp_cost": costs}
    if len(scored):
        order = np.lexsort((scored, costs[scored], -counts[scored]))
        b = int(order[0])
        h = int(scored[b])
        res.update(best_hypothesis=h, num_inliers=int(counts[h]), cost=int(costs[h]), moving_in_fixed=X32[h].copy(),
                   status=TOO_FEW_INLIERS if counts[h] < max(int(p["min_inliers"]), s) else FOUND)
        if res["status"] == FOUND:
            res["flags"] = inl[b].copy()
            res["inliers"] = corr[inl[b]].copy()
    res["moving_in_fixed"] = res["moving_in_fixed"].reshape(3, 4 if dim == 3 else 3)
    return res


def consensus(dim, fixed, movings, corrs, **params):
    """the batch: result k is consensus_one of candidate k alone (the candidate's index is not in the hash)"""
    return [consensus_one(dim, fixed, m, c, **params) for m, c in zip(movings, corrs)]
