"""The restatement of the consensus pose (tests/consensus_restatement.py) against a plain per-hypothesis, per-pair loop, its
invariants, and that every seeded case exercises what its name says.  Plus the planted-pose check against the oracle aligner: the
consensus pose and its inliers rescue a closure that the locked solve from the identity loses.  Needs no GPU and no library."""
import math

import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

F32 = np.float32
CASES = cc.small_cases()


@pytest.fixture(scope="module")
def restated():
    """every small case through the restatement, once"""
    return {name: cr.consensus(c["dim"], c["fixed"], c["movings"], c["corrs"], **c["params"]) for name, c in CASES.items()}


# ---- the plain loop: Python floats are IEEE doubles, np.float32 scalars float32; one operation per expression ----

def _mix32(x):
    x &= 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _sample(seed, h, N, s):
    if N < s:
        return None
    base = _mix32(_mix32(seed) + h)
    idx = []
    for j in range(s):
        for a in range(4):
            i = (_mix32(base + 4 * j + a) * N) >> 32
            if i not in idx:
                idx.append(i)
                break
        else:
            return None
    return idx


def _fin(x):
    return not (math.isnan(x) or math.isinf(x))


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else float("nan")


def _div(a, b):
    if b == 0:
        return float("nan") if (a == 0 or math.isnan(a)) else math.copysign(float("inf"), a) * math.copysign(1.0, b)
    return a / b


def _frame3(p):
    a = [float(p[1][i]) - float(p[0][i]) for i in range(3)]
    b = [float(p[2][i]) - float(p[0][i]) for i in range(3)]
    c = [float(p[2][i]) - float(p[1][i]) for i in range(3)]
    cross = lambda u, v: [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]  # noqa: E731
    sq = lambda u: (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]  # noqa: E731
    n = cross(a, b)
    la, ln = sq(a), sq(n)
    d = (la, sq(b), sq(c))
    return a, n, la, ln, d, cross


def _solve3(m, f, msd2, tau, length_check):
    fm, ff = _frame3(m), _frame3(f)
    for (_, _, la, ln, _, _) in (fm, ff):
        if not _fin(la) or not _fin(ln) or la < msd2 or ln < msd2 * la:
            return cr.HYP_DEGENERATE, None
    if length_check:
        for q in range(3):
            if abs(_sqrt(fm[4][q]) - _sqrt(ff[4][q])) > 2.0 * tau:
                return cr.HYP_REJECTED, None
    E, cen = [], []
    for (a, n, la, ln, _, cross), p in ((fm, m), (ff, f)):
        ra, rn = _sqrt(la), _sqrt(ln)
        e1, e3 = [_div(a[i], ra) for i in range(3)], [_div(n[i], rn) for i in range(3)]
        E.append((e1, cross(e3, e1), e3))
        cen.append([((float(p[0][i]) + float(p[1][i])) + float(p[2][i])) / 3.0 for i in range(3)])
    (m1, m2, m3), (f1, f2, f3) = E
    X = [0.0] * 12
    for i in range(3):
        for j in range(3):
            X[i * 4 + j] = (f1[i] * m1[j] + f2[i] * m2[j]) + f3[i] * m3[j]
        X[i * 4 + 3] = cen[1][i] - ((X[i * 4] * cen[0][0] + X[i * 4 + 1] * cen[0][1]) + X[i * 4 + 2] * cen[0][2])
    return (cr.HYP_SCORED if all(_fin(x) for x in X) else cr.HYP_DEGENERATE), X


def _solve2(m, f, msd2, tau, length_check):
    a0, a1 = float(m[1][0]) - float(m[0][0]), float(m[1][1]) - float(m[0][1])
    A0, A1 = float(f[1][0]) - float(f[0][0]), float(f[1][1]) - float(f[0][1])
    la, lA = a0 * a0 + a1 * a1, A0 * A0 + A1 * A1
    if not _fin(la) or not _fin(lA) or la < msd2 or lA < msd2:
        return cr.HYP_DEGENERATE, None
    if length_check and abs(_sqrt(la) - _sqrt(lA)) > 2.0 * tau:
        return cr.HYP_REJECTED, None
    den = _sqrt(la) * _sqrt(lA)
    c, s = _div(a0 * A0 + a1 * A1, den), _div(a0 * A1 - a1 * A0, den)
    cm = [(float(m[0][i]) + float(m[1][i])) * 0.5 for i in range(2)]
    cf = [(float(f[0][i]) + float(f[1][i])) * 0.5 for i in range(2)]
    X = [c, -s, cf[0] - (c * cm[0] + (-s) * cm[1]), s, c, cf[1] - (s * cm[0] + c * cm[1]), 0.0, 0.0, 1.0]
    return (cr.HYP_SCORED if all(_fin(x) for x in X[:6]) else cr.HYP_DEGENERATE), X


def plain_loop(dim, fixed, moving, corr, **params):
    p = dict(cr.DEFAULTS)
    p.update(params)
    s, H, N = (3 if dim == 3 else 2), p["num_hypotheses"], len(corr)
    tau32 = F32(p["inlier_distance"])
    tau, msd = float(tau32), float(F32(p["min_sample_distance"]))
    pairs = []
    for r in corr:
        fi, mi = int(r["fixed_idx"]), int(r["moving_idx"])
        ok = 0 <= fi < len(fixed) and 0 <= mi < len(moving)
        ok = ok and all(np.isfinite(fixed[fi][i]) and np.isfinite(moving[mi][i]) for i in range(dim))
        pairs.append((fixed[fi][:dim], moving[mi][:dim]) if ok else None)
    k = cr.fixed_point_exponent(N, tau * tau)
    counters = {cr.HYP_SCORED: 0, cr.HYP_DEGENERATE: 0, cr.HYP_REJECTED: 0}
    best = None
    for h in range(H):
        idx = _sample(p["seed"], h, N, s)
        if idx is None or any(pairs[i] is None for i in idx):
            counters[cr.HYP_DEGENERATE] += 1
            continue
        m, f = [pairs[i][1] for i in idx], [pairs[i][0] for i in idx]
        status, X = (_solve3 if dim == 3 else _solve2)(m, f, msd * msd, tau, p["length_check"])
        counters[status] += 1
        if status != cr.HYP_SCORED:
            continue
        X32 = [F32(x) for x in X]
        w = 4 if dim == 3 else 3
        count, cost, flags = 0, 0, []
        for pr in pairs:
            inl = False
            if pr is not None:
                fp, mp = pr
                e = F32(0)
                rs = []
                for i in range(dim):
                    acc = X32[i * w] * mp[0] + X32[i * w + 1] * mp[1]
                    if dim == 3:
                        acc = acc + X32[i * w + 2] * mp[2]
                    rs.append((acc + X32[i * w + dim]) - fp[i])
                e = rs[0] * rs[0] + rs[1] * rs[1]
                if dim == 3:
                    e = e + rs[2] * rs[2]
                inl = bool(e <= tau32 * tau32)
                if inl:
                    count += 1
                    cost += int(math.trunc(float(e) * 2.0 ** k))
            flags.append(inl)
        if best is None or (count, -cost) > (best[0], -best[1]):  # (ascending h: a tie keeps the earlier one)
            best = (count, cost, h, X32, flags)
    return counters, best, k


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_plain_loop(name, restated):
    c = CASES[name]
    with np.errstate(all="ignore"):
        for k, (m, corr) in enumerate(zip(c["movings"], c["corrs"])):
            counters, best, kexp = plain_loop(c["dim"], c["fixed"], m, corr, **c["params"])
            r = restated[name][k]
            assert (r["num_scored"], r["num_degenerate"], r["num_rejected"]) == (
                counters[cr.HYP_SCORED], counters[cr.HYP_DEGENERATE], counters[cr.HYP_REJECTED])
            assert r["cost_exponent"] == kexp
            if best is None:
                assert r["status"] == cr.NO_HYPOTHESIS and r["best_hypothesis"] == -1 and not r["moving_in_fixed"].any()
                continue
            count, cost, h, X32, flags = best
            assert (r["num_inliers"], r["cost"], r["best_hypothesis"]) == (count, cost, h)
            assert np.array(X32, F32).tobytes() == r["moving_in_fixed"].tobytes()
            if r["status"] == cr.FOUND:
                assert np.array_equal(r["flags"], np.array(flags, bool))


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(name, restated):
    c = CASES[name]
    H = c["params"].get("num_hypotheses", 256)
    s = 3 if c["dim"] == 3 else 2
    for k, r in enumerate(restated[name]):
        corr = c["corrs"][k]
        assert r["num_degenerate"] + r["num_rejected"] + r["num_scored"] == H
        assert r["num_pairs"] == len(corr)
        assert (r["status"] == cr.NO_HYPOTHESIS) == (r["num_scored"] == 0)
        if r["status"] == cr.FOUND:
            assert r["num_inliers"] >= max(c["params"].get("min_inliers", 0), s)
            # the inliers are the flagged records, in input order ...
            assert r["inliers"].tobytes() == corr[r["flags"]].tobytes() and len(r["inliers"]) == r["num_inliers"]
            # ... and the flags are a re-evaluation of the returned float32 pose
            pf, pm, valid = cr.gather_pairs(c["dim"], c["fixed"], c["movings"][k], corr)
            e = cr.errors(c["dim"], r["moving_in_fixed"].reshape(1, -1), pm, pf)[0]
            tau32 = F32(c["params"].get("inlier_distance", 0.05))
            assert np.array_equal(r["flags"], valid & (e <= tau32 * tau32))
        else:
            assert len(r["inliers"]) == 0 and not r["flags"].any()
        # a batch equals the K = 1 calls (the candidate's index is not in the hash)
        one = cr.consensus(c["dim"], c["fixed"], [c["movings"][k]], [corr], **c["params"])[0]
        for key in ("status", "best_hypothesis", "num_inliers", "cost", "num_scored"):
            assert one[key] == r[key]
        assert one["moving_in_fixed"].tobytes() == r["moving_in_fixed"].tobytes()


def test_cases_exercise_what_their_names_say(restated):
    R = {n: v[0] for n, v in restated.items()}
    for n in ("dim3_basic", "dim2_basic"):
        c = CASES[n]
        assert R[n]["status"] == cr.FOUND and R[n]["num_rejected"] > 0 and R[n]["num_scored"] > 0
        assert np.array_equal(R[n]["flags"], ~c["wrong"])  # exactly the true matches
        assert np.max(np.abs(R[n]["moving_in_fixed"] - c["X"][: R[n]["moving_in_fixed"].shape[0]])) < 5e-3
    for n in ("dim3_no_length_check", "dim2_no_length_check"):
        assert R[n]["num_rejected"] == 0 and R[n]["num_scored"] > R[n.replace("_no_length_check", "_basic")]["num_scored"]
    for n in ("dim3_degenerate_and_rejected", "dim2_degenerate_and_rejected", "collinear_close"):
        assert R[n]["num_degenerate"] > 0 and R[n]["num_scored"] > 0
    assert R["dim3_degenerate_and_rejected"]["num_rejected"] > 0 and R["dim2_degenerate_and_rejected"]["num_rejected"] > 0
    corr = CASES["dim3_degenerate_and_rejected"]["corrs"][0]  # invalid: the two records out of range, those of the NaN point
    invalid = (corr["moving_idx"] >= 60) | (corr["fixed_idx"] < 0) | (corr["moving_idx"] == 20)
    assert invalid.sum() >= 3 and R["dim3_degenerate_and_rejected"]["num_valid_pairs"] == 60 - invalid.sum()
    # collinear_close: the solver's own tests fire, not the sampler (every record is valid and N is large)
    assert R["collinear_close"]["num_valid_pairs"] == R["collinear_close"]["num_pairs"] and R["collinear_close"]["status"] == cr.FOUND
    for n in ("dim3_n_below_s", "dim3_n_one", "dim2_n_one"):
        assert R[n]["status"] == cr.NO_HYPOTHESIS and R[n]["num_degenerate"] == CASES[n]["params"]["num_hypotheses"]
    for n in ("dim3_n_equals_s", "dim2_n_equals_s"):  # collisions exhaust the four attempts for some hypotheses, not for all
        assert 0 < R[n]["num_degenerate"] < CASES[n]["params"]["num_hypotheses"] and R[n]["status"] == cr.FOUND
    for n in ("dim3_duplicates", "dim2_duplicates"):
        r = R[n]
        same = [h for h in range(len(r["hyp_status"])) if r["hyp_status"][h] == cr.HYP_SCORED
                and r["hyp_pose32"][h].tobytes() == r["hyp_pose32"][r["best_hypothesis"]].tobytes()]
        assert len(same) > 1 and r["best_hypothesis"] == min(same)
        assert all(r["hyp_count"][h] == r["num_inliers"] and r["hyp_cost"][h] == r["cost"] for h in same)
    for n in ("dim3_tau_exact", "dim2_tau_exact"):
        c, r = CASES[n], R[n]
        pf, pm, _ = cr.gather_pairs(c["dim"], c["fixed"], c["movings"][0], c["corrs"][0])
        e = cr.errors(c["dim"], r["moving_in_fixed"].reshape(1, -1), pm, pf)[0]
        assert e[cc.TAU_EXACT_ON] == F32(25) and r["flags"][cc.TAU_EXACT_ON]
        assert e[cc.TAU_EXACT_OFF] > F32(25) and not r["flags"][cc.TAU_EXACT_OFF]
    r = R["dim3_min_inliers_high"]
    assert r["status"] == cr.TOO_FEW_INLIERS and r["num_inliers"] > 3 and r["best_hypothesis"] >= 0 and r["moving_in_fixed"].any()
    for n in ("dim3_batch5", "dim2_batch5"):
        st = [x["status"] for x in restated[n]]
        assert st == [cr.FOUND, cr.NO_HYPOTHESIS, cr.FOUND, cr.NO_HYPOTHESIS, cr.FOUND]
        assert restated[n][1]["num_pairs"] == 0 and restated[n][3]["num_valid_pairs"] == 0 and restated[n][3]["num_pairs"] > 0


# ---- the planted pose, against the oracle only: 1 000 matches, 60 % wrong, 180 degrees of yaw, 2 mm noise ----

def _locked_solve(oracle, fixed, moving, corr, guess):
    al = oracle.OracleAligner(abi.SE3_QUAT_RIGHT)
    al.set_params(max_iterations=15)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind, c.finder = abi.SLICE_P2P, abi.FINDER_CORRESPONDENCES
    c.robustifier, c.robustifier_chi_threshold = abi.ROBUST_CAUCHY, 0.05
    si = al.add_slice(c)
    al.set_fixed(si, fixed, None)
    al.set_moving(si, moving, None)
    al.set_correspondences(si, corr)
    al.set_moving_in_fixed(guess)
    return al.compute(), al.moving_in_fixed()


def test_consensus_rescues_a_closure_met_from_the_opposite_direction(oracle):
    f, m, corr, X, wrong = cc.planted(100, 3, 1000, 0.6, yaw_deg=180.0, noise=0.002)
    status, _ = _locked_solve(oracle, f, m, corr, syn.identity(3))
    assert status != abi.SUCCESS  # the robustifier alone does not survive 60 % wrong matches from the identity
    r = cr.consensus_one(3, f, m, corr)
    assert r["status"] == cr.FOUND
    assert (r["flags"] & ~wrong).sum() == (~wrong).sum() and (r["flags"] & wrong).sum() <= 3
    status, T = _locked_solve(oracle, f, m, r["inliers"], r["moving_in_fixed"])
    assert status == abi.SUCCESS
    assert np.max(np.abs(T - X)) < 5e-3  # the tolerance of test_given_correspondences.py for the same noise
