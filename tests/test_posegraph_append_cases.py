"""The restatements of tests/posegraph_append_cases.py against the float64 Gauss-Newton step of posegraph_restatement, the
classifier's rule on a hand-written table, and the limits of the reference for every graph the GPU module grows (no GPU)."""
import numpy as np
import pytest

import posegraph_append_cases as AC
import posegraph_restatement as PR
from posegraph_append_cases import SE2, SE3

KINDS = [SE2, SE3]


def _ids(k):
    return "se2" if k == SE2 else "se3"


def _grown(case, upto_solve=None):
    """the Mirror of a case after its operations (up to, not including, solve number upto_solve); V0 = the base's size"""
    m = AC.Mirror(case["kind"], case["base"])
    V0, solves = len(m.poses), 0
    for op in case["ops"]:
        if op[0] == "solve":
            solves += 1
            if upto_solve is not None and solves == upto_solve:
                break
            continue
        m.apply(op)
    return m, V0


# ---- the elimination ---------------------------------------------------------------------------------------------------------
def _tail_case(kind, tail):
    base = AC.small_base(kind)
    V0 = base["poses"].shape[0]
    parents = {"chain32": [V0 - 1] + [V0 + t for t in range(31)], "star32": [9] * 32, "on_fixed": [0, V0, 0],
               "forest": AC._forest_parents(V0)}[tail]
    return dict(kind=kind, base=base, ops=AC.tail_ops(kind, base["poses"], parents, 3))


@pytest.mark.parametrize("damping", [0.0, 1e-3])
@pytest.mark.parametrize("tail", ["chain32", "star32", "on_fixed", "forest"])
@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_elimination_is_the_dense_step(kind, tail, damping):
    """reduced system solved densely + back-substitution = the step of the whole graph, to 1e-9 relative; the tails alternate
    the factor's orientation and carry non-diagonal information matrices"""
    case = _tail_case(kind, tail)
    m, V0 = _grown(case)
    g = m.graph()
    assert any(i > j for i, j in m.ij[-len(m.poses) + V0:]) and any(i < j for i, j in m.ij[-len(m.poses) + V0:])
    _, dx_ref, after_ref = PR.gn_step(kind, g["poses"], g["ij"], g["Z"], omega=g["omega"], fixed_mask=g["fixed_mask"], damping=damping)
    chi, dx, after = AC.eliminated_step(kind, V0, m, damping)
    scale = np.max(np.abs(dx_ref))
    assert scale > 1e-2
    assert np.max(np.abs(dx - dx_ref)) <= 1e-9 * scale
    assert np.max(np.abs(after - after_ref)) <= 1e-9
    assert abs(chi - PR.chi(kind, g["poses"], g["ij"], g["Z"], g["omega"])) <= 1e-12 * chi


@pytest.mark.parametrize("kind", KINDS, ids=_ids)
def test_elimination_restates_every_exact_gpu_case(kind):
    """the exact-tail cases of the GPU module: their inputs eliminate to the dense step too"""
    for name in AC.EXACT_TAILS:
        case = AC.exact_case(name, kind)
        damping = case["ops"][-1][1]["damping"]
        m, V0 = _grown(case)
        g = m.graph()
        _, dx_ref, _ = PR.gn_step(kind, g["poses"], g["ij"], g["Z"], omega=g["omega"], fixed_mask=g["fixed_mask"], damping=damping)
        _, dx, _ = AC.eliminated_step(kind, V0, m, damping)
        assert np.max(np.abs(dx - dx_ref)) <= 1e-9 * np.max(np.abs(dx_ref)), name


def test_truncated_pcg_converges_to_the_solve():
    """the restated preconditioned CG is CG: on a small SPD system it reaches the solution, and one iteration does not"""
    rng = np.random.default_rng(5)
    A = rng.normal(size=(12, 12))
    H = A @ A.T + 12 * np.eye(12)
    rhs = rng.normal(size=12)
    x = np.linalg.solve(H, rhs)
    assert np.max(np.abs(AC.truncated_pcg(H, rhs, 3, 12) - x)) <= 1e-6 * np.max(np.abs(x))
    assert np.max(np.abs(AC.truncated_pcg(H, rhs, 3, 1) - x)) > 1e-3 * np.max(np.abs(x))


# ---- the classifier ----------------------------------------------------------------------------------------------------------
def _table():
    """(name, expected, V0, E0, ij, fixed, enabled, removed, keep_structure): a hierarchy built for 4 poses / 3 factors"""
    base = [(0, 1), (1, 2), (2, 3)]
    F = lambda n, fixed=(): [v == 0 or v in fixed for v in range(n)]
    T = lambda n, off=(): [e not in off for e in range(n)]
    N = lambda n, on=(): [e in on for e in range(n)]
    rows = [
        ("one leaf", 1, base + [(3, 4)], F(5), T(4), N(4), 1),
        ("one leaf, leaf first", 1, base + [(4, 3)], F(5), T(4), N(4), 1),
        ("leaf on the fixed pose", 1, base + [(0, 4)], F(5), T(4), N(4), 1),
        ("chain of three", 3, base + [(3, 4), (5, 4), (5, 6)], F(7), T(6), N(6), 1),
        ("star of three", 3, base + [(1, 4), (5, 1), (1, 6)], F(7), T(6), N(6), 1),
        ("factors before their variables' order", 2, base + [(4, 5), (2, 4)], F(6), T(5), N(5), 1),
        ("chain of 32", 32, base + [(3 + t, 4 + t) for t in range(32)], F(36), T(35), N(35), 1),
        ("star of 32", 32, base + [(2, 4 + t) for t in range(32)], F(36), T(35), N(35), 1),
        ("chain of 33", None, base + [(3 + t, 4 + t) for t in range(33)], F(37), T(36), N(36), 1),
        ("star of 33", None, base + [(2, 4 + t) for t in range(33)], F(37), T(36), N(36), 1),
        ("nothing appended", None, base, F(4), T(3), N(3), 1),
        ("a new fixed variable", None, base + [(3, 4), (4, 5)], F(6, fixed=(5,)), T(5), N(5), 1),
        ("a new disabled factor", None, base + [(3, 4), (4, 5)], F(6), T(5, off=(4,)), N(5), 1),
        ("a new removed factor", None, base + [(3, 4), (4, 5)], F(6), T(5, off=(4,)), N(5, on=(4,)), 1),
        ("a new variable with two factors", None, base + [(3, 4), (1, 4)], F(5), T(5), N(5), 1),
        ("two factors on one new variable, none on the other", None, base + [(3, 4), (1, 4)], F(6), T(5), N(5), 1),
        ("a new variable without a factor", None, base + [(3, 4)], F(6), T(4), N(4), 1),
        ("a closure between old variables beside a leaf", None, base + [(3, 4), (0, 2)], F(5), T(5), N(5), 1),
        ("a closure between old variables instead of the leaf's factor", None, base + [(0, 2)], F(5), T(4), N(4), 1),
        ("a closure onto a tail variable", None, base + [(3, 4), (3, 5), (1, 5)], F(6), T(6), N(6), 1),
        ("a tail variable whose only factor goes to a later one", None, base + [(4, 5), (1, 5)], F(6), T(5), N(5), 1),
        ("keep_structure = 0", None, base + [(3, 4)], F(5), T(4), N(4), 0),
        ("an old factor disabled does not concern the tail's rule", 1, base + [(3, 4)], F(5), T(4, off=(1,)), N(4), 1),
    ]
    return [(n, x, 4, 3, ij, f, en, rm, k) for n, x, ij, f, en, rm, k in rows]


@pytest.mark.parametrize("row", _table(), ids=lambda r: r[0].replace(" ", "_"))
def test_classify_tail_table(row):
    name, expected, V0, E0, ij, fixed, enabled, removed, keep = row
    assert AC.classify_tail(V0, E0, ij, fixed, enabled, removed, keep) == expected, name


def test_structure_model_counts_cumulative_tails():
    """hier_V stays put between solves, so the tail accumulates: 32 leaves one by one are eliminated, the 33rd rebuilds"""
    m = AC.Mirror(SE2, dict(poses=np.tile(np.eye(3, dtype=np.float32), (2, 1, 1)), ij=[(0, 1)], Z=np.eye(3, dtype=np.float32)[None]))
    s = AC.StructureModel()
    assert s.solve(m) == (1, 0) and s.solve(m) == (1, 0)
    seen = []
    for k in range(34):
        m.apply(("var", np.eye(3), False), model=s)
        m.apply(("factor", 1 + k, 2 + k, np.eye(3), None, True), model=s)
        seen.append(s.solve(m))
    assert seen == [(1, t) for t in range(1, 33)] + [(2, 0), (2, 1)]
    assert s.solve(m) == (2, 1)  # (nothing appended: the tail stays eliminated)
    m.apply(("disable", 0), model=s)
    assert s.solve(m) == (3, 0)
    assert m.size() == (36, 35, 34)


# ---- the reference's limits --------------------------------------------------------------------------------------------------
def test_every_gpu_case_fits_the_float64_reference():
    """dense up to DENSE_LIMIT unknowns, or banded: no case of the GPU module can fall to a weaker reference.  Leaves start
    within 0.5 m of where their factors want them, so the float32-residual argument of _check holds"""
    cases = AC.all_cases()
    assert len(cases) == 2 * (len(AC.EXACT_TAILS) + 2 + len(AC.MULTILEVEL) + 1 + len(AC.REFUSALS) + 4 + 1)
    with_information = 0
    for name, case in cases:
        kind = case["kind"]
        m = AC.Mirror(kind, case["base"])
        solves = 0
        for op in case["ops"]:
            if op[0] != "solve":
                m.apply(op)
                continue
            solves += 1
            assert AC.reference_fits(kind, m), (name, len(m.poses))
            g = m.graph()
            r = PR.linearise(kind, g["poses"], g["ij"], g["Z"], g["omega"], g["enabled"])[0]
            new = np.array([max(e) >= case["base"]["poses"].shape[0] for e, en in zip(m.ij, m.enabled) if en], bool)
            if new.any():
                assert np.max(np.linalg.norm(r[new][:, :2 if kind == SE2 else 3], axis=1)) <= 0.5, name
        assert solves >= 1, name
        E0 = case["base"]["ij"].shape[0]
        with_information += any(np.abs(o - np.diag(np.diag(o))).max() > 0.05 for o in m.omega[E0:])
    assert 2 * with_information >= len(cases)
