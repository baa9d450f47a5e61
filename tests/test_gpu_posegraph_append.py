"""-m gpu: the appended-leaf elimination of the pose-graph solver (pg_classify_tail, k_pg_tail_down, k_pg_tail_up, k_pg_apply's
max |dx|; csrc/posegraph.hip) against float64.

The reference of every solve is posegraph_restatement.gauss_newton from the float32 poses read back from the handle right
before it, with the same iteration count, held with test_gpu_posegraph_cycles._check (chi rule, poses to 1e-5).  What
structure_info() must say after every solve is predicted by the restated classifier (posegraph_append_cases.StructureModel):
a tail that quietly rebuilds, or a refusal that quietly eliminates, fails.  The graphs and the restated elimination are
tests/posegraph_append_cases.py, proven on the CPU by tests/test_posegraph_append_cases.py."""
import numpy as np
import pytest

import posegraph_append_cases as AC
import posegraph_restatement as PR
import test_gpu_posegraph_cycles as C
from posegraph_append_cases import SE2, SE3

pytestmark = pytest.mark.gpu

KINDS = [SE2, SE3]
kinds = pytest.mark.parametrize("kind", KINDS, ids=["se2", "se3"])


def _params(s):
    return C._params(s.get("its", 1), pcg_max=s.get("pcg_max", 3000), tol=s.get("tol", 1e-10), damping=s.get("damping", 0.0))


class Run:
    """a handle, its host mirror and the model of its structure, driven through a case's operations"""

    def __init__(self, product, capfd, case, **tuning):
        self.kind, self.capfd = case["kind"], capfd
        b = case["base"]
        self.m = AC.Mirror(self.kind, b)
        self.V0 = len(self.m.poses)
        self.model = AC.StructureModel(tuning.get("keep_structure", 1))
        self.pg = product.PoseGraph(self.kind)
        self.pg.set_tuning(debug=1, **tuning)
        self.pg.set_graph(b["poses"], b["ij"], b["Z"], omega=b.get("omega"), fixed_mask=b.get("fixed_mask"), enabled=b.get("enabled"))
        self.solves = []  # (settings, stats, poses before, poses after, debug text, structure_info)

    def reference(self, before, s):
        g = self.m.graph(before)
        return PR.gauss_newton(self.kind, before, g["ij"], g["Z"], s.get("its", 1), omega=g["omega"], enabled=g["enabled"],
                               fixed_mask=g["fixed_mask"], damping=s.get("damping", 0.0))

    def rows(self):
        return self.m.enabled.count(True) * PR.dim(self.kind)

    def solve(self, s, check=True):
        before = self.pg.poses().copy()
        assert before.tobytes() == np.array(self.m.poses, np.float32).tobytes()
        self.capfd.readouterr()
        st = self.pg.solve(_params(s))
        err = self.capfd.readouterr().err
        after = self.pg.poses().copy()
        info = self.pg.structure_info()
        assert info == self.model.solve(self.m), (info, len(self.solves))
        assert self.pg.size() == self.m.size()
        self.m.poses = [p for p in after]
        self.solves.append((s, st, before, after, err, info))
        if s.get("pcg_max") == 0:  # (builds the hierarchy, moves nothing)
            assert after.tobytes() == before.tobytes() and all(x["solver_status"] == 0 for x in st)
        elif check:
            chis, ref_P = self.reference(before, s)
            C._check(st, after, chis, ref_P, self.rows())
            fixed = np.array(self.m.fixed, bool)
            assert np.array_equal(after[fixed], before[fixed])
        return st, before, after, err

    def play(self, ops, check=True):
        for op in ops:
            if op[0] == "solve":
                self.solve(op[1] if len(op) > 1 else {}, check)
            else:
                self.m.apply(op, self.pg, self.model)
        return self

    def close(self):
        self.pg.close()


def _split(ops):
    """the operations up to and including the first solve, and the rest"""
    k = next(n for n, op in enumerate(ops) if op[0] == "solve")
    return ops[:k + 1], ops[k + 1:]


# ---- a. exact tails: level 0 is the coarsest level and dense, one CG iteration is the direct solve ------------------------------
@kinds
@pytest.mark.parametrize("name", list(AC.EXACT_TAILS))
def test_exact_tail_one_cg_iteration(product, capfd, name, kind):
    """a wrong K, c, folded H_pp or b_p shows in the one step: nothing converges it away"""
    case = AC.exact_case(name, kind)
    build, rest = _split(case["ops"])
    run = Run(product, capfd, case).play(build)
    shape = C.Shape(PR.dim(kind), run.solves[0][4])
    assert shape.nl == 0 and shape.dense, shape
    run.play(rest)
    s, st, before, after, _, info = run.solves[-1]
    nt = len(run.m.poses) - run.V0
    assert info == (1, nt) and nt == len(AC.EXACT_TAILS[name][0](run.V0))
    assert len(st) == 1 and st[0]["pcg_iterations"] == 1, st
    step = np.abs(after.astype(np.float64) - before)
    assert np.max(step[run.V0:]) > 1e-2 and np.max(step[:run.V0]) > 1e-2  # leaves and base poses moved
    run.close()


# ---- a'. level 0 smoothed: the cycle reads the re-inverted smoother blocks of the parents ----------------------------------------
@kinds
@pytest.mark.parametrize("pcg_max", [1, 2])
def test_truncated_pcg_on_a_smoothed_level_sees_the_refreshed_smoother_blocks(product, capfd, kind, pcg_max):
    """Where level 0 is the coarsest level and dense its inverse is the whole cycle: the smoother blocks (Minv) that
    k_pg_tail_down re-inverts for every parent are never read, and a converged solve cannot see them anywhere.  On a level 0
    that is smoothed (a star above the dense limit) the cycle is block-Jacobi sweeps with exactly those blocks, and CG cut after
    1 or 2 iterations returns a fixed function of them: restated in float64 (posegraph_append_cases.truncated_pcg on the
    eliminated system; the cycle's operands rounded to float32 as k_mg_to_float does) and held at the suite's 1e-5.
    The truncated step is far from the exact one, so this is the preconditioner, not the solve."""
    case = AC.smoothed_case(kind, pcg_max)
    build, rest = _split(case["ops"])
    run = Run(product, capfd, case).play(build)
    shape = C.Shape(PR.dim(kind), run.solves[0][4])
    assert shape.nl == 0 and not shape.dense and shape.stalled, shape
    run.play(rest, check=False)
    s, st, before, after, _, info = run.solves[-1]
    assert info == (1, 32) and st[0]["pcg_iterations"] == pcg_max, (info, st)
    run.m.poses = [p for p in before]
    chi, dx, ref = AC.eliminated_step(kind, run.V0, run.m, solver=lambda H, rhs, D: AC.truncated_pcg(H, rhs, D, pcg_max))
    _, _, exact = AC.eliminated_step(kind, run.V0, run.m)
    gap = float(np.max(np.abs(ref - exact)))
    print("smoothed level 0, %d CG iterations: truncated vs exact step %.3g, product vs truncated %.3g" %
          (pcg_max, gap, float(np.max(np.abs(after - ref)))))
    assert gap > 1e-3
    C._check(st, after, [chi], ref.astype(np.float32), run.rows())
    run.close()


# ---- b. a multi-level base: a tail of 32 is eliminated, the 33rd leaf rebuilds -------------------------------------------------
MULTI = [(n, k) for n in AC.MULTILEVEL for k in KINDS]


@pytest.mark.parametrize("name,kind", MULTI, ids=["%s-%s" % (n, C._ids(k)) for n, k in MULTI])
def test_tail_of_32_then_33_on_a_multilevel_base(product, capfd, name, kind):
    case = AC.multilevel_case(name, kind)
    build, rest = _split(case["ops"])
    run = Run(product, capfd, case).play(build)
    shape = C.Shape(PR.dim(kind), run.solves[0][4])
    assert shape.nl >= 2, shape
    run.play(rest)
    (_, st32, b32, a32, _, i32), (_, st33, _, _, e33, i33) = run.solves[1:]
    assert i32 == (1, AC.TAIL_LIMIT) and i33 == (2, 0), (i32, i33)
    assert all(x["pcg_iterations"] < 3000 for x in st32 + st33)
    assert np.max(np.abs(a32.astype(np.float64) - b32)[run.V0:]) > 1e-2
    assert C.Shape(PR.dim(kind), e33).levels[0][0] == run.V0 + AC.TAIL_LIMIT + 1  # (the rebuilt hierarchy holds the leaves)
    run.close()


# ---- c. growing from the first pose, solved after every append --------------------------------------------------------------
@kinds
def test_growing_from_the_first_pose(product, capfd, kind):
    """one fixed pose and no factor, then 70 rounds of one pose + one factor + solve(max_iterations = 2): every solve against
    the float64 steps from the poses before it; leaves 1 .. 32, a rebuild at the 33rd append, 1 .. 32 again, a rebuild"""
    case = AC.growing_case(kind)
    first, rest = _split(case["ops"])
    run = Run(product, capfd, case).play(first)
    _, st, before, after, _, info = run.solves[0]
    assert len(st) == 1 and st[0]["solver_status"] == 0 and st[0]["chi"] == 0.0, st
    assert after.tobytes() == before.tobytes() and info == (1, 0)
    run.play(rest)
    seen = [x[5] for x in run.solves[1:]]
    expect = ([(1, t) for t in range(1, 33)] + [(2, 0)] + [(2, t) for t in range(1, 33)] + [(3, 0)] + [(3, t) for t in range(1, 5)])
    assert len(seen) == AC.GROW_ROUNDS and seen == expect, seen
    assert run.pg.size() == (AC.GROW_ROUNDS + 1, AC.GROW_ROUNDS, AC.GROW_ROUNDS)
    run.close()


# ---- d. what the classifier refuses -------------------------------------------------------------------------------------------
@kinds
@pytest.mark.parametrize("name", AC.REFUSALS)
def test_refused_tails_rebuild_and_solve_right(product, capfd, name, kind):
    case, tuning = AC.refusal_case(name, kind)
    run = Run(product, capfd, case, **tuning).play(case["ops"])
    infos = [x[5] for x in run.solves]
    if name == "closure_onto_tail":
        assert infos == [(1, 0), (1, 2), (2, 0)], infos
    else:
        assert infos == [(1, 0), (2, 0)], infos
    if name == "disabled_factor":  # the leaf without an enabled factor stays where it is
        assert run.solves[-1][3][-1].tobytes() == run.solves[-1][2][-1].tobytes()
    run.close()


@kinds
@pytest.mark.parametrize("how", ["disable", "remove"])
def test_tail_factor_dropped_after_elimination_undamped(product, capfd, how, kind):
    """the leaf has no factor left and a singular block: the same solver_status as a fresh handle given the same graph,
    and no other pose further than 1e-5 from that handle's"""
    case, orphan = AC.orphan_case(kind, how, 0.0)
    ops = case["ops"]
    run = Run(product, capfd, case).play(ops[:-1])
    assert [x[5] for x in run.solves] == [(1, 0), (1, 4)]
    s = ops[-1][1]
    st, before, after, _ = run.solve(s, check=False)
    assert run.solves[-1][5] == (2, 0)
    g = run.m.graph(before)
    one = product.PoseGraph(kind)
    one.set_graph(before, g["ij"], g["Z"], omega=g["omega"], fixed_mask=g["fixed_mask"], enabled=g["enabled"])
    st1 = one.solve(_params(s))
    assert [x["solver_status"] for x in st] == [x["solver_status"] for x in st1], (st, st1)
    others = np.arange(after.shape[0]) != orphan
    assert np.max(np.abs(after[others] - one.poses()[others])) <= 1e-5
    one.close()
    run.close()


@kinds
@pytest.mark.parametrize("how", ["disable", "remove"])
def test_tail_factor_dropped_after_elimination_damped(product, capfd, how, kind):
    case, orphan = AC.orphan_case(kind, how, 1e-3)
    run = Run(product, capfd, case).play(case["ops"])
    assert [x[5] for x in run.solves] == [(1, 0), (1, 4), (2, 0)]
    _, st, before, after, _, _ = run.solves[-1]
    assert after[orphan].tobytes() == before[orphan].tobytes()
    run.close()


# ---- e. the leaves' steps do not decide whether the hierarchy is kept -----------------------------------------------------------
@kinds
def test_leaf_steps_stay_out_of_the_kept_hierarchy_rule(product, capfd, kind):
    """a converged base and three leaves 0.45 m off: the max |dx| the solver reports (and compares with lag_below) is the
    base graph's"""
    case = AC.kept_case(kind)
    probe = product.PoseGraph(kind)
    lag = probe.tuning().lag_below
    probe.close()
    assert lag > 1e-3
    run = Run(product, capfd, case, lag_below=lag).play(case["ops"])
    (_, _, _, _, e0, i0), (s, st, before, after, err, info) = run.solves
    assert C.Shape(PR.dim(kind), e0).nl >= 2
    assert i0 == (1, 0) and info == (1, 3)
    steps = [(int(a), float(b)) for a, b in C._LAG.findall(err)]
    assert [k for k, _ in steps] == [0, 1], steps
    assert all(d < 1e-3 for _, d in steps), steps
    moved = np.abs(after.astype(np.float64) - before)
    assert np.max(moved[run.V0:]) > 0.2 and np.max(moved[:run.V0]) < 1e-3
    run.close()


# ---- f. evaluate_factors covers the appended factors -----------------------------------------------------------------------------
@kinds
def test_evaluate_factors_after_appends(product, capfd, kind):
    """chi of every factor id after a tail of 32 was solved, against e^T Omega e of the float64 restatement at the poses read
    back, at the tolerance of test_gpu_posegraph_robust.test_evaluate_factors_enabled_disabled_removed (1e-6 relative +
    1e-12).  This test is why k_pg_factor_eval forms its residual in double: with edge_linearize's float32 transforms the
    worst factor here was 2.15e-5 off in SE(2) (chi 3.53646e-4 for 3.53653e-4) and 2.03e-5 in SE(3)."""
    case = AC.multilevel_case("generator", kind)
    ops = case["ops"]
    second = [n for n, op in enumerate(ops) if op[0] == "solve"][1]
    run = Run(product, capfd, case).play(ops[:second + 1], check=False)
    assert run.solves[-1][5] == (1, AC.TAIL_LIMIT)
    P = run.pg.poses().copy()
    chi, w = run.pg.evaluate_factors()
    g = run.m.graph(P)
    E = g["ij"].shape[0]
    assert chi.shape == w.shape == (E,) and E == case["base"]["ij"].shape[0] + AC.TAIL_LIMIT
    r, _, _, Om, _, _ = PR.linearise(kind, P, g["ij"], g["Z"], g["omega"])
    ref = np.einsum("ea,eab,eb->e", r, Om, r)
    err = np.abs(chi - ref)
    worst = int(np.argmax(err - 1e-6 * ref))
    print("evaluate_factors after appends: worst factor %d of %d, chi %.6g, reference %.6g, difference %.3g (relative %.3g)" %
          (worst, E, chi[worst], ref[worst], err[worst], err[worst] / max(ref[worst], 1e-300)))
    assert np.array_equal(w, np.ones(E, np.float32))
    assert np.all(err <= 1e-6 * ref + 1e-12)
    run.close()
