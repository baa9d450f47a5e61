"""Appended-leaf elimination of the pose-graph solver (csrc/posegraph.hip: pg_classify_tail, k_pg_tail_down, k_pg_tail_up),
restated without a GPU, and the graphs tests/test_gpu_posegraph_append.py grows.

* `classify_tail`: the classifier's rule (the comment above pg_classify_tail, DESIGN.md "Appended leaves are eliminated, not
  rebuilt"); `StructureModel` follows a handle's lifecycle with it and says what structure_info() must report after a solve.
* `eliminate`: the Schur complement of the tail in float64 numpy on the blocks of posegraph_restatement (`K = S^-1 H_vp`,
  `c = S^-1 b_v`, `H_pp -= H_pv K`, `b_p -= H_pv c` children first; `dx_v = -(c + K dx_p)` parents first).
* `truncated_pcg`: k iterations of CG preconditioned by the cycle of a hierarchy whose level 0 is the coarsest and too large
  for the dense inverse (damped block-Jacobi: one sweep and three residual corrections on float32 copies of the blocks).
* A case is a base graph (the dicts of test_gpu_posegraph_cycles) plus append operations ("var", pose, fixed),
  ("factor", i, j, Z, omega, enabled), ("solve"[, settings]), ("disable", id), ("remove", id); `Mirror` keeps the host copy.

tests/test_posegraph_append_cases.py proves the restatements against posegraph_restatement.gn_step on the CPU."""
import numpy as np

import posegraph_restatement as PR
from test_gpu_posegraph_cycles import SE2, SE3, chain, generator, star

KINDS = [SE2, SE3]
TAIL_LIMIT = 32   # leaves pg_classify_tail accepts behind one hierarchy
MG_OMEGA = 0.8    # damping of the block-Jacobi smoother (srrg2_posegraph_default_tuning)
SMOOTHED_CORRECTIONS = 3  # residual corrections of a smoothed coarsest level (k_mg_coarse_cycle)


# ---- the classifier ----------------------------------------------------------------------------------------------------------
def classify_tail(V0, E0, ij, fixed, enabled, removed, keep_structure=1):
    """Variables V0.. and factors E0.. were appended behind a hierarchy built for (V0, E0).  Returns the number of leaves the
    solve eliminates, or None when it must rebuild.  A forest of leaves: between 1 and TAIL_LIMIT new variables, none fixed;
    as many new factors, all enabled and in the graph; the higher endpoint of every new factor is a new variable, and no
    new variable is the higher endpoint of two (so every new variable has exactly one factor to a variable below it)."""
    if not keep_structure:
        return None
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    nt = len(fixed) - V0
    if not 0 < nt <= TAIL_LIMIT or ij.shape[0] - E0 != nt:
        return None
    children = set()
    for e in range(E0, ij.shape[0]):
        if not enabled[e] or removed[e]:
            return None
        child = int(max(ij[e]))
        if child < V0 or child in children:
            return None
        children.add(child)
    if any(fixed[v] for v in range(V0, len(fixed))):
        return None
    return nt


class StructureModel:
    """(hierarchy builds, eliminated leaves) a handle must report after each solve: appends are classified at the next solve
    against the graph the hierarchy was built for; a changed flag, or a tail the classifier refuses, rebuilds"""

    def __init__(self, keep_structure=1):
        self.keep, self.builds, self.leaves = keep_structure, 0, 0
        self.dirty, self.pending, self.V0, self.E0 = True, False, 0, 0

    def appended(self):
        self.pending = True

    def flag_changed(self):
        self.dirty = True

    def solve(self, m):
        if not self.dirty and self.pending:
            self.pending = False
            nt = classify_tail(self.V0, self.E0, m.ij, m.fixed, m.enabled, m.removed, self.keep)
            if nt is None:
                self.dirty = True
            else:
                self.leaves = nt
        if self.dirty:
            self.builds, self.leaves, self.V0, self.E0 = self.builds + 1, 0, len(m.fixed), len(m.ij)
            self.dirty = self.pending = False
        return self.builds, self.leaves


# ---- the elimination ---------------------------------------------------------------------------------------------------------
def eliminate(kind, V0, V, Hii, Hjj, Hij, i, j, b, fixed, damping=0.0):
    """The tail V0 .. V-1 (each variable with one factor, to a variable of lower index) folded into the first V0 variables.
    Hii, Hjj, Hij, b: posegraph_restatement._blocks of the factors (i, j).  Returns (H, rhs, back): the reduced system H dx0 = rhs
    as a dense (V0 D)^2 matrix with identity rows for fixed poses, and back(dx0 (V0, D)) -> dx (V, D)."""
    D = PR.dim(kind)
    fixed = np.asarray(fixed, bool)
    Hd = np.zeros((V, D, D))
    np.add.at(Hd, i, Hii)
    np.add.at(Hd, j, Hjj)
    Hd[~fixed] += damping * np.eye(D)
    Hd[fixed] = np.eye(D)
    b = np.array(b, np.float64)
    b[fixed] = 0.0
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    tail = np.flatnonzero(hi >= V0)
    K, c, parent = {}, {}, {}
    for e in tail[np.argsort(-hi[tail], kind="stable")]:  # children first: a child's index is above its parent's
        v, p = int(hi[e]), int(lo[e])
        assert v not in K and not fixed[v], "not a forest of free leaves"
        Hvp = Hij[e].T if v == j[e] else Hij[e]  # (Hij is the block (i, j))
        K[v], c[v], parent[v] = np.linalg.solve(Hd[v], Hvp), np.linalg.solve(Hd[v], b[v]), p
        if not fixed[p]:
            Hd[p] -= Hvp.T @ K[v]
            b[p] -= Hvp.T @ c[v]
    assert len(K) == V - V0, "a tail variable without a factor"
    core = np.flatnonzero(hi < V0)
    H4 = np.zeros((V0, V0, D, D))
    H4[np.arange(V0), np.arange(V0)] = Hd[:V0]
    np.add.at(H4, (i[core], j[core]), Hij[core])
    np.add.at(H4, (j[core], i[core]), np.swapaxes(Hij[core], 1, 2))
    f0 = fixed[:V0]
    H4[f0, :] = 0.0
    H4[:, f0] = 0.0
    H4[f0, f0] = np.eye(D)
    H = H4.transpose(0, 2, 1, 3).reshape(V0 * D, V0 * D)

    def back(dx0):
        dx = np.zeros((V, D))
        dx[:V0] = dx0
        dx[:V0][f0] = 0.0
        for v in range(V0, V):  # parents first
            p = parent[v]
            dx[v] = -(c[v] + (0.0 if fixed[p] else K[v] @ dx[p]))
        return dx

    return H, -b[:V0].reshape(-1), back


def eliminated_step(kind, V0, m, damping=0.0, solver=None):
    """one Gauss-Newton step of Mirror m through the elimination: (chi, dx (V, D), poses after).  solver(H, rhs, D) -> dx0
    (default: the dense solve)"""
    D = PR.dim(kind)
    g = m.graph()
    X = np.asarray(g["poses"], np.float64)
    V = X.shape[0]
    fixed = g["fixed_mask"].astype(bool)
    r, Ji, Jj, Om, i, j = PR.linearise(kind, X, g["ij"], g["Z"], g["omega"], g["enabled"])
    chi0 = float(np.einsum("ea,eab,eb->", r, Om, r))
    Hii, Hjj, Hij, b = PR._blocks(kind, V, r, Ji, Jj, Om, i, j)
    H, rhs, back = eliminate(kind, V0, V, Hii, Hjj, Hij, i, j, b, fixed, damping)
    dx0 = np.linalg.solve(H, rhs) if solver is None else solver(H, rhs, D)
    dx = back(dx0.reshape(V0, D))
    after = X.copy()
    after[~fixed] = PR.box_plus(kind, X[~fixed], dx[~fixed])
    return chi0, dx, after


def truncated_pcg(H, rhs, D, iterations, omega=MG_OMEGA):
    """`iterations` of CG on H x = rhs from x = 0, preconditioned by the cycle of a one-level hierarchy whose level is
    smoothed, not inverted: x = w Dinv r, then three times x += w Dinv (r - H x), on the float32 copies of H's blocks and of
    the inverted diagonal blocks that the cycle reads (k_mg_to_float); CG's own products are float64"""
    n = H.shape[0]
    Hf = H.astype(np.float32).astype(np.float64)
    Dinv = np.zeros_like(H)
    for v in range(n // D):
        s = slice(v * D, (v + 1) * D)
        Dinv[s, s] = np.linalg.inv(H[s, s])
    Dinv = Dinv.astype(np.float32).astype(np.float64)

    def cycle(r):
        x = omega * (Dinv @ r)
        for _ in range(SMOOTHED_CORRECTIONS):
            x = x + omega * (Dinv @ (r - Hf @ x))
        return x

    x = np.zeros(n)
    r = np.array(rhs, np.float64)
    z = cycle(r)
    p, rz = z.copy(), float(r @ z)
    for _ in range(iterations):
        Ap = H @ p
        pAp = float(p @ Ap)
        alpha = rz / pAp if pAp > 0.0 else 0.0
        x = x + alpha * p
        r = r - alpha * Ap
        z = cycle(r)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x


# ---- the host copy of a graph that grows -------------------------------------------------------------------------------------
class Mirror:
    def __init__(self, kind, base):
        self.kind, D = kind, PR.dim(kind)
        P = np.asarray(base["poses"], np.float32)
        ij = np.asarray(base["ij"], np.int32).reshape(-1, 2)
        E = ij.shape[0]
        self.tshape = P.shape[1:]
        self.poses = [p for p in P]
        self.ij = [tuple(int(a) for a in e) for e in ij]
        self.Z = [z for z in np.asarray(base["Z"], np.float32).reshape((E,) + self.tshape)]
        om = base.get("omega")
        self.omega = [np.eye(D, dtype=np.float32)] * E if om is None else [o for o in np.asarray(om, np.float32).reshape(E, D, D)]
        fm = base.get("fixed_mask")
        self.fixed = [v == 0 for v in range(P.shape[0])] if fm is None else [bool(f) for f in fm]
        en = base.get("enabled")
        self.enabled = [True] * E if en is None else [bool(e) for e in en]
        self.removed = [False] * E

    def apply(self, op, pg=None, model=None):
        """one append operation on the mirror and, when given, on a PoseGraph handle and a StructureModel"""
        D = PR.dim(self.kind)
        if op[0] == "var":
            self.poses.append(np.asarray(op[1], np.float32))
            self.fixed.append(bool(op[2]))
            if pg is not None:
                assert pg.add_variable(op[1], fixed=bool(op[2])) == len(self.poses) - 1
            if model is not None:
                model.appended()
        elif op[0] == "factor":
            _, i, j, Z, om, en = op
            self.ij.append((int(i), int(j)))
            self.Z.append(np.asarray(Z, np.float32))
            self.omega.append(np.eye(D, dtype=np.float32) if om is None else np.asarray(om, np.float32))
            self.enabled.append(bool(en))
            self.removed.append(False)
            if pg is not None:
                assert pg.add_factor(int(i), int(j), Z, information=om, enabled=bool(en)) == len(self.ij) - 1
            if model is not None:
                model.appended()
        elif op[0] == "disable":
            if model is not None and self.enabled[op[1]]:
                model.flag_changed()
            self.enabled[op[1]] = False
            if pg is not None:
                pg.set_factor_enabled(op[1], False)
        elif op[0] == "remove":
            if model is not None and self.enabled[op[1]]:
                model.flag_changed()
            self.enabled[op[1]] = False
            self.removed[op[1]] = True
            if pg is not None:
                pg.remove_factor(op[1])
        else:
            raise KeyError(op[0])

    def size(self):
        """what PoseGraph.size() reports: (variables, factors still in the graph, enabled factors)"""
        return len(self.poses), self.removed.count(False), self.enabled.count(True)

    def graph(self, poses=None):
        D, E = PR.dim(self.kind), len(self.ij)
        return dict(poses=np.array(self.poses, np.float32) if poses is None else np.asarray(poses, np.float32),
                    ij=np.array(self.ij, np.int32).reshape(E, 2), Z=np.array(self.Z, np.float32).reshape((E,) + self.tshape),
                    omega=np.array(self.omega, np.float32).reshape(E, D, D), enabled=np.array(self.enabled, np.uint8),
                    fixed_mask=np.array(self.fixed, np.uint8))


def reference_fits(kind, m):
    """the float64 restatement takes this graph: dense, or banded at any size (posegraph_restatement.gn_step)"""
    ij = np.array([e for e, en in zip(m.ij, m.enabled) if en], np.int64).reshape(-1, 2)
    banded = len(m.poses) > 1 and ij.size > 0 and np.max(np.abs(ij[:, 0] - ij[:, 1])) <= PR.BANDED_WIDTH
    return bool(banded or len(m.poses) * PR.dim(kind) <= PR.DENSE_LIMIT)


# ---- leaves ------------------------------------------------------------------------------------------------------------------
def leaf_information(kind, rng):
    """an anisotropic, non-diagonal SPD information matrix: eigenvalues 0.2 .. 1 on random axes (<= 1: the chi rule of
    test_gpu_posegraph_cycles._check bounds e^T Omega e by |e|^2)"""
    D = PR.dim(kind)
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    O = Q @ np.diag(np.linspace(0.2, 1.0, D)) @ Q.T
    return ((O + O.T) / 2).astype(np.float32)


def _hop(kind, rng):
    """the relative pose a leaf's factor measures: 8 cm in a random direction and a small rotation"""
    a = rng.uniform(0, 2 * np.pi)
    if kind == SE2:
        d = [0.08 * np.cos(a), 0.08 * np.sin(a), rng.uniform(-0.1, 0.1)]
    else:
        d = [0.08 * np.cos(a), 0.08 * np.sin(a), rng.uniform(-0.02, 0.02)] + list(rng.uniform(-0.03, 0.03, 3))
    return PR.v2t(kind, np.array(d))


def _offset(kind, rng, scale=1.0):
    """where a leaf starts relative to its target: up to 0.12 m per axis and 0.08 rad (SE(3): 0.025 per quaternion component).
    Its parent may start as far from its own target, so the leaf is within 0.5 m / 0.2 rad of where its factor wants it"""
    s = np.array([0.12, 0.12, 0.08] if kind == SE2 else [0.12] * 3 + [0.025] * 3)
    return rng.uniform(-1, 1, s.size) * s * scale


def tail_ops(kind, base_poses, parents, seed, info=True, flip=lambda t: t % 2 == 1, fixed=(), offset=None):
    """operations that append leaf V0 + t with one factor to parents[t] (< V0 + t).  flip(t): the leaf is the factor's first
    endpoint (the measurement inverted).  Targets chain from the base's poses through the hops; every leaf starts at its
    target (+) an offset, whatever its parent's offset was.  fixed: tail indices appended as fixed variables."""
    rng = np.random.default_rng(seed)
    target = [np.asarray(p, np.float64) for p in base_poses]
    V0, ops = len(target), []
    for t, p in enumerate(parents):
        assert 0 <= p < V0 + t
        Z = _hop(kind, rng)
        tgt = PR._mul(kind, target[p], Z)
        target.append(tgt)
        d = _offset(kind, rng) if offset is None else np.asarray(offset, np.float64)
        ops.append(("var", PR.box_plus(kind, tgt, d).astype(np.float32), t in fixed))
        om = leaf_information(kind, rng) if info else None
        if flip(t):
            ops.append(("factor", V0 + t, p, PR._inv(kind, Z).astype(np.float32), om, True))
        else:
            ops.append(("factor", p, V0 + t, Z.astype(np.float32), om, True))
    return ops


BUILD = ("solve", dict(its=1, pcg_max=0))  # builds the hierarchy and leaves the poses where they are


def small_base(kind, V=20, seed=101):
    """at most 32 poses on the 2 m circle: level 0 is the coarsest level and dense"""
    return chain(kind, V, seed, closures=3, reversed_every=5)


# ---- a. exact tails: name -> (parents of the tail (V0 = 20), identity information?, damping) ----------------------------------
def _forest_parents(V0):
    # leaf A on the fixed pose 0, a chain of five off A, a leaf on pose 7, three leaves on pose 3, a chain of two off one of them
    A = V0
    return [0, A, A + 1, A + 2, A + 3, A + 4, 7, 3, 3, 3, V0 + 8, V0 + 10]


EXACT_TAILS = {
    "leaf": (lambda V0: [V0 - 1], True, 0.0),
    "leaf_flipped": (lambda V0: [5], False, 0.0),
    "chain32": (lambda V0: [V0 - 1] + [V0 + t for t in range(31)], False, 0.0),
    "star32": (lambda V0: [9] * 32, False, 0.0),
    "forest": (_forest_parents, False, 0.0),
    "forest_damped": (_forest_parents, True, 1e-3),
}


def exact_case(name, kind):
    parents, identity, damping = EXACT_TAILS[name]
    base = small_base(kind)
    V0 = base["poses"].shape[0]
    flip = (lambda t: True) if name == "leaf_flipped" else (lambda t: t % 2 == 1)
    ops = [BUILD] + tail_ops(kind, base["poses"], parents(V0), 7 + len(name), info=not identity, flip=flip)
    ops.append(("solve", dict(its=1, pcg_max=1, damping=damping)))
    return dict(kind=kind, base=base, ops=ops)


# ---- a'. a level 0 that is smoothed, not inverted: the cycle reads the parents' re-inverted smoother blocks -------------------
def smoothed_case(kind, pcg_max):
    """star of 299 free leaves (coarsening stalls above the dense limit); the tail: 20 leaves on the base's leaf 5 (one factor
    of its own, so the folded blocks are most of its diagonal), six on the centre, a chain of six off the base's leaf 9"""
    base = star(kind, 299, 4)
    V0 = base["poses"].shape[0]
    parents = [5] * 20 + [0] * 6 + [9] + [V0 + 26 + t for t in range(5)]
    ops = [BUILD] + tail_ops(kind, base["poses"], parents, 11) + [("solve", dict(its=1, pcg_max=pcg_max))]
    return dict(kind=kind, base=base, ops=ops)


# ---- b. multi-level bases ----------------------------------------------------------------------------------------------------
def _chain600(kind):
    return chain(kind, 600, 61, fixed=(0, 301, 302), reversed_every=11, closures=5)


def _gen(kind):
    return generator(kind, 400, 900, 62) if kind == SE2 else generator(kind, 300, 900, 63)


MULTILEVEL = {
    # a banded chain takes its leaves within BANDED_WIDTH of the end: leaf t on the pose 1 + t % 7 places below it
    "chain600": (_chain600, lambda V0: [V0 + t - 1 - t % 7 for t in range(33)]),
    # a dense reference takes them anywhere: a chain of 11 off the last pose, a star of 11 on pose 17, the rest scattered
    "generator": (_gen, lambda V0: [V0 - 1] + [V0 + t for t in range(10)] + [17] * 11 + [(37 * t) % V0 for t in range(11)]),
}
CONVERGED = dict(its=3, pcg_max=3000, tol=1e-8)


def multilevel_case(name, kind):
    make, parents = MULTILEVEL[name]
    base = make(kind)
    t = tail_ops(kind, base["poses"], parents(base["poses"].shape[0]), 21)
    assert len(t) == 2 * (TAIL_LIMIT + 1)
    ops = [BUILD] + t[:2 * TAIL_LIMIT] + [("solve", CONVERGED)] + t[2 * TAIL_LIMIT:] + [("solve", CONVERGED)]
    return dict(kind=kind, base=base, ops=ops)


# ---- c. growing from the first pose ------------------------------------------------------------------------------------------
GROW_ROUNDS = 70


def growing_case(kind, rounds=GROW_ROUNDS):
    """one fixed pose, then a pose and a factor per round, solved after every round: on the previous pose, every 7th on the
    pose five before it"""
    rng = np.random.default_rng(33)
    first = PR.v2t(kind, np.array([2.0, 0.0, 0.3] if kind == SE2 else [2.0, 0.0, 0.05, 0.0, 0.0, 0.1]))
    base = dict(poses=first[None].astype(np.float32), ij=np.zeros((0, 2), np.int32), Z=np.zeros((0,) + first.shape, np.float32),
                fixed_mask=np.ones(1, np.uint8))
    ops = [("solve", dict(its=1))]
    target = [first.astype(np.float32).astype(np.float64)]
    for k in range(1, rounds + 1):
        p = max(k - 5, 0) if k % 7 == 0 else k - 1
        if kind == SE2:
            d = [0.08, 0.0016, 0.04 + rng.uniform(-0.01, 0.01)]  # (round the 2 m circle, as the catalogue's chains go)
        else:
            d = [0.08, 0.0016, rng.uniform(-0.01, 0.01), rng.uniform(-0.005, 0.005), rng.uniform(-0.005, 0.005), 0.02]
        Zp = PR.v2t(kind, np.array(d))
        tgt = PR._mul(kind, target[k - 1], Zp)
        target.append(tgt)
        Z = PR._mul(kind, PR._inv(kind, target[p]), tgt)
        ops.append(("var", PR.box_plus(kind, tgt, _offset(kind, rng)).astype(np.float32), False))
        om = leaf_information(kind, rng) if k % 2 else None
        if k % 3 == 0:
            ops.append(("factor", k, p, PR._inv(kind, Z).astype(np.float32), om, True))
        else:
            ops.append(("factor", p, k, Z.astype(np.float32), om, True))
        ops.append(("solve", dict(its=2)))
    return dict(kind=kind, base=base, ops=ops)


# ---- d. what the classifier refuses ------------------------------------------------------------------------------------------
REFUSALS = ["fixed_variable", "disabled_factor", "two_factors", "closure_onto_tail", "factor_to_later_tail", "keep_structure_0"]
SOLVE2 = dict(its=2)


def refusal_case(name, kind):
    """(case, tuning): a base of 20 poses, what is appended, and the solve that must rebuild"""
    base = small_base(kind, seed=103)
    V0, E0 = base["poses"].shape[0], base["ij"].shape[0]
    rng = np.random.default_rng(41)
    tuning, ops = {}, [BUILD]
    if name == "fixed_variable":  # a free leaf and a fixed one
        ops += tail_ops(kind, base["poses"], [4, 11], 42, fixed=(1,)) + [("solve", SOLVE2)]
    elif name == "disabled_factor":  # two leaves, the second one's only factor disabled (damping keeps its block regular)
        t = tail_ops(kind, base["poses"], [4, 11], 43)
        t[3] = t[3][:5] + (False,)
        ops += t + [("solve", dict(its=2, damping=1e-3))]
    elif name == "two_factors":  # one new pose between two old ones
        t = tail_ops(kind, base["poses"], [6], 44)
        X = np.asarray(t[0][1], np.float64)
        Z2 = PR._mul(kind, PR._inv(kind, np.asarray(base["poses"][8], np.float64)), X)
        ops += t + [("factor", 8, V0, Z2.astype(np.float32), leaf_information(kind, rng), True), ("solve", SOLVE2)]
    elif name == "closure_onto_tail":  # two leaves, eliminated; then a factor from an old pose onto the second
        t = tail_ops(kind, base["poses"], [6, 12], 45)
        X = np.asarray(t[2][1], np.float64)
        Z2 = PR._mul(kind, PR._inv(kind, np.asarray(base["poses"][3], np.float64)), X)
        ops += t + [("solve", SOLVE2), ("factor", 3, V0 + 1, Z2.astype(np.float32), leaf_information(kind, rng), True),
                    ("solve", SOLVE2)]
    elif name == "factor_to_later_tail":  # A and B appended; A's only factor goes to B, B's to an old pose
        t = tail_ops(kind, base["poses"], [9, V0], 46)  # (targets: A on pose 9, B on A)
        va, _, vb, fb = t  # (fb joins A and B; A's factor to pose 9 is left out)
        Zb = PR._mul(kind, PR._inv(kind, np.asarray(base["poses"][9], np.float64)), np.asarray(vb[1], np.float64))
        ops += [va, vb, fb, ("factor", 9, V0 + 1, Zb.astype(np.float32), leaf_information(kind, rng), True), ("solve", SOLVE2)]
    elif name == "keep_structure_0":
        tuning = dict(keep_structure=0)
        ops += tail_ops(kind, base["poses"], [4, V0], 47) + [("solve", SOLVE2)]
    else:
        raise KeyError(name)
    return dict(kind=kind, base=base, ops=ops), tuning


def orphan_case(kind, how, damping):
    """a tail of four, eliminated; then the factor of its third leaf (which has no child) disabled or removed, and a solve"""
    base = small_base(kind, seed=105)
    V0, E0 = base["poses"].shape[0], base["ij"].shape[0]
    ops = [BUILD] + tail_ops(kind, base["poses"], [V0 - 1, V0, 4, V0 + 1], 51)
    ops += [("solve", dict(its=2, damping=damping)), (how, E0 + 2), ("solve", dict(its=2, damping=damping))]
    return dict(kind=kind, base=base, ops=ops), V0 + 2


# ---- e. a kept hierarchy -----------------------------------------------------------------------------------------------------
def kept_case(kind):
    """the banded chain converged, then three leaves that start 0.45 m from where their factors want them"""
    base = _chain600(kind)
    V0 = base["poses"].shape[0]
    off = [0.36, -0.27, 0.1] if kind == SE2 else [0.3, -0.25, 0.22, 0.03, -0.02, 0.04]
    ops = [("solve", dict(its=6, pcg_max=3000, tol=1e-8))] + tail_ops(kind, base["poses"], [V0 - 1, V0, V0 - 4], 71, offset=off)
    ops.append(("solve", CONVERGED))
    return dict(kind=kind, base=base, ops=ops)


def all_cases():
    """every (name, case) tests/test_gpu_posegraph_append.py runs"""
    out = []
    for kind in KINDS:
        k = "se2" if kind == SE2 else "se3"
        out += [("exact-%s-%s" % (n, k), exact_case(n, kind)) for n in EXACT_TAILS]
        out += [("smoothed-%d-%s" % (n, k), smoothed_case(kind, n)) for n in (1, 2)]
        out += [("multilevel-%s-%s" % (n, k), multilevel_case(n, kind)) for n in MULTILEVEL]
        out += [("growing-%s" % k, growing_case(kind))]
        out += [("refusal-%s-%s" % (n, k), refusal_case(n, kind)[0]) for n in REFUSALS]
        out += [("orphan-%s-%g-%s" % (h, d, k), orphan_case(kind, h, d)[0]) for h in ("disable", "remove") for d in (0.0, 1e-3)]
        out += [("kept-%s" % k, kept_case(kind))]
    return out
