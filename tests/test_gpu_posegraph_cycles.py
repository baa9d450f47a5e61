"""-m gpu: every V-cycle shape and solver knob of the pose-graph solver (csrc/posegraph.hip) against float64.

The reference is the numpy restatement (tests/posegraph_restatement.py; dense up to ~4 500 unknowns, block-banded for
odometry chains with short closures), or the oracle's block-Jacobi PCG at pcg_tolerance = 1e-10 where neither fits.  Which cycle ran is read from
the solver's own `posegraph hierarchy:` debug line (set_tuning(debug=1), printed when the structure is built) and restated in
`Shape` with the rules of pg_solve_t; every case asserts the level sizes it was built for, so moving a constant fails the case
instead of quietly testing a different path.  A converged solve cannot see a wrong preconditioner, so besides converged
solves this module holds the preconditioner itself: exact at level 0 (one CG iteration is the direct solve), and the two
cycle implementations against each other after 1, 2 and 5 CG iterations."""
import re

import numpy as np
import pytest

import posegraph_restatement as PR
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import posegraph as pgm
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SE2, SE3 = abi.SE2_RIGHT, abi.SE3_QUAT_RIGHT
KINDS = [SE2, SE3]
# the constants of csrc/posegraph.hip the shape rules below restate
MG_FUSE_NODES, MG_FUSE_BLOCKS, MG_COARSEST_NODES, MG_FUSE_LAST_NODES = 170, 1200, 32, 16
LDS_BYTES = 150 * 1024  # dynamic LDS k_mg_coarsest_inverse asks for
PCG_CHUNK = 10

_HIER = re.compile(r"posegraph hierarchy:(.*?) coarsest (dense|smoothed);")
_LEVEL = re.compile(r"(\d+) nodes / (\d+) blocks")
_LAG = re.compile(r"posegraph: iteration (\d+), max \|dx\| (\S+)")
_LDS = re.compile(r"posegraph: coarsest inverse of (\d+) unknowns, in_lds (\d)")


class Shape:
    """the cycle pg_solve_t runs for a hierarchy, restated from its debug line"""

    def __init__(self, D, text, two_phase=True):
        m = _HIER.search(text)
        assert m, "no hierarchy line in the solver's debug output:\n" + text[-2000:]
        self.D, self.two_phase = D, bool(two_phase)
        self.levels = [(int(n), int(ne)) for n, ne in _LEVEL.findall(m.group(1))]
        self.dense = m.group(2) == "dense"
        L = self.levels
        self.nl = len(L) - 1
        self.lf = next((l for l in range(self.nl) if L[l][0] <= MG_FUSE_NODES and L[l][1] <= MG_FUSE_BLOCKS), self.nl)
        # (pg_solve_t: fuse_last needs levels[nl].n == levels[nl - 1].nc, which holds by construction)
        self.fuse_last = self.dense and self.lf == self.nl >= 2 and L[-1][0] <= MG_FUSE_LAST_NODES
        self.dense_bottom = self.two_phase and self.fuse_last and L[-2][0] * D <= 1024
        self.fused_path = self.two_phase and self.lf >= 1 and self.nl >= 1
        # build_hierarchy stops at a level of <= 32 free nodes; a coarsest level above that is where matching stalled
        self.stalled = L[-1][0] > MG_COARSEST_NODES
        nc = L[-1][0] * D
        expect = None if not self.dense else (2 if 2 * nc * nc * 8 <= LDS_BYTES else 1 if nc * nc * 8 <= LDS_BYTES else 0)
        # the mode k_mg_coarsest_inverse ran in, as the solver reports it (it falls back to 0 when the LDS request fails)
        seen = {(int(n), int(m)) for n, m in _LDS.findall(text)}
        assert seen == (set() if expect is None else {(nc, expect)}), (seen, nc, expect)
        self.in_lds = expect

    def nodes(self):
        return tuple(n for n, _ in self.levels)

    def labels(self):
        s = set()
        if self.nl == 0:
            s.add("level0_coarsest")
        if self.stalled:
            s.add("stalled_dense" if self.dense else "stalled_smoothed")
        if self.nl >= 1:
            s.add("lf0" if self.lf == 0 else "lf1" if self.lf == 1 else "lf2+")
        if any(n <= MG_FUSE_NODES and ne > MG_FUSE_BLOCKS for n, ne in self.levels[:self.lf]):
            s.add("lf_dense_level")
        if self.in_lds is not None:
            s.add("inverse_lds%d" % self.in_lds)
        if self.fused_path and self.fuse_last and not self.dense_bottom:
            s.add("fuse_last")  # k_mg_down2_coarsest
        if self.dense_bottom:
            s.add("dense_bottom")  # k_bd_*, k_mg_bottom_dense
        if not self.two_phase and self.nl >= 1:
            s.add("six_phase")
        return s

    def __repr__(self):
        return "Shape(levels=%s, %s, nl=%d, lf=%d, labels=%s)" % (self.levels, "dense" if self.dense else "smoothed", self.nl, self.lf,
                                                               sorted(self.labels()))


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def _poses(kind, xy, yaw, seed):
    """ground-truth poses at positions xy (V, 2 or 3) with headings yaw (+ small roll / pitch for SE(3))"""
    if kind == SE2:
        return PR.v2t(SE2, np.concatenate([xy[:, :2], yaw[:, None]], 1))
    rng = np.random.default_rng(seed)
    t = np.concatenate([xy[:, :2], xy[:, 2:3] if xy.shape[1] > 2 else rng.normal(size=(xy.shape[0], 1)) * 0.05], 1)
    half = np.stack([rng.normal(size=xy.shape[0]) * 0.01, rng.normal(size=xy.shape[0]) * 0.01, yaw / 2], 1)
    q = np.sin(half[:, 2:3]) * np.array([0.0, 0.0, 1.0]) + half * [1, 1, 0]  # (small roll / pitch, yaw about z)
    return PR.v2t(SE3, np.concatenate([t, q], 1))


def _graph(kind, gt, ij, seed, fixed=(0,), perturb=0.03, noise=0.01):
    # (perturbation of the initial poses: sigma * perturb / noise, i.e. 0.03 m / 0.015 rad (SE(2)) whatever the noise)
    """factors ij with measurements = true relative pose (+) noise; initial poses = truth (+) perturbation, fixed ones true"""
    D = PR.dim(kind)
    rng = np.random.default_rng(seed)
    ij = np.asarray(ij, np.int32).reshape(-1, 2)
    sig = np.array([noise, noise, noise / 2] if kind == SE2 else [noise] * 3 + [noise / 4] * 3)
    Z = PR.box_plus(kind, PR._mul(kind, PR._inv(kind, gt[ij[:, 0]]), gt[ij[:, 1]]), rng.normal(size=(ij.shape[0], D)) * sig)
    P = PR.box_plus(kind, gt, rng.normal(size=(gt.shape[0], D)) * sig * perturb / noise)
    fm = np.zeros(gt.shape[0], np.uint8)
    fm[list(fixed)] = 1
    P[fm.astype(bool)] = gt[fm.astype(bool)]
    return dict(poses=P.astype(np.float32), ij=ij, Z=Z.astype(np.float32), fixed_mask=fm)


def chain(kind, V, seed, fixed=(0,), closures=0, reversed_every=0, duplicates=(), noise=2e-4, anchor_every=0):
    """an odometry chain round and round a circle of 2 m, optionally with a few short closures, reversed and duplicated factors
    and a fixed pose every `anchor_every` poses; small odometry noise keeps the drift of a long chain, hence the step, small.

    Small positions and anchors keep the solver's float32 residual visible at most at the few-1e-6 level in the step:
    edge_linearize (csrc/posegraph.hip) forms Z^-1 Xi^-1 Xj in float32, which rounds the residual by ~1e-7 |t|, and a long
    free chain amplifies that error of b by the conditioning of H -- on a 10 m circle without anchors the steps of 3 000-12 000
    pose chains moved by 1-3e-5 (restated in numpy with a float32 residual: 2-3e-5)."""
    fixed = tuple(fixed) + (tuple(range(anchor_every, V, anchor_every)) if anchor_every else ())
    s = np.arange(V, dtype=np.float64)
    xy = np.stack([2 * np.cos(0.04 * s), 2 * np.sin(0.04 * s), 0.1 * np.sin(0.005 * s)], 1)
    gt = _poses(kind, xy, 0.3 * np.sin(0.02 * s), seed)
    ij = np.stack([np.arange(V - 1), np.arange(1, V)], 1)
    if reversed_every:
        ij[::reversed_every] = ij[::reversed_every, ::-1]
    extra = [ij[list(duplicates)]] if len(duplicates) else []
    if closures:
        rng = np.random.default_rng(seed + 1)
        ci = rng.integers(0, V - 6, closures)
        extra.append(np.stack([ci, ci + rng.integers(2, 6, closures)], 1))
    ij = np.concatenate([ij] + extra).astype(np.int32)
    return _graph(kind, gt, ij, seed, fixed, noise=noise)


def star(kind, leaves, seed, duplicate=False):
    """centre 0 (free) joined to `leaves` free leaves and one fixed leaf (the last pose): matching pairs the centre with one
    leaf and leaves every other leaf alone, so coarsening stalls at level 0"""
    rng = np.random.default_rng(seed)
    V = leaves + 2
    ang = rng.uniform(0, 2 * np.pi, V)
    rad = rng.uniform(0.5, 3.0, V)
    xy = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.normal(size=V) * 0.2], 1)
    xy[0] = 0
    gt = _poses(kind, xy, rng.uniform(-1, 1, V), seed)
    ij = np.stack([np.zeros(V - 1, int), np.arange(1, V)], 1)
    ij[1::3] = ij[1::3, ::-1]  # (reversed factors)
    if duplicate:
        ij = np.concatenate([ij, ij[[0, 2]]])
    return _graph(kind, gt, ij, seed, fixed=(V - 1,))


def clique(kind, V, seed, drop=40):
    """a small but dense graph: all pairs of V poses but `drop` (more than MG_FUSE_BLOCKS blocks on <= MG_FUSE_NODES nodes)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-3, 3, (V, 3))
    gt = _poses(kind, xy, rng.uniform(-1, 1, V), seed)
    a, b = np.triu_indices(V, 1)
    keep = np.ones(a.size, bool)
    keep[rng.choice(np.flatnonzero(np.abs(a - b) > 1), drop, replace=False)] = False
    return _graph(kind, gt, np.stack([a[keep], b[keep]], 1), seed, fixed=(3,))


def random_dense(kind, V, E, seed):
    """V poses in a box, a path through them plus E - V + 1 random factors between any two: its first coarse level is
    small but dense"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-5, 5, (V, 3))
    gt = _poses(kind, xy, rng.uniform(-1, 1, V), seed)
    path = np.stack([np.arange(V - 1), np.arange(1, V)], 1)
    a = rng.integers(0, V, 2 * E)
    b = rng.integers(0, V, 2 * E)
    ok = a != b
    ij = np.concatenate([path, np.stack([a[ok], b[ok]], 1)[:E - V + 1]])
    return _graph(kind, gt, ij, seed, fixed=(0, V // 2))


def generator(kind, V, E, seed):
    g = syn.pose_graph_2d(V=V, E=E, seed=seed) if kind == SE2 else syn.pose_graph_3d(V=V, E=E, seed=seed)
    P = g["poses_init"]
    return dict(poses=P, ij=g["ij"], Z=g["Z"], fixed_mask=None)


def info_case(kind, seed=77):
    """full information matrices, disabled factors, several fixed poses, damping (SE(2) and SE(3))"""
    g = generator(kind, 400, 900, seed) if kind == SE2 else generator(kind, 300, 900, seed)
    D = PR.dim(kind)
    E = g["ij"].shape[0]
    V = g["poses"].shape[0]
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(E, D, D)) * 0.3
    g["omega"] = ((np.eye(D) + np.einsum("eab,ecb->eac", A, A)) * 50.0).astype(np.float32)
    en = np.ones(E, np.uint8)
    en[V + 3::5] = 0
    g["enabled"] = en
    fm = np.zeros(V, np.uint8)
    fm[[0, 100, 101, 250]] = 1
    g["fixed_mask"] = fm
    return g


# name -> (builder(kind), tuning, damping, GN iterations)
CASES = {
    "two": (lambda k: chain(k, 2, 1, duplicates=(0,)), {}, 0.0, 2),
    "p33": (lambda k: chain(k, 33, 2, closures=4, reversed_every=7, duplicates=(5,)), {}, 0.0, 2),
    "star200": (lambda k: star(k, 199, 3), {}, 0.0, 1),
    "star300": (lambda k: star(k, 299, 4), {}, 0.0, 1),
    "clique60": (lambda k: clique(k, 60, 5), {}, 0.0, 1),
    "chain_lf1": (lambda k: chain(k, 600, 6, fixed=(0, 301, 302), reversed_every=11, duplicates=(40, 41)), {}, 0.1, 2),
    "chain_lf2": (lambda k: chain(k, 3000, 7, anchor_every=500), {}, 0.0, 1),
    "chain_p4": (lambda k: chain(k, 3000, 8, anchor_every=500), {"match_passes": 4}, 0.0, 1),
    "chain_p5": (lambda k: chain(k, 11200, 9, anchor_every=800), {"match_passes": 5}, 0.0, 1),
    "random_dense": (lambda k: random_dense(k, 700, 4000, 10), {}, 0.0, 1),
    "long_se2": (lambda k: chain(k, 12000, 11, closures=12, anchor_every=400), {"match_passes": 1}, 0.0, 1),
    "info": (info_case, {}, 0.5, 2),
    "rows_lo": (lambda k: generator(k, 83 if k == SE2 else 41, 250 if k == SE2 else 120, 12), {}, 0.0, 1),
    "rows_eq": (lambda k: generator(k, 84 if k == SE2 else 42, 250 if k == SE2 else 120, 13), {}, 0.0, 1),
    "rows_hi": (lambda k: generator(k, 85 if k == SE2 else 43, 250 if k == SE2 else 120, 14), {}, 0.0, 1),
    "tiles_lo": (lambda k: generator(k, 335 if k == SE2 else 167, 1000 if k == SE2 else 500, 15), {}, 0.0, 1),
    "tiles_eq": (lambda k: generator(k, 336 if k == SE2 else 168, 1000 if k == SE2 else 500, 16), {}, 0.0, 1),
    "tiles_hi": (lambda k: generator(k, 337 if k == SE2 else 169, 1000 if k == SE2 else 500, 17), {}, 0.0, 1),
}
SE2_ONLY = {"long_se2", "chain_p5"}

# frozen from the solver's debug line on an MI355X: (kind, case) -> (nodes per level, branch labels)
EXPECT = {
    (SE2, "two"): ((2,), {"inverse_lds2", "level0_coarsest"}),
    (SE3, "two"): ((2,), {"inverse_lds2", "level0_coarsest"}),
    (SE2, "p33"): ((33, 4), {"inverse_lds2", "lf0"}),
    (SE3, "p33"): ((33, 4), {"inverse_lds2", "lf0"}),
    (SE2, "star200"): ((201,), {"inverse_lds0", "level0_coarsest", "stalled_dense"}),
    (SE3, "star200"): ((201,), {"inverse_lds0", "level0_coarsest", "stalled_dense"}),
    (SE2, "star300"): ((301,), {"level0_coarsest", "stalled_smoothed"}),
    (SE3, "star300"): ((301,), {"level0_coarsest", "stalled_smoothed"}),
    (SE2, "clique60"): ((60, 8), {"inverse_lds2", "lf1", "lf_dense_level"}),
    (SE3, "clique60"): ((60, 8), {"inverse_lds2", "lf1", "lf_dense_level"}),
    (SE2, "chain_lf1"): ((600, 76, 10), {"inverse_lds2", "lf1"}),
    (SE3, "chain_lf1"): ((600, 76, 10), {"inverse_lds2", "lf1"}),
    (SE2, "chain_lf2"): ((3000, 378, 48, 6), {"inverse_lds2", "lf2+"}),
    (SE3, "chain_lf2"): ((3000, 378, 48, 6), {"inverse_lds2", "lf2+"}),
    (SE2, "chain_p4"): ((3000, 192, 12), {"dense_bottom", "inverse_lds2", "lf2+"}),
    (SE3, "chain_p4"): ((3000, 192, 12), {"fuse_last", "inverse_lds2", "lf2+"}),
    (SE2, "chain_p5"): ((11200, 350, 14), {"fuse_last", "inverse_lds2", "lf2+"}),
    (SE2, "random_dense"): ((700, 102, 13), {"dense_bottom", "inverse_lds2", "lf2+", "lf_dense_level"}),
    (SE3, "random_dense"): ((700, 103, 13), {"dense_bottom", "inverse_lds2", "lf2+", "lf_dense_level"}),
    (SE2, "long_se2"): ((12000, 6000, 3000, 1500, 750, 390, 210, 120, 60, 30), {"inverse_lds2", "lf2+"}),
    (SE2, "info"): ((400, 50, 7), {"inverse_lds2", "lf1"}),
    (SE3, "info"): ((300, 41, 6), {"inverse_lds2", "lf1"}),
    (SE2, "rows_lo"): ((83, 11), {"inverse_lds2", "lf0"}),
    (SE3, "rows_lo"): ((41, 5), {"inverse_lds2", "lf0"}),
    (SE2, "rows_eq"): ((84, 11), {"inverse_lds2", "lf0"}),
    (SE3, "rows_eq"): ((42, 6), {"inverse_lds2", "lf0"}),
    (SE2, "rows_hi"): ((85, 11), {"inverse_lds2", "lf0"}),
    (SE3, "rows_hi"): ((43, 6), {"inverse_lds2", "lf0"}),
    (SE2, "tiles_lo"): ((335, 42, 6), {"inverse_lds2", "lf1"}),
    (SE3, "tiles_lo"): ((167, 22), {"inverse_lds1", "lf0"}),
    (SE2, "tiles_eq"): ((336, 42, 6), {"inverse_lds2", "lf1"}),
    (SE3, "tiles_eq"): ((168, 23), {"inverse_lds1", "lf0"}),
    (SE2, "tiles_hi"): ((337, 43, 6), {"inverse_lds2", "lf1"}),
    (SE3, "tiles_hi"): ((169, 22), {"inverse_lds1", "lf0"}),
}

_graph_cache = {}


def build_case(name, kind):
    key = (name, kind)
    if key not in _graph_cache:
        _graph_cache[key] = CASES[name][0](kind)
    return _graph_cache[key]


def _params(its, pcg_max=3000, tol=1e-10, damping=0.0):
    p = pgm.default_params()
    p.max_iterations, p.pcg_max_iterations, p.pcg_tolerance, p.damping = its, pcg_max, tol, damping
    return p


def gpu_solve(product, capfd, kind, g, params, **tuning):
    """solve on a fresh handle with debug output; returns (stats, poses, Shape, debug text)"""
    pg = product.PoseGraph(kind)
    pg.set_tuning(debug=1, **tuning)
    pg.set_graph(g["poses"], g["ij"], g["Z"], omega=g.get("omega"), fixed_mask=g.get("fixed_mask"), enabled=g.get("enabled"))
    capfd.readouterr()
    st = pg.solve(params)
    err = capfd.readouterr().err
    shape = Shape(pg.D, err, tuning.get("two_phase", 1))
    P = pg.poses().copy()
    pg.close()
    return st, P, shape, err


def reference(kind, g, its, damping=0.0, oracle=None):
    """(chi per iteration, poses after `its` steps): the float64 restatement, or the oracle at 1e-10 where it does not fit"""
    D = PR.dim(kind)
    V = g["poses"].shape[0]
    ij = np.asarray(g["ij"])
    banded = np.max(np.abs(ij[:, 0] - ij[:, 1])) <= PR.BANDED_WIDTH
    if banded or V * D <= PR.DENSE_LIMIT:
        return PR.gauss_newton(kind, g["poses"], g["ij"], g["Z"], its, omega=g.get("omega"), enabled=g.get("enabled"),
                               fixed_mask=g.get("fixed_mask"), damping=damping)
    assert oracle is not None
    pg = oracle.OraclePoseGraph(kind)
    pg.set_graph(g["poses"], g["ij"], g["Z"], omega=g.get("omega"), fixed_mask=g.get("fixed_mask"), enabled=g.get("enabled"))
    st = pg.solve(_params(its, pcg_max=100000, damping=damping))
    assert all(s["solver_status"] == 0 and s["pcg_iterations"] < 100000 for s in st), st
    return [s["chi"] for s in st], pg.poses().copy()


_ref_cache = {}


def cached_reference(name, kind, oracle):
    key = (name, kind)
    if key not in _ref_cache:
        _, _, damping, its = CASES[name]
        _ref_cache[key] = reference(kind, build_case(name, kind), its, damping, oracle)
    return _ref_cache[key]


def _check(st, P, ref_chis, ref_P, m, chi_rel=1e-5, pose_tol=1e-5):
    """chi of every iteration within chi_rel of the reference, plus the floor of the solver's float32 residual: edge_linearize
    (csrc/posegraph.hip) forms Z^-1 Xi^-1 Xj in float32, so each of the m residual components carries a rounding of up to
    ~2.4e-7 at the catalogue's <= 2 m positions, and chi = sum e^2 moves by up to 2 sqrt(m chi) 2.4e-7 (this only matters
    near the optimum: chi ~1e-5 on the second iteration of small graphs)"""
    assert len(st) == len(ref_chis)
    for k, (s, c) in enumerate(zip(st, ref_chis)):
        assert s["solver_status"] == 0, st
        floor = 2.0 * np.sqrt(m * c) * 2.4e-7
        assert abs(s["chi"] - c) <= chi_rel * max(c, 1e-12) + floor, (k, s["chi"], c)
    d = float(np.max(np.abs(P - ref_P)))
    assert d <= pose_tol, d


# ---- a. the catalogue: one graph per branch, both dimensions ----------------------------------------------------------------
CATALOGUE = [(n, k) for n in CASES for k in KINDS if k == SE2 or n not in SE2_ONLY]


def _ids(v):
    return {SE2: "se2", SE3: "se3"}.get(v, str(v))


@pytest.mark.parametrize("name,kind", CATALOGUE, ids=["%s-%s" % (n, _ids(k)) for n, k in CATALOGUE])
def test_catalogue(oracle, product, capfd, name, kind):
    _, tuning, damping, its = CASES[name]
    g = build_case(name, kind)
    st, P, shape, _ = gpu_solve(product, capfd, kind, g, _params(its, damping=damping), **tuning)
    print(name, kind, shape)
    assert EXPECT.get((kind, name)) == (shape.nodes(), shape.labels()), shape
    chis, ref_P = cached_reference(name, kind, oracle)
    _check(st, P, chis, ref_P, g["ij"].shape[0] * PR.dim(kind))
    fm = g.get("fixed_mask")
    fixed = np.zeros(P.shape[0], bool) if fm is None else fm.astype(bool)
    if fm is None:
        fixed[0] = True
    assert np.array_equal(P[fixed], np.asarray(g["poses"])[fixed])


# ---- b. exact preconditioner: level 0 is the coarsest and dense, so the cycle is H^-1 --------------------------------------
# name -> (kind, builder, k_mg_coarsest_inverse's in_lds mode)
EXACT = {
    "se3_16": (SE3, lambda: generator(SE3, 16, 40, 31), 2),
    "se3_23": (SE3, lambda: generator(SE3, 23, 60, 32), 1),
    "se3_24": (SE3, lambda: generator(SE3, 24, 60, 33), 0),
    "se3_32": (SE3, lambda: generator(SE3, 32, 90, 34), 0),
    "se3_star256": (SE3, lambda: star(SE3, 255, 35), 0),
    "se3_star40_dup": (SE3, lambda: star(SE3, 39, 36, duplicate=True), 0),
    "se2_32": (SE2, lambda: generator(SE2, 32, 80, 37), 2),
    "se2_star40": (SE2, lambda: star(SE2, 39, 38), 1),
    "se2_star100": (SE2, lambda: star(SE2, 99, 39), 0),
    "se2_star256_dup": (SE2, lambda: star(SE2, 255, 40, duplicate=True), 0),
}


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_preconditioner_one_cg_iteration(product, capfd, name):
    """pcg_max_iterations = 1: one CG step with the preconditioner H^-1 is the direct solve (alpha = 1, x = H^-1 (-b))"""
    kind, make, mode = EXACT[name]
    g = make()
    st, P, shape, _ = gpu_solve(product, capfd, kind, g, _params(1, pcg_max=1))
    assert shape.nl == 0 and shape.dense and shape.in_lds == mode, shape
    assert st[0]["solver_status"] == 0 and st[0]["pcg_iterations"] == 1, st
    chis, ref_P = PR.gauss_newton(kind, g["poses"], g["ij"], g["Z"], 1, fixed_mask=g["fixed_mask"])
    assert np.max(np.abs(ref_P - np.asarray(g["poses"]))) > 1e-2  # the step moves the poses
    _check(st, P, chis, ref_P, g["ij"].shape[0] * PR.dim(kind))


# ---- c. truncated PCG: the two-phase cycle against the six-phase one ---------------------------------------------------------
TRUNCATED = [("chain_lf2", SE2), ("chain_lf2", SE3), ("chain_p4", SE2), ("chain_p4", SE3), ("chain_p5", SE2),
             ("random_dense", SE2), ("random_dense", SE3)]


@pytest.mark.parametrize("pcg_max", [1, 2, 5])
@pytest.mark.parametrize("name,kind", TRUNCATED, ids=["%s-%s" % (n, _ids(k)) for n, k in TRUNCATED])
def test_truncated_pcg_two_phase_matches_six_phase(product, capfd, name, kind, pcg_max):
    """One GN step cut after 1, 2, 5 CG iterations: x is then a fixed polynomial of the preconditioner applied to b, so the
    two implementations of the V-cycle (k_mg_down2 / k_mg_up2 / k_mg_down2_coarsest / k_bd_* / k_mg_bottom_dense with the fused
    CG steps, against the six-phase k_mg_op chain, k_mg_coarse_cycle and the unfused CG steps) must agree to rounding."""
    _, tuning, _, _ = CASES[name]
    g = build_case(name, kind)
    st1, P1, s1, _ = gpu_solve(product, capfd, kind, g, _params(1, pcg_max=pcg_max), **tuning)
    st0, P0, s0, _ = gpu_solve(product, capfd, kind, g, _params(1, pcg_max=pcg_max), two_phase=0, **tuning)
    assert s1.fused_path and not s0.fused_path and s1.nodes() == s0.nodes()
    assert st1[0]["pcg_iterations"] == st0[0]["pcg_iterations"] == pcg_max
    step = float(np.max(np.abs(P1.astype(np.float64) - np.asarray(g["poses"]))))
    assert step > 1e-2  # the comparison has teeth
    d = float(np.max(np.abs(P1 - P0)))
    print("truncated", name, kind, pcg_max, "two-phase vs six-phase %.3g, step %.3g" % (d, step))
    # (+ one float32 spacing of the largest pose entry: the two runs round their poses to float32 independently)
    assert d <= 1e-6 + float(np.spacing(np.max(np.abs(P1)))), (d, step)


# ---- d. the captured CG chunk against eager launches -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=["se2", "se3"])
@pytest.mark.parametrize("pcg_max", [1, 9, 10, 11, 20, 25, 3000])
def test_graph_replay_is_bit_identical(product, capfd, kind, pcg_max):
    """use_graph = 1 replays chunks of PCG_CHUNK captured iterations, use_graph = 0 launches them one by one: the same
    kernels on the same operands, so poses, chi, pcg_iterations and pcg_residual are identical bits.  pcg_max = 3000 at
    tolerance 1e-6 converges inside a chunk"""
    g = build_case("chain_lf1", kind)
    tol = 1e-6 if pcg_max == 3000 else 1e-10
    runs = [gpu_solve(product, capfd, kind, g, _params(2, pcg_max=pcg_max, tol=tol), use_graph=u) for u in (1, 0)]
    (sa, Pa, _, ea), (sb, Pb, _, eb) = runs
    assert ("CG chunk captured" in ea) == (pcg_max >= PCG_CHUNK) and "CG chunk captured" not in eb
    assert sa == sb and Pa.tobytes() == Pb.tobytes()
    if pcg_max == 3000:
        assert all(s["pcg_iterations"] % PCG_CHUNK != 0 for s in sa), sa
    else:
        assert all(s["pcg_iterations"] == pcg_max for s in sa), sa


@pytest.mark.parametrize("kind", KINDS, ids=["se2", "se3"])
@pytest.mark.parametrize("use_graph", [1, 0])
def test_zero_cg_iterations_leave_the_poses(product, capfd, kind, use_graph):
    g = build_case("p33", kind)
    st, P, _, _ = gpu_solve(product, capfd, kind, g, _params(2, pcg_max=0), use_graph=use_graph)
    assert P.tobytes() == np.asarray(g["poses"], np.float32).tobytes()
    c = PR.chi(kind, g["poses"], g["ij"], g["Z"])
    assert len(st) == 2 and all(s["solver_status"] == 0 and s["pcg_iterations"] == 0 for s in st)
    assert all(abs(s["chi"] - c) <= 1e-5 * c for s in st)


# ---- e. the knobs ------------------------------------------------------------------------------------------------------------
KNOB_GRAPH = {SE2: lambda: chain(SE2, 1000, 41, closures=300, fixed=(0, 500)),
              SE3: lambda: chain(SE3, 500, 42, closures=150, fixed=(0, 250))}
KNOB_ITERATIONS = 3
KNOBS = ([("match_passes", v) for v in (1, 2, 3, 4)] + [("omega_p", v) for v in (0.0, 0.5, 0.75)] +
         [("omega", v) for v in (0.6, 0.8, 1.0)] + [("lag_below", v) for v in (0.0, 0.05, 1e9)] +
         [("keep_structure", v) for v in (0, 1)])
_knob_ref = {}


KNOB_PARAMS = [pytest.param(k, n, v, id="%s=%g-%s" % (n, v, _ids(k))) for n, v in KNOBS for k in KINDS]


@pytest.mark.parametrize("kind,knob,value", KNOB_PARAMS)
def test_knob_sweep(product, capfd, kind, knob, value):
    if kind not in _knob_ref:
        g = KNOB_GRAPH[kind]()
        _knob_ref[kind] = (g, PR.gauss_newton(kind, g["poses"], g["ij"], g["Z"], KNOB_ITERATIONS, fixed_mask=g["fixed_mask"]))
    g, (chis, ref_P) = _knob_ref[kind]
    st, P, shape, err = gpu_solve(product, capfd, kind, g, _params(KNOB_ITERATIONS), **{knob: value})
    if knob == "lag_below":
        # pg_solve_t: iteration it > 0 keeps the previous hierarchy when the last step's max |dx| < lag_below (printed then)
        steps = [(int(a), float(b)) for a, b in _LAG.findall(err)]
        if value == 0.0:
            assert steps == []
        else:
            assert [k for k, _ in steps] == list(range(KNOB_ITERATIONS - 1))
            reused = [d < value for _, d in steps]
            assert all(reused) if value == 1e9 else not all(reused)
    _check(st, P, chis, ref_P, g["ij"].shape[0] * PR.dim(kind))


@pytest.mark.parametrize("kind", KINDS, ids=["se2", "se3"])
def test_keep_structure_across_set_graph(product, capfd, kind):
    """keep_structure = 1 reuses the structure for a second set() of the same topology; 0 rebuilds it: the same poses"""
    g = KNOB_GRAPH[kind]()
    out = []
    for keep in (1, 0):
        pg = product.PoseGraph(kind)
        pg.set_tuning(keep_structure=keep)
        for _ in range(2):
            pg.set_graph(g["poses"], g["ij"], g["Z"], fixed_mask=g["fixed_mask"])
            st = pg.solve(_params(1))
            assert st[0]["solver_status"] == 0
        out.append((pg.structure_info()[0], pg.poses().copy()))
        pg.close()
    assert out[0][0] == 1 and out[1][0] == 2, out
    assert np.max(np.abs(out[0][1] - out[1][1])) <= 1e-6


# multigrid PCG against the oracle's block-Jacobi PCG on one GN step of 3 000 SE(2) poses at tolerance 1e-10
ITERATION_RATIO = 10


def test_multigrid_takes_fewer_cg_iterations_than_block_jacobi(oracle, product, capfd):
    """a coarse correction that silently does nothing leaves a block-Jacobi-like PCG: many more CG iterations.  Measured on
    an MI355X: the oracle's block-Jacobi PCG 1 742 CG iterations, multigrid 37 (a 47x gap); the bound asks for 10x, more than
    2x headroom on the measured gap and on the multigrid count"""
    g = generator(SE2, 3000, 9000, 5100)
    p = _params(1, pcg_max=20000)
    ref = oracle.OraclePoseGraph(SE2)
    ref.set_graph(g["poses"], g["ij"], g["Z"])
    so = ref.solve(p)
    sg, _, shape, _ = gpu_solve(product, capfd, SE2, g, p)
    print("CG iterations: oracle block-Jacobi %d, multigrid %d, %s" % (so[0]["pcg_iterations"], sg[0]["pcg_iterations"], shape))
    assert so[0]["solver_status"] == sg[0]["solver_status"] == 0
    assert shape.nl >= 2
    assert sg[0]["pcg_iterations"] * ITERATION_RATIO <= so[0]["pcg_iterations"]


# ---- a long free chain at match_passes = 1 ----------------------------------------------------------------------------------
_LONG_FREE = {}


def _long_free_chain():
    if not _LONG_FREE:
        g = chain(SE2, 12000, 11, closures=12)  # (long_se2 without its anchors: one fixed pose)
        _LONG_FREE["g"] = g
        _LONG_FREE["ref"] = PR.gauss_newton(SE2, g["poses"], g["ij"], g["Z"], 1, fixed_mask=g["fixed_mask"])[1]
    return _LONG_FREE["g"], _LONG_FREE["ref"]


@pytest.mark.parametrize("passes", [
    3, pytest.param(1, marks=pytest.mark.xfail(strict=True, reason=(
        "open: on this 12 000-pose chain with one fixed pose the ten-level match_passes = 1 hierarchy stalls PCG -- relative "
        "residual ~9e-5 after 20 000 iterations, poses 0.19 off -- and the solve still reports solver_status 0; "
        "match_passes = 3 converges in ~120 iterations on the same system")))])
def test_long_free_chain_converges(product, passes):
    g, ref = _long_free_chain()
    pg = product.PoseGraph(SE2)
    pg.set_tuning(match_passes=passes)
    pg.set_graph(g["poses"], g["ij"], g["Z"], fixed_mask=g["fixed_mask"])
    st = pg.solve(_params(1, pcg_max=3000))
    assert st[0]["solver_status"] == 0 and st[0]["pcg_iterations"] < 3000, st
    assert np.max(np.abs(pg.poses() - ref)) <= 1e-5


# ---- coverage of the branch table --------------------------------------------------------------------------------------------
TABLE = {"level0_coarsest", "stalled_dense", "stalled_smoothed", "lf0", "lf1", "lf2+", "lf_dense_level", "inverse_lds2",
         "inverse_lds1", "inverse_lds0", "fuse_last", "dense_bottom"}


def test_every_branch_is_hit_in_both_dimensions():
    """the labels the frozen catalogue shapes and the exact-preconditioner cases carry.  Each catalogue case asserts its shape
    on the GPU before its numbers, each exact case its level-0 shape and in_lds mode; the six-phase cycle, the chunks and
    the knobs have their own tests above"""
    for kind in KINDS:
        D = PR.dim(kind)
        hit = set()
        for (k, name), (_, labels) in EXPECT.items():
            if k == kind:
                hit |= labels
        hit |= {"inverse_lds%d" % m for k, _, m in EXACT.values() if k == kind}
        assert TABLE <= hit, (D, sorted(TABLE - hit))
