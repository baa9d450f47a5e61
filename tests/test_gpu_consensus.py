"""srrg2_consensus_compute on the GPU against tests/consensus_restatement.py: results, counters, offsets and inlier records bit for
bit, at the smallest shapes that can still go wrong (every tile, wave and workgroup size of csrc/consensus.hip: the constants of
tests/consensus_cases.py), every refusal with the outputs untouched, and the HBST detector with and without the verification on
a closure met from the opposite direction with 60 % wrong matches."""
import ctypes as C

import numpy as np
import pytest

import consensus_cases as cc
import consensus_restatement as cr
import hbst_restatement as hr
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import consensus as cn
from srrg2_slam_interfaces_amd import loop_detector as ld
from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu

FIELDS = ("status", "best_hypothesis", "num_inliers", "num_pairs", "num_valid_pairs", "num_degenerate", "num_rejected", "num_scored",
          "cost_exponent", "cost")
SMALL = cc.small_cases()


@pytest.fixture(scope="module")
def verifiers(product):
    """one handle per dim for the whole module: every test is also a test of workspace reuse"""
    v = {2: product.ConsensusVerifier(2), 3: product.ConsensusVerifier(3)}
    yield v
    for x in v.values():
        x.close()


def _same(got, want, where=""):
    assert len(got) == len(want), where
    for k, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert g[f] == w[f], (where, k, f, g[f], w[f])
        assert g["moving_in_fixed"].tobytes() == w["moving_in_fixed"].tobytes(), (where, k, g["moving_in_fixed"], w["moving_in_fixed"])
        assert g["inliers"].tobytes() == w["inliers"].tobytes(), (where, k)


def _check(verifiers, c, **extra):
    p = dict(c["params"], **extra)
    want = cr.consensus(c["dim"], c["fixed"], c["movings"], c["corrs"], **p)
    got = verifiers[c["dim"]].compute(c["fixed"], c["movings"], c["corrs"], **p)
    _same(got, want, str(p))
    return got, want


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_cases(name, verifiers):
    """N below, at and above the sample size, duplicates (the lowest h wins), e == tau^2 exactly, collinear and too-close samples,
    length_check 0 and 1, non-finite points and out-of-range indices, min_inliers above the count, K = 5 with an empty and an
    all-invalid candidate in the middle; dim 2 and dim 3 (tests/test_consensus_restatement.py checks that each case exercises
    what its name says)"""
    got, _ = _check(verifiers, SMALL[name])
    c = SMALL[name]
    if len(c["movings"]) > 1:  # result k of a batch is the result of a K = 1 call on candidate k alone
        for k in range(len(c["movings"])):
            one = verifiers[c["dim"]].compute(c["fixed"], [c["movings"][k]], [c["corrs"][k]], **c["params"])
            _same(one, [got[k]], "K = 1, candidate %d" % k)


@pytest.mark.parametrize("dim", [2, 3])
def test_pair_counts_at_every_tile_edge(dim, verifiers):
    """N one below, at and one past WAVE, BLOCK, SCORE_TILE and SCAN_TILE: one batch with a candidate per size (its total crosses
    the scan's second level), then the largest alone"""
    movings, corrs = [], []
    fixed = None
    for n in cc.PAIR_EDGES:
        f, m, c, _, _ = cc.planted(40, dim, cc.PAIR_EDGES[-1], 0.5)
        fixed = f
        movings.append(m)
        corrs.append(c[:n])
    case = cc.case(dim, fixed, movings, corrs, num_hypotheses=48, seed=9)
    got, _ = _check(verifiers, case)
    assert [g["num_pairs"] for g in got] == cc.PAIR_EDGES and all(g["status"] == abi.CONSENSUS_FOUND for g in got)
    _check(verifiers, cc.case(dim, fixed, movings[-1:], corrs[-1:], num_hypotheses=48, seed=9))


@pytest.mark.parametrize("H", cc.HYPOTHESIS_EDGES)
def test_hypothesis_counts_at_every_chunk_edge(H, verifiers):
    """H = 1, 1 000 and one below, at and one past SCORE_CHUNK, WAVE and the hypothesis kernel's BLOCK; without the length check
    every sampled hypothesis is scored, so the survivor count crosses the same edges"""
    for dim in (2, 3):
        f, m, c, _, _ = cc.planted(41 + dim, dim, 150, 0.5)
        for lc in (0, 1):
            got, _ = _check(verifiers, cc.case(dim, f, [m], [c], num_hypotheses=H, seed=H, length_check=lc))
            assert got[0]["num_degenerate"] + got[0]["num_rejected"] + got[0]["num_scored"] == H


def test_largest_shape(verifiers):
    """5 000 pairs x 1 024 hypotheses, 60 % wrong, three candidates of different sizes; and 2 500 pairs with every hypothesis scored"""
    movings, corrs = [], []
    for k, n in enumerate((5000, 3000, 4097)):
        f, m, c, _, _ = cc.planted(50, 3, 5000, 0.6)
        movings.append(m)
        corrs.append(c[:n])
    got, _ = _check(verifiers, cc.case(3, f, movings, corrs, num_hypotheses=1024, seed=3))
    assert all(g["status"] == abi.CONSENSUS_FOUND and g["num_rejected"] > 800 for g in got)
    _check(verifiers, cc.case(3, f, movings[:1], [corrs[0][:2500]], num_hypotheses=1024, seed=4, length_check=0))


def test_k_zero(verifiers, product):
    assert verifiers[3].compute(np.zeros((4, 3), np.float32), [], []) == []
    res, inl, offs = verifiers[3].compute_raw(None, 12, 0, None, 12, np.zeros(1, np.int32), abi.MEM_HOST, np.zeros(0, cn.CORR_DTYPE),
                                             np.zeros(1, np.int32), verifiers[3].params())
    assert len(res) == 0 and len(inl) == 0 and offs.tolist() == [0]


def _device_copy(lib, a):
    lib.srrg2_amd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.srrg2_amd_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.srrg2_amd_device_free.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert lib.srrg2_amd_device_malloc(C.c_size_t(max(a.nbytes, 16)), C.byref(p)) == 0
    assert lib.srrg2_amd_memcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1, None) == 0
    return p


@pytest.mark.parametrize("dim", [2, 3])
def test_strides_memories_and_scenes(dim, verifiers, product):
    """strides 12 and 16 (dim 2: 8, 12 and 16), host and device memory, scenes: the same bits every way"""
    c = cc.batch5(dim, seed=12)
    want = cr.consensus(dim, c["fixed"], c["movings"], c["corrs"], **c["params"])
    v = verifiers[dim]
    lib = v._lib
    for cols in ([2, 3, 4] if dim == 2 else [3, 4]):
        pad = lambda a: np.ascontiguousarray(np.concatenate([a[:, :dim], np.full((len(a), cols - dim), 7.0, np.float32)], 1))  # noqa: E731
        f, ms = pad(c["fixed"]), [pad(m) for m in c["movings"]]
        _same(v.compute(f, ms, c["corrs"], **c["params"]), want, "host, stride %d" % (4 * cols))
        moff = np.zeros(len(ms) + 1, np.int32)
        moff[1:] = np.cumsum([len(m) for m in ms])
        coff = np.zeros(len(ms) + 1, np.int32)
        coff[1:] = np.cumsum([len(x) for x in c["corrs"]])
        df, dm = _device_copy(lib, f), _device_copy(lib, np.concatenate(ms))
        try:
            raw = v.compute_raw(df.value, 4 * cols, len(f), dm.value, 4 * cols, moff, abi.MEM_DEVICE, np.concatenate(c["corrs"]), coff,
                                v.params(**c["params"]))
            _same(v._unpack(*raw), want, "device, stride %d" % (4 * cols))
        finally:
            lib.srrg2_amd_device_free(df)
            lib.srrg2_amd_device_free(dm)
    b = product.scene_binding(0)
    scenes = []
    for a in [c["fixed"]] + [m if len(m) else c["fixed"][:1] for m in c["movings"]]:  # (a candidate without pairs: any cloud)
        s = mapping.Scene(b, dim)
        s.set(a)
        scenes.append(s)
    _same(v.compute(scenes[0], scenes[1:], c["corrs"], **c["params"]), want, "scenes")
    with pytest.raises(ValueError):
        v.compute(scenes[0], c["movings"], c["corrs"])


def test_capacity_and_null_outputs(verifiers):
    """inlier_capacity below the count: the first records arrive, the offsets are not limited; inliers_out NULL; capacity 0"""
    c = cc.batch5(3, seed=13)
    want = cr.consensus(3, c["fixed"], c["movings"], c["corrs"], **c["params"])
    all_inl = np.concatenate([w["inliers"] for w in want])
    offsets = np.concatenate([[0], np.cumsum([len(w["inliers"]) for w in want])])
    v = verifiers[3]
    f, m = c["fixed"], np.concatenate(c["movings"])
    moff = np.concatenate([[0], np.cumsum([len(x) for x in c["movings"]])]).astype(np.int32)
    coff = np.concatenate([[0], np.cumsum([len(x) for x in c["corrs"]])]).astype(np.int32)
    recs = np.concatenate(c["corrs"])
    for cap, want_inliers in ((len(all_inl) // 2, True), (0, True), (len(recs), False), (len(recs), True)):
        res, inl, offs = v.compute_raw(f.ctypes.data, 12, len(f), m.ctypes.data, 12, moff, abi.MEM_HOST, recs, coff, v.params(**c["params"]),
                                       capacity=cap, want_inliers=want_inliers)
        assert offs.tolist() == offsets.tolist()
        assert inl.tobytes() == (all_inl[:cap].tobytes() if want_inliers else b"")
        assert [int(r["num_inliers"]) for r in res] == [w["num_inliers"] for w in want]


def test_two_different_calls_on_one_handle(product):
    """workspace reuse: a large call, a small one of the other shape, the large one again, on a fresh handle"""
    v = product.ConsensusVerifier(3)
    big, small = cc.basic(3, seed=21, n=3000, H=512), SMALL["dim3_batch5"]
    want_big = cr.consensus(3, big["fixed"], big["movings"], big["corrs"], **big["params"])
    want_small = cr.consensus(3, small["fixed"], small["movings"], small["corrs"], **small["params"])
    for c, want in ((big, want_big), (small, want_small), (big, want_big), (small, want_small)):
        _same(v.compute(c["fixed"], c["movings"], c["corrs"], **c["params"]), want)
    v.close()


def test_refusals_leave_the_outputs_untouched(verifiers, product):
    c = SMALL["dim3_batch5"]
    v = verifiers[3]
    lib = v._lib
    K = len(c["movings"])
    f, m = c["fixed"], np.concatenate(c["movings"])
    moff = np.concatenate([[0], np.cumsum([len(x) for x in c["movings"]])]).astype(np.int32)
    coff = np.concatenate([[0], np.cumsum([len(x) for x in c["corrs"]])]).astype(np.int32)
    recs = np.concatenate(c["corrs"])
    good = dict(h=v._h, fixed=f.ctypes.data, fstride=12, nf=len(f), K=K, moving=m.ctypes.data, mstride=12, moff=moff, mem=abi.MEM_HOST,
                recs=recs.ctypes.data, coff=coff, params=v.params(**c["params"]), results=True, cap=len(recs))

    def call(**change):
        a = dict(good, **change)
        res = np.full(K * 96, 0xAB, np.uint8)
        inl = np.full(len(recs) * 12, 0xAB, np.uint8)
        offs = np.full(K + 1, -77, np.int64)
        rc = lib.srrg2_consensus_compute(
            a["h"], a["fixed"], a["fstride"], a["nf"], a["K"], a["moving"], a["mstride"],
            None if a["moff"] is None else a["moff"].ctypes.data_as(C.POINTER(C.c_int32)), a["mem"], a["recs"],
            None if a["coff"] is None else a["coff"].ctypes.data_as(C.POINTER(C.c_int32)),
            None if a["params"] is None else C.byref(a["params"]), res.ctypes.data if a["results"] else None, inl.ctypes.data,
            C.c_int64(a["cap"]), offs.ctypes.data_as(C.POINTER(C.c_int64)))
        untouched = (res == 0xAB).all() and (inl == 0xAB).all() and (offs == -77).all()
        return rc, untouched

    assert call()[0] == 0
    INVALID = -1
    bad_params = [dict(num_hypotheses=0), dict(num_hypotheses=65537), dict(inlier_distance=0.0), dict(inlier_distance=-1.0),
                  dict(inlier_distance=float("nan")), dict(inlier_distance=float("inf")), dict(min_sample_distance=-0.1),
                  dict(min_sample_distance=float("nan")), dict(min_sample_distance=float("inf")), dict(min_inliers=-1),
                  dict(length_check=2), dict(length_check=-1), dict(reserved=(1, 0)), dict(reserved=(0, 1))]
    down = moff.copy()
    down[2] = down[1] - 1
    cdown = coff.copy()
    cdown[-1] = cdown[-2] - 1
    refusals = [dict(h=None), dict(params=None), dict(results=False), dict(K=-1), dict(moff=down), dict(coff=cdown), dict(moff=None),
                dict(coff=None), dict(fixed=None), dict(moving=None), dict(recs=None), dict(fstride=8), dict(fstride=14), dict(mstride=8),
                dict(mstride=18), dict(cap=-1), dict(mem=abi.MEM_DEVICE_KEPT), dict(mem=5), dict(nf=-1)]
    refusals += [dict(params=v.params(**dict(c["params"], **b))) for b in bad_params]
    for change in refusals:
        rc, untouched = call(**change)
        assert rc == INVALID and untouched, change
        assert lib.srrg2_amd_last_error()
    assert call()[0] == 0  # the handle is as it was
    with pytest.raises(RuntimeError):
        product.ConsensusVerifier(4)
    with pytest.raises(RuntimeError):
        product.ConsensusVerifier(3, device=4096)
    with pytest.raises(TypeError):
        v.compute(f, c["movings"], c["corrs"], no_such_parameter=1)


def test_defaults(verifiers):
    p = cn.default_params()
    assert (p.num_hypotheses, p.min_inliers, p.seed, p.length_check, p.reserved[0], p.reserved[1]) == (256, 0, 0, 1, 0, 0)
    assert p.inlier_distance == np.float32(0.05) and p.min_sample_distance == np.float32(0.1)
    assert {k: getattr(p, k) for k in cr.DEFAULTS} == {k: (np.float32(x) if isinstance(x, float) else x) for k, x in cr.DEFAULTS.items()}


# ---- end to end: the world of tests/test_hbst_detector_end_to_end.py, one candidate met from the opposite direction with 60 % of
# ---- its matches made wrong

def _aligner(make):
    al = make(abi.SE3_QUAT_RIGHT)
    al.set_params(max_iterations=15)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind = abi.SLICE_P2P
    c.finder = abi.FINDER_CORRESPONDENCES
    c.robustifier = abi.ROBUST_CAUCHY
    c.robustifier_chi_threshold = 0.05
    al.add_slice(c)
    return al


def _apply(T, P):
    return (P @ T[:, :3].T + T[:, 3]).astype(np.float32)


def _world(seed):
    """landmarks, their descriptors, five reference local maps (graph ids 100 .. 104) and the query (graph id 200); map 101 is met
    from the opposite direction (180 degrees of yaw)"""
    rng = np.random.default_rng(seed)
    N = 8000
    W = rng.uniform(-5, 5, (N, 3))
    D = hr.random_descriptors(rng, N)
    query_pose = syn.se3(rng.uniform(-0.2, 0.2, 3), np.deg2rad(rng.uniform(-5, 5, 3)))
    maps = []
    plan = [(range(0, 2000), range(0, 1500), 1, False),  # 100: a closure
            (range(2000, 4000), range(2000, 3800), 1, False),  # 101: a closure, opposite direction, 60 % wrong matches (below);
            # the query sees 1 800 of its landmarks, so that the 40 % true matches still pass relocalize_min_inliers = 500
            (list(range(4000, 4300)) + list(range(7300, 8000)), range(4000, 4300), 2, False),  # 102: too few after dedup
            (range(4300, 5800), range(4300, 5800), 1, True),  # 103: too noisy (the geometry disagrees)
            (range(5800, 7300), range(5800, 7300), 1, False)]  # 104: too young
    q_lm = []
    for k, (own, seen, times, scramble) in enumerate(plan):
        rpy = np.deg2rad(rng.uniform(-20, 20, 3))
        if k == 1:
            rpy[2] = np.pi
        pose = syn.se3(rng.uniform(-1, 1, 3), rpy)
        own = np.array(list(own))
        P = _apply(syn.se3_inv(pose), W[own])
        if scramble:
            P = rng.uniform(-5, 5, P.shape).astype(np.float32)
        maps.append(dict(graph_id=100 + k, points=P, descriptors=D[own].copy(), X_gt=syn.se3_mul(syn.se3_inv(query_pose), pose)))
        q_lm += list(seen) * times
    q_lm = np.array(q_lm)
    n_out = 500
    Q = np.concatenate([_apply(syn.se3_inv(query_pose), W[q_lm]), rng.uniform(-5, 5, (n_out, 3)).astype(np.float32)])
    Q = Q + rng.normal(scale=0.002, size=Q.shape).astype(np.float32)
    QD = np.concatenate([np.stack([hr.flip_bits(rng, D[i], int(rng.integers(0, 9))) for i in q_lm]), hr.random_descriptors(rng, n_out)])
    perm = rng.permutation(len(Q))
    valid = (rng.random(len(Q)) < 0.97).astype(np.uint8)
    return maps, dict(graph_id=200, points=Q[perm].astype(np.float32), descriptors=QD[perm], valid=valid)


def _candidates(product, maps, q):
    """the detector's own matches, with 60 % of candidate 101's made wrong (their moving index moved to another point of the map)"""
    det = ld.MultiLoopDetectorHBST(_aligner(product.MultiAligner), relocalize_min_inliers=500, minimum_age_difference_to_candidates=1)
    for m in maps:
        det.compute_correspondences(m["graph_id"], m["descriptors"], None, m["points"])
        det.add_previous_query()
    det.compute_correspondences(q["graph_id"], q["descriptors"], q["valid"], q["points"])
    cands = []
    rng = np.random.default_rng(5)
    for r in det.indices():
        corr = det.correspondences(r).copy()
        if det.graph_id(r) == 101:
            wrong = rng.random(len(corr)) < 0.6
            corr["moving_idx"][wrong] = (corr["moving_idx"][wrong] + rng.integers(1, 2000, int(wrong.sum()))) % 2000
        cands.append(dict(reference=det.graph_id(r), moving=maps[r]["points"], moving_normals=None, correspondences=corr))
    return cands


def _detector(product, **kw):
    return ld.MultiLoopDetectorHBST(_aligner(product.MultiAligner), relocalize_min_inliers=500, relocalize_max_chi_inliers=0.005,
                                    minimum_age_difference_to_candidates=1, **kw)


def test_detector_finds_the_opposite_direction_closure_only_with_consensus(product, oracle):
    maps, q = _world(31)
    cands = _candidates(product, maps, q)
    assert [c["reference"] for c in cands] == [100, 101, 102, 103]
    n101 = len(cands[1]["correspondences"])
    # without the verification: today's behaviour, and the closure is lost
    plain = _detector(product, relocalize_min_inliers_ratio=0.7)
    closures = plain.compute_alignments(200, q["points"], None, cands)
    assert [c["target"] for c in closures] == [100]
    assert dict(plain.drops)[101] != "" and set(dict(plain.drops)) == {101, 102, 103}
    loose = _detector(product, relocalize_min_inliers_ratio=0.3)  # (not the ratio gate alone: the solve itself fails)
    assert [c["target"] for c in loose.compute_alignments(200, q["points"], None, cands)] == [100]
    assert 101 in dict(loose.drops)
    det = _detector(product, relocalize_min_inliers_ratio=0.3, consensus=dict(seed=1))
    closures = det.compute_alignments(200, q["points"], None, cands)
    assert [c["target"] for c in closures] == [100, 101]
    c101 = closures[1]
    assert np.max(np.abs(c101["measurement"] - maps[1]["X_gt"])) < 5e-3
    assert c101["num_matches"] == n101 and c101["num_correspondences"] == len(c101["correspondences"]) < 0.5 * n101
    assert c101["num_inliers"] / c101["num_matches"] >= 0.3
    drops = dict(det.drops)
    assert drops[102] == "ALIGNER DROP [code: %d]" % abi.NOT_ENOUGH_CORRESPONDENCES
    assert drops[103].startswith("CONSENSUS DROP [code: ") and set(drops) == {102, 103}
    # the ratio gate is taken against the ORIGINAL count: at 0.7 the verified closure is still refused
    strict = _detector(product, relocalize_min_inliers_ratio=0.7, consensus=dict(seed=1))
    assert [c["target"] for c in strict.compute_alignments(200, q["points"], None, cands)] == [100]
    assert dict(strict.drops)[101] == "MIN_INLIERS_RATIO DROP"
    # candidate 100 comes out as it does today: the same closure within the solve's own convergence
    assert np.max(np.abs(closures[0]["measurement"] - maps[0]["X_gt"])) < 5e-3
    assert np.max(np.abs(closures[0]["measurement"] - plain.detected_closures[0]["measurement"])) < 5e-3
    # the batched solve is the oracle aligner's, given the same guess and inlier list
    assert len(det.last_consensus) == 3
    for closure, r in zip(closures, [det.last_consensus[0], det.last_consensus[1]]):
        ref = _aligner(oracle.OracleAligner)
        ref.set_fixed(0, q["points"], None)
        ref.set_moving(0, maps[closure["target"] - 100]["points"], None)
        ref.set_correspondences(0, r["inliers"])
        ref.set_moving_in_fixed(r["moving_in_fixed"])
        assert ref.compute() == abi.SUCCESS
        assert ref.moving_in_fixed().tobytes() == closure["measurement"].tobytes()
        assert closure["correspondences"].tobytes() == r["inliers"].tobytes()


def test_detector_with_scenes(product):
    """the same verification with every cloud a device-resident scene"""
    maps, q = _world(31)
    cands = _candidates(product, maps, q)
    b = product.scene_binding(0)

    def scene(points):
        s = mapping.Scene(b, 3)
        s.set(points)
        return s

    host = _detector(product, relocalize_min_inliers_ratio=0.3, consensus=dict(seed=1))
    want = host.compute_alignments(200, q["points"], None, cands)
    dev = _detector(product, relocalize_min_inliers_ratio=0.3, consensus=dict(seed=1))
    got = dev.compute_alignments(200, scene(q["points"]), None, [dict(c, moving=scene(c["moving"])) for c in cands])
    assert [c["target"] for c in got] == [c["target"] for c in want] == [100, 101]
    for a, w in zip(got, want):
        assert a["measurement"].tobytes() == w["measurement"].tobytes() and a["correspondences"].tobytes() == w["correspondences"].tobytes()
    assert dev.drops == host.drops
