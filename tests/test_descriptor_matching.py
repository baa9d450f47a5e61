"""The matching half of MultiLoopDetectorHBST_ (multi_loop_detector_hbst_impl.cpp:41-197): CPU legs pin the numpy
restatement (tests/hbst_restatement.py) on hand-built cases and check the Python arguments; gpu legs compare the
device database (srrg2_descriptor_db_*) with the restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hbst_restatement as hr
from srrg2_slam_interfaces_amd import descriptors as dd
from srrg2_slam_interfaces_amd import loop_detector as ld


def _with_distance(rng, base, k):
    return hr.flip_bits(rng, base, k)


# ---- the restatement on hand-built cases -----------------------------------------------------------------------------
def test_distance_at_the_threshold_is_strict():
    rng = np.random.default_rng(1)
    ref = hr.random_descriptors(rng, 1)
    db = hr.RestatedDatabase()
    db.add(ref)
    for k, thr, hit in [(24, 25, True), (25, 25, False), (24, 25.0, True), (25, 25.0, False), (24, 24.5, True),
                        (25, 25.5, True), (0, 0.0, False), (0, 1e-6, True), (256, 256.0, False), (256, 257, True),
                        (255, 257, True)]:
        q = _with_distance(rng, ref[0], k)[None]
        assert hr.hamming(q, ref)[0, 0] == k
        res = db.match(q, query_index=5, max_distance=thr)
        assert (res["indices"] == [0]) == hit, (k, thr)
        if hit:
            c = res["correspondences"][0]
            assert c.tolist() == [(0, 0, float(k))]


def test_ties_keep_the_lower_query_index_and_the_smaller_distance_wins():
    rng = np.random.default_rng(2)
    ref = hr.random_descriptors(rng, 2)
    db = hr.RestatedDatabase()
    db.add(ref)
    a = _with_distance(rng, ref[0], 7)
    q = np.stack([hr.random_descriptors(rng, 1)[0], a, a.copy(), _with_distance(rng, ref[1], 9),
                  _with_distance(rng, ref[1], 3), _with_distance(rng, ref[1], 3)])
    res = db.match(q, query_index=1)
    c = res["correspondences"][0]
    assert c.tolist() == [(1, 0, 7.0), (4, 1, 3.0)]
    assert res["num_matches"] == [5]


def test_one_query_matches_several_reference_descriptors():
    rng = np.random.default_rng(3)
    base = hr.random_descriptors(rng, 1)[0]
    ref = np.stack([_with_distance(rng, base, k) for k in (2, 30, 5, 11)])
    db = hr.RestatedDatabase()
    db.add(ref)
    res = db.match(base[None], query_index=1)
    assert res["correspondences"][0].tolist() == [(0, 0, 2.0), (0, 2, 5.0), (0, 3, 11.0)]


def test_invalid_points_keep_their_indices():
    rng = np.random.default_rng(4)
    ref = hr.random_descriptors(rng, 6)
    valid_ref = np.array([0, 1, 0, 1, 1, 0], np.uint8)
    db = hr.RestatedDatabase()
    assert db.add(ref, valid_ref) == 0
    q = np.stack([_with_distance(rng, ref[i], 1) for i in range(6)])
    valid_q = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    res = db.match(q, valid_q, query_index=1)
    # ref 3 is only matched by query 3, which is invalid; ref 0, 2, 5 are not in the database
    assert res["correspondences"][0].tolist() == [(1, 1, 1.0), (4, 4, 1.0)]


def test_count_gate_is_strict_on_the_pairs_before_deduplication():
    rng = np.random.default_rng(5)
    ref = hr.random_descriptors(rng, 3)
    db = hr.RestatedDatabase()
    db.add(ref)
    q = np.stack([_with_distance(rng, ref[0], 1), _with_distance(rng, ref[0], 2), _with_distance(rng, ref[1], 1)])
    # 3 pairs, 2 correspondences after deduplication
    assert db.match(q, query_index=1, min_matches=3)["indices"] == []
    res = db.match(q, query_index=1, min_matches=2)
    assert res["indices"] == [0] and res["num_matches"] == [3] and len(res["correspondences"][0]) == 2
    assert db.match(q, query_index=1, min_matches=3)["map_counts"] == {0: 3}


def test_age_gate_with_the_unsigned_wrap():
    rng = np.random.default_rng(6)
    db = hr.RestatedDatabase()
    maps = [hr.random_descriptors(rng, 4) for _ in range(6)]
    for m in maps:
        db.add(m)
    q = np.concatenate([np.stack([_with_distance(rng, m[0], 2)]) for m in maps])
    # query index 3: maps 0..5; min_age 1 -> 3 - r > 1 for r in {0, 1}; r = 2, 3 fail; r = 4, 5 wrap and pass
    res = db.match(q, query_index=3, min_age=1)
    assert res["indices"] == [0, 1, 4, 5]
    assert res["map_counts"] == {0: 1, 1: 1, 2: -1, 3: -1, 4: 1, 5: 1}
    # min_age 0: only r == q fails
    assert db.match(q, query_index=3, min_age=0)["indices"] == [0, 1, 2, 4, 5]
    assert not hr.age_gate_passes(3, 3, 0) and hr.age_gate_passes(3, 4, 10 ** 9) and hr.age_gate_passes(3, 1, 1)
    assert not hr.age_gate_passes(3, 2, 1)
    # a new map (index 6) with min_age 2: r < 4 pass
    assert db.match(q, min_age=2)["indices"] == [0, 1, 2, 3]


def test_skipped_adds_and_a_requeried_graph_id():
    """addPreviousQuery skips a registered graph id and a map without valid descriptors (:46-56); a registered map is
    queried with its own index (:124-128), so it never matches itself"""
    rng = np.random.default_rng(7)
    db = hr.RestatedDatabase()
    a = hr.random_descriptors(rng, 5)
    assert db.add(a) == 0
    assert db.add(a, np.zeros(5, np.uint8)) == -1
    assert db.add(np.zeros((0, 32), np.uint8)) == -1
    b = hr.random_descriptors(rng, 5)
    assert db.add(b) == 1
    res = db.match(a, query_index=0)  # map 0 queried again: itself is gated out, map 1 (r > q) passes
    assert res["map_counts"] == {0: -1, 1: 0}
    res = db.match(np.concatenate([a, b]), query_index=0)
    assert res["indices"] == [1] and res["correspondences"][0]["fixed_idx"].tolist() == [5, 6, 7, 8, 9]


def test_detector_requeried_graph_id_and_skips_on_the_host_logic():
    """the graph id -> index bookkeeping of the detector (host logic), with a fake database"""

    class FakeDB:
        def __init__(self):
            self.ref = hr.RestatedDatabase()
            self.queries = []

        def add(self, d, v):
            return self.ref.add(d, v)

        def match(self, d, v, query_index, max_distance, min_age, min_matches):
            self.queries.append(query_index)
            r = self.ref.match(d, v, query_index, max_distance, min_age, min_matches)
            return dd.MatchResult(np.array(r["indices"], np.int32), np.array(r["num_matches"], np.int64),
                                  r["correspondences"], np.array([r["map_counts"][k] for k in sorted(r["map_counts"])]),
                                  0.0)

    rng = np.random.default_rng(8)
    det = ld.MultiLoopDetectorHBST(object(), relocalize_min_inliers=0, database=FakeDB())
    a, b = hr.random_descriptors(rng, 4), hr.random_descriptors(rng, 4)
    det.compute_correspondences(10, a)
    assert det.add_previous_query() == 0
    det.compute_correspondences(10, a)  # the same graph id: query index 0, not added again
    assert det.add_previous_query() == -1
    det.compute_correspondences(11, b, np.zeros(4, np.uint8))  # nothing valid: not added
    assert det.add_previous_query() == -1
    det.compute_correspondences(12, np.concatenate([b, a]))
    assert det.indices() == [0] and det.correspondences(0)["fixed_idx"].tolist() == [4, 5, 6, 7]
    assert det.add_previous_query() == 1
    assert det.database.queries == [0, 0, 1, 1]
    assert det.graph_id(1) == 12


# ---- Python arguments (no device) ------------------------------------------------------------------------------------
def test_python_argument_checks():
    with pytest.raises(ValueError):
        dd.as_descriptors(np.zeros((3, 31), np.uint8))
    with pytest.raises(ValueError):
        dd.as_descriptors(np.zeros((3, 8), np.float32))
    assert dd.as_descriptors(np.zeros((3, 4), np.uint64)).shape == (3, 32)
    with pytest.raises(ValueError):
        dd.as_valid(np.ones(4), 3)
    with pytest.raises(ValueError):
        dd.check_match_args(float("nan"), 0, 0)
    with pytest.raises(ValueError):
        dd.check_match_args(25.0, -1, 0)
    with pytest.raises(ValueError):
        dd.check_match_args(25.0, 0, -1)
    with pytest.raises(NotImplementedError, match="unsupported"):
        ld.MultiLoopDetectorHBST(object(), maximum_distance_for_merge=1.0)
    with pytest.raises(ValueError):
        ld.MultiLoopDetectorHBST(object(), maximum_descriptor_distance=float("nan"))
    det = ld.MultiLoopDetectorHBST(object(), maximum_leaf_size=7, maximum_partitioning=0.5, maximum_depth=3)
    assert det.database is None  # created at the first query only
    with pytest.raises(ValueError):
        det.compute_correspondences(0, np.zeros((2, 16), np.uint8))
    assert det.compute_correspondences(0, np.zeros((0, 32), np.uint8)) == []  # an empty query needs no database
    assert det.add_previous_query() == -1


def test_the_c_abi_refuses_without_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    from srrg2_slam_interfaces_amd import _capi

    h = C.c_void_p()
    assert _capi.lib().srrg2_descriptor_db_create(0, C.byref(h)) == -2  # SRRG2_E_NO_DEVICE
    with pytest.raises(RuntimeError, match="no HIP device"):
        dd.DescriptorDatabase()


# ---- device vs restatement -------------------------------------------------------------------------------------------
def assert_same(res, ref, maps=None):
    assert res.indices.tolist() == ref["indices"]
    assert res.num_matches.tolist() == ref["num_matches"]
    assert len(res.correspondences) == len(ref["correspondences"])
    for a, b in zip(res.correspondences, ref["correspondences"]):
        assert a.tobytes() == b.tobytes()
    if maps is None:
        assert len(res.map_counts) == len(ref["map_counts"])
    keys = sorted(ref["map_counts"]) if maps is None else sorted(maps)
    assert [int(res.map_counts[k]) for k in keys] == [ref["map_counts"][k] for k in keys]


def _planted_query(rng, maps, nq, share=0.3, max_flips=30):
    """nq query descriptors: a share are near-duplicates of random database descriptors (0 .. max_flips bits), some of
    them twice (ties), the rest random"""
    q = hr.random_descriptors(rng, nq)
    flat = np.concatenate([m for m in maps if len(m)]) if any(len(m) for m in maps) else np.zeros((0, 32), np.uint8)
    if len(flat) and nq:
        pick = rng.random(nq) < share
        src = rng.integers(0, len(flat), nq)
        for i in np.nonzero(pick)[0]:
            q[i] = hr.flip_bits(rng, flat[src[i]], int(rng.integers(0, max_flips + 1)))
        dup = np.nonzero(pick)[0]
        for i in dup[: len(dup) // 8]:
            q[rng.integers(0, nq)] = q[i]
    return q


def _both(product, maps, valids=None):
    db = product.DescriptorDatabase()
    ref = hr.RestatedDatabase()
    for i, m in enumerate(maps):
        v = None if valids is None else valids[i]
        assert db.add(m, v) == ref.add(m, v)
    return db, ref


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 20000])
def test_gpu_random_maps_and_query_sizes(product, nq):
    rng = np.random.default_rng(100 + nq)
    sizes = [0, 1, 63, 64, 65, 1000, 5000] if nq < 20000 else [0, 1, 63, 64, 65, 1000]
    maps = [hr.random_descriptors(rng, s) for s in sizes]
    db, ref = _both(product, maps)
    assert db.size() == (len(ref.maps), sum(len(m[0]) for m in ref.maps))
    q = _planted_query(rng, maps, nq)
    valid = (rng.random(nq) < 0.9).astype(np.uint8)
    for kw in [dict(max_distance=25.0, min_age=0, min_matches=0), dict(max_distance=40.0, min_age=1, min_matches=3),
               dict(max_distance=12.5, min_age=0, min_matches=1, query_index=2)]:
        assert_same(db.match(q, valid, **kw), ref.match(q, valid, **kw))


@pytest.mark.gpu
def test_gpu_thresholds_at_the_edges(product):
    rng = np.random.default_rng(21)
    maps = [hr.random_descriptors(rng, 300) for _ in range(3)]
    db, ref = _both(product, maps)
    q = _planted_query(rng, maps, 500, share=0.6, max_flips=40)
    for t in [0.0, -1.0, 1e-6, 24.0, 24.5, 25.0, 25.5, 128.0, 255.5, 256.0, 257.0, float("inf"), float("-inf")]:
        assert_same(db.match(q, max_distance=t), ref.match(q, max_distance=t))


@pytest.mark.gpu
def test_gpu_all_invalid_and_empty(product):
    rng = np.random.default_rng(22)
    maps = [hr.random_descriptors(rng, 100) for _ in range(3)]
    valids = [None, np.zeros(100, np.uint8), (rng.random(100) < 0.5).astype(np.uint8)]
    db, ref = _both(product, maps, valids)
    assert len(db) == 2
    q = _planted_query(rng, maps, 300, share=0.8)
    assert_same(db.match(q, np.zeros(300, np.uint8)), ref.match(q, np.zeros(300, np.uint8)))
    assert_same(db.match(np.zeros((0, 32), np.uint8)), ref.match(np.zeros((0, 32), np.uint8)))
    v = (rng.random(300) < 0.3).astype(np.uint8)
    assert_same(db.match(q, v), ref.match(q, v))
    empty = product.DescriptorDatabase()
    res = empty.match(q)
    assert len(res) == 0 and len(res.map_counts) == 0


@pytest.mark.gpu
def test_gpu_age_gate_and_requeried_index(product):
    rng = np.random.default_rng(23)
    maps = [hr.random_descriptors(rng, int(rng.integers(1, 200))) for _ in range(12)]
    db, ref = _both(product, maps)
    q = _planted_query(rng, maps, 800, share=0.9, max_flips=10)
    for qi in [0, 3, 11, 12, 40]:
        for age in [0, 1, 4, 11, 12, 2 ** 32 - 1]:
            kw = dict(query_index=qi, min_age=age, min_matches=2)
            assert_same(db.match(q, **kw), ref.match(q, **kw))


@pytest.mark.gpu
def test_gpu_grown_database_equals_one_built_at_once(product):
    rng = np.random.default_rng(24)
    maps = [hr.random_descriptors(rng, int(rng.integers(0, 120))) for _ in range(300)]
    grown = product.DescriptorDatabase()
    ref = hr.RestatedDatabase()
    q = _planted_query(rng, maps, 600, share=0.7)
    for i, m in enumerate(maps):
        assert grown.add(m) == ref.add(m)
        if i % 50 == 49:  # matching in between growths
            assert_same(grown.match(q, min_matches=1), ref.match(q, min_matches=1))
    fresh = product.DescriptorDatabase()
    for m in maps:
        fresh.add(m)
    a, b = grown.match(q), fresh.match(q)
    assert_same(a, ref.match(q))
    assert a.map_counts.tobytes() == b.map_counts.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.correspondences, b.correspondences))


@pytest.mark.gpu
def test_gpu_two_handles_alive_at_once(product):
    rng = np.random.default_rng(25)
    m1 = [hr.random_descriptors(rng, 500) for _ in range(4)]
    m2 = [hr.random_descriptors(rng, 700) for _ in range(3)]
    d1, r1 = _both(product, m1)
    d2, r2 = _both(product, m2)
    q1, q2 = _planted_query(rng, m1, 1500, share=0.5), _planted_query(rng, m2, 900, share=0.5)
    a1, a2 = d1.match(q1), d2.match(q2)
    assert_same(a1, r1.match(q1))
    assert_same(a2, r2.match(q2))
    assert_same(d1.match(q2), r1.match(q2))


@pytest.mark.gpu
def test_gpu_error_codes(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    h = C.c_void_p()
    assert lib.srrg2_descriptor_db_create(10 ** 6, C.byref(h)) == -1
    assert lib.srrg2_descriptor_db_create(0, None) == -1
    assert lib.srrg2_descriptor_db_create(0, C.byref(h)) == 0
    q = np.zeros((4, 32), np.uint8)
    p = q.ctypes.data_as(C.POINTER(C.c_uint8))
    K = C.c_int()
    idx = C.c_int()
    assert lib.srrg2_descriptor_db_add(h, None, None, 3, C.byref(idx)) == -1
    assert lib.srrg2_descriptor_db_add(h, p, None, -1, C.byref(idx)) == -1
    assert lib.srrg2_descriptor_db_add(h, None, None, 0, C.byref(idx)) == 0 and idx.value == -1
    assert lib.srrg2_descriptor_db_add(h, p, None, 4, C.byref(idx)) == 0 and idx.value == 0
    assert lib.srrg2_descriptor_db_match(h, p, None, 4, 1, float("nan"), 0, 0, C.byref(K)) == -1
    assert lib.srrg2_descriptor_db_match(h, p, None, -1, 1, 25.0, 0, 0, C.byref(K)) == -1
    assert lib.srrg2_descriptor_db_match(h, None, None, 4, 1, 25.0, 0, 0, C.byref(K)) == -1
    assert lib.srrg2_descriptor_db_match(h, p, None, 4, -1, 25.0, 0, 0, C.byref(K)) == -1
    assert lib.srrg2_descriptor_db_match(h, p, None, 4, 1, 25.0, 0, -1, C.byref(K)) == -1
    big = np.zeros(((1 << 23) + 1, 32), np.uint8)  # one more than a query may hold
    assert lib.srrg2_descriptor_db_match(h, big.ctypes.data_as(C.POINTER(C.c_uint8)), None, len(big), 1, 25.0, 0, 0,
                                         C.byref(K)) == -1
    assert lib.srrg2_descriptor_db_match(h, p, None, 4, 1, 25.0, 0, 0, C.byref(K)) == 0 and K.value == 1
    n = C.c_int(0)
    buf = (C.c_int32 * 1)()
    assert lib.srrg2_descriptor_db_get_candidates(h, buf, None, None, C.byref(n)) == -1  # capacity 0 < 1
    n = C.c_int(1)
    assert lib.srrg2_descriptor_db_get_candidates(h, buf, None, None, C.byref(n)) == 0 and buf[0] == 0
    nc = C.c_int64(0)
    assert lib.srrg2_descriptor_db_get_correspondences(h, None, C.byref(nc)) == 0 and nc.value == 4
    assert lib.srrg2_descriptor_db_destroy(h) == 0
    assert lib.srrg2_descriptor_db_destroy(None) == 0
    with pytest.raises(ValueError):
        product.DescriptorDatabase().match(q, max_distance=float("nan"))


@pytest.mark.gpu
def test_gpu_full_size_sampled(product):
    """1 000 maps x 1 000 descriptors, a 2 000-descriptor query: the candidate list, every map's count on a sample and
    the correspondences of 16 sampled maps plus every candidate (maps are independent: a sample is exact)"""
    rng = np.random.default_rng(26)
    maps = [hr.random_descriptors(rng, 1000) for _ in range(1000)]
    db, ref = _both(product, maps)
    # closure-like query: 3 maps share many near-duplicates, 40 maps a few
    q = hr.random_descriptors(rng, 2000)
    slot = 0
    for r in (100, 500, 900):
        for j in rng.choice(1000, 300, replace=False):
            q[slot] = hr.flip_bits(rng, maps[r][j], int(rng.integers(0, 20)))
            slot += 1
    for r in rng.choice(1000, 40, replace=False):
        for j in rng.choice(1000, 5, replace=False):
            q[slot] = hr.flip_bits(rng, maps[r][j], int(rng.integers(0, 30)))
            slot += 1
    res = db.match(q, min_matches=50, min_age=10)
    cands = set(res.indices.tolist()) | {100, 500, 900}
    sample = set(rng.choice(1000, 16, replace=False).tolist()) | cands
    r = ref.match(q, min_matches=50, min_age=10, only_maps=sample)
    assert res.indices.tolist() == r["indices"] == [100, 500, 900]
    assert_same(res, r, maps=sample)
    assert int((res.map_counts == -1).sum()) == 10  # the ten newest maps (990 .. 999) are too young
