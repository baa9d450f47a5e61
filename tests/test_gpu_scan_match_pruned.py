"""GPU: pruned scan matching (csrc/scan_match.hip: srrg2_gridmap_build_bounds / _get_bounds / _match_scans_pruned) against the
numpy restatement of its contract (tests/scan_match_pruned_restatement.py), BIT FOR BIT: the bound planes, every member of every
result and every statistic; and against srrg2_gridmap_match_scans on the same handle and inputs, whose answer it has to give.  At
the smallest shapes where the kernels can go wrong (tests/scan_match_pruned_cases.py names them)."""
import ctypes as C
import math

import numpy as np
import pytest

import adaptor_restatement as ar
import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_cases as smc
import scan_match_pruned_cases as pc
import scan_match_pruned_restatement as sp
import scan_match_restatement as sm
from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID = -1
DEG = math.radians(1.0)


def _grid_of(product, g, sc):
    m = product.OccupancyGrid(0)
    m.reset(g["rows"], g["cols"], float(g["res"]), (float(g["ox"]), float(g["oy"])))
    m.set_scan_model(sc["angle_min"], sc["angle_increment"], sc["num_beams"], float(sc["range_min"]), float(sc["range_max"]),
                     sc["sensor_in_robot"], sc["clear_beyond_max"])
    return m


def _drawn(product, d, levels=4):
    m = _grid_of(product, d["g"], d["sc"])
    m.integrate(d["ranges"], d["poses"], want_result=False)
    m.build_likelihood(1, 50, d["R"], d["lut"])
    m.build_bounds(levels)
    return m


def _same(got, want, what=""):
    assert got["robot_in_world"].tobytes() == want["robot_in_world"].tobytes(), "pose " + what
    for k in pc.MEMBERS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), "%s %s: %s != %s" % (k, what, got[k], want[k])
    if "stats" in got and "stats" in want:
        assert len(got["stats"]) == len(want["stats"])
        for i, (a, b) in enumerate(zip(got["stats"], want["stats"])):
            for k in pc.STATS:
                assert a[k] == b[k], "stats[%d].%s %s: %s != %s" % (i, k, what, a[k], b[k])


def _check(m, field, scans, guesses, sc, g, window, step, levels, limit=0, planes=None, what=""):
    """one pruned call against the restatement (results and statistics) and against the exhaustive call on the same handle"""
    wx, wy, ht = window
    want = sp.match(field, scans, guesses, sc, g, wx, wy, ht, step, levels, limit, planes=planes)
    got = m.match_scans_pruned(scans, guesses, (wx, wy), ht, step, levels, limit, want_stats=True)
    what = "%s window %s levels %d limit %d" % (what, window, levels, limit)
    _same(got, want, what)
    _same(m.match_scans(scans, guesses, (wx, wy), ht, step), got, what + " (exhaustive)")
    return got


@pytest.fixture(scope="module")
def recovery(product):
    rm = smc.recovery_map()
    m = _grid_of(product, rm["g"], rm["sc"])
    m.integrate(rm["ranges"], rm["poses"], want_result=False)
    m.build_likelihood(1, 50, 4)
    m.build_bounds(6)
    assert np.array_equal(m.likelihood(), rm["field"])
    return m, rm


def test_bound_planes_bit_for_bit(recovery):
    m, rm = recovery
    planes = pc.recovery_planes()
    for l in range(1, 7):
        got = m.bounds(l)
        assert got.shape == (160 + 2 ** l - 1, 200 + 2 ** l - 1) and np.array_equal(got, planes[l]), l
    assert planes[6].max() == rm["field"].max() and (planes[1] != planes[2][2:, 2:]).any()


def test_recovery_trials(recovery):
    """trials 0 .. 9 as one batch, window 25 x 25 x 21 at 1 degree, levels 1 .. 4 (and 6: blocks wider than the window)"""
    m, rm = recovery
    truth, scans, guesses = pc.recovery_batch()
    for levels in (1, 2, 3, 4, 6):
        got = _check(m, rm["field"], scans, guesses, rm["sc"], rm["g"], (12, 12, 10), DEG, levels, planes=pc.recovery_planes())
        assert not any(s["fell_back"] for s in got["stats"]) and got["score"].min() > 0
        # (it pruned: bounds and scores together, with a whole seed block and the guess, are fewer than the candidates)
        assert max(sum(s["num_evaluated"]) for s in got["stats"]) + 4 ** levels + 1 < 25 * 25 * 21


@pytest.mark.parametrize("window", pc.BLOCK_EDGES, ids=str)
def test_block_edges(recovery, window):
    """windows that blocks tile exactly, with a hanging last block, and that one block covers and hangs over; half_steps_theta = 0"""
    m, rm = recovery
    truth, scans, guesses = pc.recovery_batch()
    near = np.stack([t @ gc.pose(0.11, -0.07, 0.02) for t in truth[:3]]).astype(F)
    for levels in (1, 2, 3, 4, 5):
        _check(m, rm["field"], scans[:3], near, rm["sc"], rm["g"], window, 0.02, levels, planes=pc.recovery_planes())


def test_grid_edges_and_an_empty_grid(product):
    """a 29 x 37-cell grid; guesses in a corner cell, on the border and outside, so that blocks reach negative cells and cells past
    cols / rows; blocks larger than the grid (levels 5 and 6)"""
    d = pc.drawn(29, 37, 65, K=3, seed=7)
    g, sc = d["g"], d["sc"]
    m = _drawn(product, d, 6)
    planes = sp.bound_planes(d["field"], 6)
    for l in range(1, 7):
        assert np.array_equal(m.bounds(l), planes[l]), l
    guesses = np.stack([gc.pose(-0.98, 0.52, 0.4), gc.pose(0.84, 1.2, -2.0), gc.pose(-1.0, 1.0, 3.0), gc.pose(-1.4, 0.2, 1.0),
                        gc.pose(1.2, 2.3, 0.0), d["poses"][0] @ gc.pose(0.1, 0.05, 0.1)]).astype(F)
    scans = np.concatenate([d["ranges"], d["ranges"]])
    hit = 0
    for window in ((5, 4, 1), (9, 6, 2), (20, 16, 0), (2, 31, 1)):
        for levels in (1, 2, 3, 4, 5, 6):
            hit += _check(m, d["field"], scans, guesses, sc, g, window, 0.05, levels, planes=planes)["score"].max() > 0
    assert hit
    e = product.OccupancyGrid(0)
    e.reset(0, 9)
    e.set_scan_model(sc["angle_min"], sc["angle_increment"], 65, 0.02, 20.0)
    e.build_likelihood()
    e.build_bounds(2)
    assert e.bounds(1).shape == (1, 10) and e.bounds(2).shape == (3, 12) and not e.bounds(2).any()
    got = _check(e, np.zeros((0, 9), np.uint8), scans[:3], guesses[:3], sc, gr.grid(0, 9), (2, 1, 1), 0.02, 2)
    assert not got["dx"].any() and not got["score"].any() and got["num_scored_beams"].min() > 0


def test_ties(product):
    """an all-zero field: the guess comes back and nothing survives; a table of all 255 at R = 16: plateaus; a table that is not
    monotone; the bare room scanned from its centre with quarter turns: with the guess among the winners, and off them, where the
    lowest flat index has to win"""
    d = pc.drawn(64, 80, 181, K=2, seed=9, boxes=False, noise=0.0)
    g, sc, room = d["g"], d["sc"], d["room"]
    m = _grid_of(product, g, sc)
    m.build_likelihood(1, 50, 4)
    m.build_bounds(3)
    centre = gc.pose(0.5 * (room[0] + room[1]), 0.5 * (room[2] + room[3]), 0.0)
    scan = gc.room_scans(room, centre[None], sc)
    got = _check(m, np.zeros((64, 80), np.uint8), scan, centre[None], sc, g, (5, 6, 2), 0.5 * math.pi, 3)
    assert got["stats"][0]["num_survivors"] == [0] * 7 and (got["dx"][0], got["dy"][0], got["jtheta"][0], got["score"][0]) == (0, 0, 0, 0)
    assert got["robot_in_world"].tobytes() == centre.astype(F).tobytes()
    m.integrate(d["ranges"], d["poses"], want_result=False)
    wild = np.random.default_rng(4).integers(0, 256, 17).astype(np.uint8)
    ties = 0
    for R, lut in ((16, np.full(257, 255, np.uint8)), (4, wild), (2, None)):
        m.build_likelihood(1, 50, R, lut)
        m.build_bounds(4)
        field = sm.likelihood(d["hits"], d["misses"], 1, 50, R, sm.default_lut(R) if lut is None else lut)
        for guess in (centre, centre @ gc.pose(0.1, -0.05, 0.0)):
            for levels in (1, 3, 4):
                got = _check(m, field, scan, guess[None], sc, g, (5, 6, 2), 0.5 * math.pi, levels, what="R %d" % R)
            vol = m.match_scans(scan, guess[None], (5, 6), 2, 0.5 * math.pi, want_scores=True)["scores"]
            ties += int((vol == vol.max()).sum() > 1)
    assert ties >= 2  # (the plateaus tie whatever the guess is)


def test_degenerate_scans_and_batches(recovery):
    """all NaN, no return inside [range_min, range_max], an easy scan, a tie and one that overflows its list, in one batch of 5:
    every row is the row of its own K = 1 call; num_scans = 0 and num_beams = 0"""
    m, rm = recovery
    truth, scans, guesses = pc.recovery_batch()
    batch = np.stack([scans[0], np.full(361, np.nan, F), scans[1], np.full(361, 25.0, F), scans[2]])
    gs = np.stack([guesses[0], guesses[1], truth[1], guesses[3], guesses[2]])
    window, levels, limit = (12, 12, 10), 3, 8
    got = _check(m, rm["field"], batch, gs, rm["sc"], rm["g"], window, DEG, levels, limit, planes=pc.recovery_planes())
    fell = [s["fell_back"] for s in got["stats"]]
    assert 0 < sum(fell) < 5 and fell[1] == fell[3] == 0 and list(got["num_scored_beams"][[1, 3]]) == [0, 0]
    for k in range(5):
        one = m.match_scans_pruned(batch[k:k + 1], gs[k:k + 1], window[:2], window[2], DEG, levels, limit, want_stats=True)
        _same(one, {n: v[k:k + 1] for n, v in got.items()}, "row %d" % k)
    none = m.match_scans_pruned(np.zeros((0, 361), F), np.zeros((0, 3, 3), F), (3, 3), 1, DEG, 2, want_stats=True)
    assert none["dx"].shape == (0,) and none["stats"] == []
    m.set_scan_model(rm["sc"]["angle_min"], rm["sc"]["angle_increment"], 0, 0.05, 20.0)
    beamless = dict(rm["sc"], num_beams=0)
    try:
        got = _check(m, rm["field"], np.zeros((3, 0), F), guesses[:3], beamless, rm["g"], (3, 4, 1), DEG, 2)
        assert not got["score"].any() and not got["dx"].any()
    finally:
        m.set_scan_model(rm["sc"]["angle_min"], rm["sc"]["angle_increment"], 361, float(rm["sc"]["range_min"]), float(rm["sc"]["range_max"]))


@pytest.mark.parametrize("limit", (1, 4))
def test_fall_back(recovery, limit):
    m, rm = recovery
    truth, scans, guesses = pc.recovery_batch()
    for levels in (1, 2, 4):
        got = _check(m, rm["field"], scans[:4], guesses[:4], rm["sc"], rm["g"], (12, 12, 10), DEG, levels, limit, planes=pc.recovery_planes())
        fell = [s for s in got["stats"] if s["fell_back"]]
        assert fell and all(s["num_evaluated"][0] == 13125 for s in fell), (limit, levels)


def test_past_the_caps(product):
    d, scans, guesses, window, step = pc.caps_case()
    g, sc = d["g"], d["sc"]
    m = _drawn(product, d, 2)
    planes = sp.bound_planes(d["field"], 2)
    assert planes[1].size > pc.BOUNDS_CAP and np.array_equal(m.bounds(1), planes[1]) and np.array_equal(m.bounds(2), planes[2])
    got = _check(m, d["field"], scans, guesses, sc, g, window, step, 1, planes=planes)
    st = got["stats"]
    assert 3 * 9 * -(-st[0]["num_evaluated"][1] // 9 // 256) > pc.TOP_CAP and st[0]["num_evaluated"][1] > pc.EXPAND_CAP
    assert st[1]["num_evaluated"][0] > pc.LIST_CAP and st[0]["num_candidates"] > pc.FALLBACK_CAP
    got = _check(m, d["field"], scans, guesses, sc, g, window, step, 1, 1000, planes=planes)
    assert [s["fell_back"] for s in got["stats"]] == [0, 1, 1]
    # the level kernel past its list cap: one beam
    d, sc1, scans, guesses, window, step = pc.caps_level_case()
    m.set_scan_model(sc1["angle_min"], sc1["angle_increment"], 1, 0.02, 20.0)
    got = _check(m, d["field"], scans, guesses, sc1, g, window, step, 2, planes=planes)
    assert got["stats"][0]["num_evaluated"][1] > pc.LIST_CAP and got["stats"][0]["num_evaluated"][0] > pc.LIST_CAP


def test_past_the_seed_cap(product):
    """more scans than k_prune_seed launches workgroups: 1 030 scans of 4 beams, a window of 3 x 3 x 1"""
    d = pc.drawn(29, 37, 65, K=3, seed=7)
    g = d["g"]
    m = _drawn(product, d, 1)
    a0, inc = gc.fan(4)
    sc = gr.scanner(a0, inc, 4, range_min=0.02, range_max=20.0)
    m.set_scan_model(a0, inc, 4, 0.02, 20.0)
    K = pc.SEED_CAP + 6
    truth = gc.trajectory(d["room"], K, 51)
    scans = gc.room_scans(d["room"], truth, sc, sigma=0.004, seed=52)
    guesses = np.stack([p @ gc.pose(0.04, -0.03, 0.02) for p in truth]).astype(F)
    got = _check(m, d["field"], scans, guesses, sc, g, (1, 1, 0), 0.0, 1)
    assert len(np.unique(got["dx"][-6:] * 3 + got["dy"][-6:])) > 1


def test_staleness_refusals_and_device_inputs(product):
    import torch
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    rm = smc.recovery_map()
    g, sc = rm["g"], rm["sc"]
    truth, scans, guesses = pc.recovery_batch()
    m = _grid_of(product, g, sc)
    args = (scans[:2], guesses[:2], (3, 3), 1, DEG)
    with pytest.raises(RuntimeError, match="stale"):
        m.build_bounds(2)  # no field yet
    m.integrate(rm["ranges"], rm["poses"], want_result=False)
    m.build_likelihood(1, 50, 4)
    with pytest.raises(RuntimeError, match="stale"):
        m.match_scans_pruned(*args, levels=2)  # a field, no planes
    with pytest.raises(RuntimeError, match="stale"):
        m.bounds(1)
    m.build_bounds(2)
    with pytest.raises(RuntimeError, match="above the number"):
        m.match_scans_pruned(*args, levels=3)
    with pytest.raises(RuntimeError, match="above the number"):
        m.bounds(3)
    want = sp.match(rm["field"], scans[:2], guesses[:2], sc, g, 3, 3, 1, DEG, 2)
    _same(m.match_scans_pruned(*args, want_stats=True), want, "levels=None: all that were built")
    # refused calls with a handle leave results and statistics as they were
    res, stats = (abi.GridMapMatchResult * 2)(), (abi.GridMapPruneStats * 2)()
    C.memset(res, 0x5a, C.sizeof(res)), C.memset(stats, 0x5a, C.sizeof(stats))
    before = bytes(res), bytes(stats)

    def call(levels=2, limit=0, wx=3, K=2):
        mp, pp = abi.GridMapMatchParams(), abi.GridMapPruneParams()
        mp.half_window_x, mp.half_window_y, mp.half_steps_theta, mp.theta_step = wx, 3, 1, DEG
        pp.num_levels, pp.max_list_entries = levels, limit
        return lib.srrg2_gridmap_match_scans_pruned(m._h, C.c_void_p(scans.ctypes.data), K, C.c_void_p(guesses.ctypes.data), abi.MEM_HOST,
                                                    C.byref(m.scan), C.byref(mp), C.byref(pp), res, stats)

    for kw in (dict(levels=0), dict(levels=7), dict(levels=3), dict(limit=-1), dict(wx=-1), dict(K=-1)):
        assert call(**kw) == E_INVALID and b"gridmap_match_scans_pruned" in lib.srrg2_amd_last_error(), kw
        assert (bytes(res), bytes(stats)) == before
    assert call() == 0 and (bytes(res), bytes(stats)) != before and stats[1].as_dict()["floor_score"] == want["stats"][1]["floor_score"]
    # ranges and guesses on the device
    dr, dg = torch.from_numpy(scans[:2].copy()).cuda(), torch.from_numpy(guesses[:2].copy()).cuda()
    torch.cuda.synchronize()
    _same(m.match_scans_pruned(dr, dg, (3, 3), 1, DEG, 2, want_stats=True), want, "device inputs")
    # whatever makes the field stale makes the planes stale: a rebuilt field, an integrated scan, a reset
    m.build_likelihood(1, 50, 4)
    with pytest.raises(RuntimeError, match="stale"):
        m.match_scans_pruned(*args, levels=2)
    m.build_bounds(2)
    m.integrate(scans[:1], truth[:1], want_result=False)
    for again in (lambda: m.match_scans_pruned(*args, levels=2), lambda: m.build_bounds(2), lambda: m.bounds(1)):
        with pytest.raises(RuntimeError, match="stale"):
            again()
    m.build_likelihood(1, 50, 4)
    m.build_bounds(1)
    m.reset(5, 7, 0.1, (0.0, 0.0))
    with pytest.raises(RuntimeError, match="stale"):
        m.bounds(1)


def test_localize_and_through_the_stack(recovery, product):
    """the ten recovery scans without a guess, against the whole map at 4 degrees: the restatement's answer, the exhaustive
    call's answer on the same window; then the SE(2) aligner from the first localised pose on the scene of the map"""
    m, rm = recovery
    g, sc = rm["g"], rm["sc"]
    truth, scans, _ = pc.recovery_batch()
    step = 4.0 * DEG
    wx, wy, ht = pc.localize_window(g, step)
    assert (wx, wy, ht) == (100, 80, 45)
    centre = np.tile(pc.centre_pose(g), (10, 1, 1))
    assert m.centre_pose().tobytes() == pc.centre_pose(g).tobytes()
    want = sp.match(rm["field"], scans, centre, sc, g, wx, wy, ht, step, 4, planes=pc.recovery_planes())
    got = m.localize(scans, step, 4, want_stats=True)
    _same(got, want, "localize")
    _same(m.match_scans(scans, centre, (wx, wy), ht, step), got, "the exhaustive call on the whole map")
    _same(m.localize(scans, step), {k: v for k, v in want.items() if k != "stats"}, "levels=None: the six built")
    assert (max(sum(s["num_evaluated"]) for s in got["stats"]) + 4 ** 4 + 1) * 100 < got["stats"][0]["num_candidates"]  # (it pruned)
    fresh = _grid_of(product, g, sc)  # localize builds the planes itself
    fresh.integrate(rm["ranges"], rm["poses"], want_result=False)
    fresh.build_likelihood(1, 50, 4)
    _same(fresh.localize(scans[:2], step), {k: v[:2] for k, v in want.items() if k != "stats"}, "planes built by localize")
    matched = got["robot_in_world"][0]
    scene = mapping.Scene(product.scene_binding(0), 2)
    assert m.to_scene(scene, 1, 50) > 300
    points = ar.adapt_laser_scan(scans[0], sc["angle_min"], sc["angle_increment"], half_window=0)["points"]
    al = product.MultiAligner(abi.SE2_RIGHT, device=0)
    si = al.add_slice(cue_config(abi.SE2_RIGHT, abi.SLICE_P2P, 0.3))
    fp, fn, nf = scene.device_arrays()
    al.set_cloud_device("set_fixed", si, fp, 16, None, 16, nf)
    al.set_moving(si, points)
    al.set_moving_in_fixed(np.asarray(matched, F))
    al.compute()
    start, end = smc.pose_error(matched, truth[0]), smc.pose_error(al.moving_in_fixed(), truth[0])
    print("localised: |error| = %.3f m %.3f m %.2f deg; after the aligner: %.3f m %.3f m %.2f deg" %
          (start[0], start[1], math.degrees(start[2]), end[0], end[1], math.degrees(end[2])))
    assert al.status() == abi.SUCCESS and math.hypot(end[0], end[1]) < 0.05 and end[2] < step
