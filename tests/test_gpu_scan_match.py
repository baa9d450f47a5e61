"""GPU: correlative scan matching (csrc/scan_match.hip) against the numpy restatement of its contract
(tests/scan_match_restatement.py), BIT FOR BIT: the likelihood field, every member of every result and the whole score volume, at
the smallest shapes where the kernels can go wrong; the tie order; staleness; refusals that leave planes, field and destinations as
they were; and through the stack: the SE(2) aligner started from the matcher's pose on the scene of the map."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import adaptor_restatement as ar
import gridmap_cases as gc
import gridmap_restatement as gr
import scan_match_cases as smc
import scan_match_restatement as sm
from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID = -1
MEMBERS = ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")


def _grid_of(product, g, sc):
    m = product.OccupancyGrid(0)
    m.reset(g["rows"], g["cols"], float(g["res"]), (float(g["ox"]), float(g["oy"])))
    m.set_scan_model(sc["angle_min"], sc["angle_increment"], sc["num_beams"], float(sc["range_min"]), float(sc["range_max"]),
                     sc["sensor_in_robot"], sc["clear_beyond_max"])
    return m


def _same(got, want, what=""):
    assert got["robot_in_world"].tobytes() == want["robot_in_world"].tobytes(), "pose " + what
    for k in MEMBERS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), "%s %s: %s != %s" % (k, what, got[k], want[k])
    if "scores" in got:
        assert got["scores"].shape == want["scores"].shape and np.array_equal(got["scores"], want["scores"]), "volume " + what


@functools.lru_cache(maxsize=None)
def _map(rows, cols, nb, K=3, seed=3, clockwise=False, mounted=False):
    """a room drawn into the grid from K poses, with mixed ranges: planes, and the field of radius 2"""
    g = gr.grid(rows, cols, 0.05, (-1.0, 0.5))
    a0, inc = gc.fan(nb, clockwise=clockwise)
    sc = gr.scanner(a0, inc, nb, range_min=0.02, range_max=20.0, sensor_in_robot=gc.pose(0.21, -0.13, -0.6) if mounted else None)
    room = gc.room_of(g)
    poses = gc.trajectory(room, K, seed)
    ranges = gc.mixed(gc.room_scans(room, poses, sc, sigma=0.004, seed=seed + 1), seed + 2)
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    field = sm.likelihood(h, w, 1, 50, 2, sm.default_lut(2))
    for a in (poses, ranges, h, w, field):
        a.setflags(write=False)
    return g, sc, room, poses, ranges, h, w, field


def _drawn(product, case, R=2):
    g, sc, room, poses, ranges, h, w, field = case
    m = _grid_of(product, g, sc)
    m.integrate(ranges, poses, want_result=False)
    m.build_likelihood(1, 50, R)
    return m


@pytest.mark.parametrize("shape", gc.GRIDS, ids=str)
def test_field_bit_for_bit(product, shape):
    """grids 1 x 1 .. 129 x 257, R = 0, 1, 4, 16 (larger than the small grids), both thresholds, the default table and a table that
    is not monotone; occupied cells in the corners and on the edges, unknown neighbours"""
    rows, cols = shape
    g = gr.grid(rows, cols, 0.05, (0.0, 0.0))
    sc = gr.scanner(0.0, 0.1, 1, range_min=0.001, range_max=20.0)
    rng = np.random.default_rng(rows * 1000 + cols)
    # one-beam scans: a range of 1 mm is a hit in the sensor's own cell, the longer ones leave misses on their way
    cells = [(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1), (cols // 2, 0), (0, rows // 2)]
    cells += [(int(rng.integers(cols)), int(rng.integers(rows))) for _ in range(max(2, rows * cols // 40))]
    poses = np.stack([gc.pose((x + 0.5) * 0.05, (y + 0.5) * 0.05, rng.uniform(-3, 3)) for x, y in cells] * 2)
    ranges = np.concatenate([np.full(len(cells), 0.001, F), rng.uniform(0.05, 0.4, len(cells)).astype(F)])[:, None]
    h, w = gr.new_planes(g)
    gr.integrate(h, w, ranges, poses, sc, g)
    m = _grid_of(product, g, sc)
    m.integrate(ranges, poses, want_result=False)
    assert h[0, 0] and h[-1, -1] and (rows * cols < 100 or ((h + w) == 0).any())
    for R in (0, 1, 4, 16):
        wild = np.random.default_rng(R).integers(0, 256, R * R + 1).astype(np.uint8)
        for need, pct, lut in ((1, 50, None), (2, 34, None), (1, 100, wild), (1, 0, wild)):
            m.build_likelihood(need, pct, R, lut)
            want = sm.likelihood(h, w, need, pct, R, sm.default_lut(R) if lut is None else lut)
            assert np.array_equal(m.likelihood(), want), (shape, R, need, pct)
    assert want.any()


def test_field_padded_stride_and_misaligned_destination(product):
    import torch

    case = _map(129, 257, 361)
    m = _drawn(product, case, R=4)
    want = sm.likelihood(case[5], case[6], 1, 50, 4, sm.default_lut(4))
    assert len(np.unique(want)) > 5
    buf = np.full((129, 300), 0xaa, np.uint8)
    view = buf[:, 3:3 + 257]
    assert view.ctypes.data % 4 == 3 and m.likelihood(out=view) is view
    assert np.array_equal(view, want) and (buf[:, :3] == 0xaa).all() and (buf[:, 260:] == 0xaa).all()
    dev = torch.full((129 * 300 + 8,), 0xaa, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m.likelihood(out=(dev.data_ptr() + 3, 300))
    got = dev.cpu().numpy()[:129 * 300].reshape(129, 300)
    assert np.array_equal(got[:, 3:260], want) and (got[:, :3] == 0xaa).all() and (got[:, 260:] == 0xaa).all()


def _guesses(poses, seed, offset=0.12, turn=0.08):
    rng = np.random.default_rng(seed)
    if len(poses) == 0:
        return np.zeros((0, 3, 3), F)
    return np.stack([p @ gc.pose(*(rng.uniform(-1, 1, 3) * (offset, offset, turn))) for p in poses]).astype(F).reshape(-1, 3, 3)


# (grid, num_beams, K, (wx, wy, ht)): every beam count, every K, the five windows of the contract's edges, row widths either side of
# a wave (63, 65, 129; 101 is two tiles of 64 lanes, 65 and 129 are tiles of 32) with wy either side of a tile of dy rows
# (0, 2, 33)
MATCHES = (((7, 5), 1, 1, (0, 0, 0)), ((64, 64), 63, 3, (1, 0, 0)), ((64, 64), 64, 3, (0, 1, 0)), ((64, 64), 65, 3, (0, 0, 1)),
           ((64, 64), 361, 3, (14, 14, 12)), ((129, 257), 1081, 1, (5, 9, 2)), ((64, 64), 65, 65, (3, 2, 1)), ((64, 64), 0, 3, (2, 2, 1)),
           ((64, 64), 63, 0, (2, 2, 1)), ((64, 64), 65, 1, (31, 0, 0)), ((64, 64), 65, 1, (32, 2, 0)), ((129, 257), 65, 1, (64, 33, 0)),
           ((129, 257), 65, 1, (50, 2, 0)), ((64, 64), 64, 1, (7, 33, 1)), ((64, 64), 64, 1, (15, 17, 0)))


@pytest.mark.parametrize("case", MATCHES, ids=str)
def test_match_bit_for_bit(product, case):
    (rows, cols), nb, K, (wx, wy, ht) = case
    g, sc, room, poses, ranges, h, w, field = drawn = _map(rows, cols, max(nb, 16))
    m = _drawn(product, drawn)
    # the scans to match: their own scanner (nb beams), K poses of another trajectory, guesses off by a few cells and degrees
    a0, inc = gc.fan(nb)
    sc2 = gr.scanner(a0, inc, nb, range_min=0.02, range_max=20.0)
    truth = gc.trajectory(room, K, 21)
    scans = gc.mixed(gc.room_scans(room, truth, sc2, sigma=0.004, seed=22), 23)
    guesses = _guesses(truth, 24)
    m.set_scan_model(a0, inc, nb, 0.02, 20.0)
    step = 0.03
    want = sm.match(field, scans, guesses, sc2, g, wx, wy, ht, step)
    got = m.match_scans(scans, guesses, (wx, wy), ht, step, want_scores=True)
    _same(got, want, str(case))
    _same(m.match_scans(scans, guesses, (wx, wy), ht, step), {k: v for k, v in want.items() if k != "scores"}, "without the volume")
    if K and nb >= 63:
        assert want["score"].max() > 0 and want["num_scored_beams"].min() > 0 and want["num_scored_beams"].max() < nb


def test_match_hanging_over_the_border_clockwise_mounted_and_from_the_device(product):
    """guesses near a corner and outside the grid, so that window and beams hang over it; a clockwise scanner on a mount; ranges,
    guesses and the volume in device memory"""
    import torch

    drawn = _map(64, 64, 361, clockwise=True, mounted=True)
    g, sc, room, poses, ranges, h, w, field = drawn
    m = _drawn(product, drawn)
    assert sc["angle_increment"] < 0
    guesses = np.stack([gc.pose(-0.9, 0.6, 0.4), gc.pose(2.3, 3.8, -2.0), gc.pose(-1.4, 0.2, 1.0), poses[0] @ gc.pose(0.1, 0.05, 0.1)]).astype(F)
    scans = np.concatenate([ranges, ranges[:1]])
    want = sm.match(field, scans, guesses, sc, g, 9, 6, 2, 0.05)
    assert want["score"][:3].max() > 0 and (want["scores"][:3] == 0).any()
    _same(m.match_scans(scans, guesses, (9, 6), 2, 0.05, want_scores=True), want, "host")
    dr, dg = torch.from_numpy(scans.copy()).cuda(), torch.from_numpy(guesses.copy()).cuda()
    vol = torch.full((want["scores"].size + 4,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    got = m.match_scans(dr, dg, (9, 6), 2, 0.05, want_scores=vol[:want["scores"].size])
    back = vol.cpu().numpy()
    assert np.array_equal(back[:-4].reshape(want["scores"].shape), want["scores"]) and (back[-4:] == -7).all()
    got["scores"] = want["scores"]
    _same(got, want, "device")


def test_past_the_scoring_launch_cap(product):
    """the scoring kernel launches at most 8 192 workgroups and strides over the tiles beyond: 65 scans x 129 rotations of one
    tile each are 8 385"""
    drawn = _map(64, 64, 65)
    g, sc, room, poses, ranges, h, w, field = drawn
    m = _drawn(product, drawn)
    truth = gc.trajectory(room, 65, 31)
    scans = gc.room_scans(room, truth, sc, sigma=0.004, seed=32)
    guesses = _guesses(truth, 33, turn=0.3)
    assert 65 * 129 > 8192
    want = sm.match(field, scans, guesses, sc, g, 0, 0, 64, 0.01)
    assert len(np.unique(want["jtheta"])) > 5 and np.abs(want["jtheta"][-5:]).max() > 0  # (the last scans lie beyond the first trip)
    _same(m.match_scans(scans, guesses, (0, 0), 64, 0.01, want_scores=True), want)


def _hand_made(product, cells, rows=9, cols=12):
    """a field that is 255 on `cells` and 0 elsewhere (hits drawn by one-beam scans, radius 0), and a one-beam scanner"""
    g = gr.grid(rows, cols, 0.1, (0.0, 0.0))
    sc = gr.scanner(0.0, 0.1, 1, range_min=0.001, range_max=20.0)
    m = _grid_of(product, g, sc)
    if cells:
        m.integrate(np.full((len(cells), 1), 0.001, F), np.stack([gc.pose((x + 0.5) * 0.1, (y + 0.5) * 0.1, 0.0) for x, y in cells]))
    m.build_likelihood(1, 50, 0)
    field = np.zeros((rows, cols), np.uint8)
    for x, y in cells:
        field[y, x] = 255
    assert np.array_equal(m.likelihood(), field)
    return m, g, sc, field


def test_ties(product):
    """an empty field hands the guess back; two equal maxima: the lowest flat index; the guess among the maxima: the guess"""
    guess = gc.pose(0.43, 0.44, 0.0)[None]  # the beam of 0.2 m ends in cell (6, 4)
    scan = np.full((1, 1), 0.2, F)
    for cells, (dx, dy, score) in (((), (0, 0, 0)), (((8, 5), (5, 3)), (-1, -1, 255)), (((8, 5), (5, 3), (6, 4)), (0, 0, 255)),
                                   (((8, 5), (4, 5)), (-2, 1, 255))):
        m, g, sc, field = _hand_made(product, cells)
        want = sm.match(field, scan, guess, sc, g, 2, 2, 1, 0.001)
        got = m.match_scans(scan, guess, (2, 2), 1, 0.001, want_scores=True)
        _same(got, want, str(cells))
        # (all three rotations of a milliradian end in the same cell: the first of them holds the lowest flat index)
        assert (got["dx"][0], got["dy"][0], got["score"][0]) == (dx, dy, score), cells
        assert got["jtheta"][0] == (0 if (dx, dy) == (0, 0) else -1) and (got["scores"] == 255).sum() == 3 * len(cells)
    # a scan without a return on a field that is not empty
    got = m.match_scans(np.full((1, 1), np.nan, F), guess, (2, 2), 1, 0.001, want_scores=True)
    assert not got["scores"].any() and (got["dx"][0], got["dy"][0], got["jtheta"][0], got["num_scored_beams"][0]) == (0, 0, 0, 0)
    assert got["robot_in_world"].tobytes() == guess.astype(F).tobytes()


def test_staleness_and_misuse_leave_everything_as_it_was(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    drawn = _map(64, 64, 65)
    g, sc, room, poses, ranges, h, w, field = drawn
    m = _grid_of(product, g, sc)
    with pytest.raises(RuntimeError, match="stale"):
        m.match_scans(ranges, poses, (1, 1))
    with pytest.raises(RuntimeError, match="stale"):
        m.likelihood()
    m.integrate(ranges, poses)
    with pytest.raises(RuntimeError, match="stale"):
        m.match_scans(ranges, poses, (1, 1))
    m.build_likelihood(1, 50, 2)
    want = sm.match(field, ranges, poses, sc, g, 2, 1, 1, 0.02)
    _same(m.match_scans(ranges, poses, (2, 1), 1, 0.02, want_scores=True), want, "after the build")
    # refused calls with a handle: destinations, planes and field stay
    res = (abi.GridMapMatchResult * 3)()
    C.memset(res, 0x5a, C.sizeof(res))
    before = bytes(res)
    vol = np.full(3 * 45, 0x5a5a5a5a, np.int32)

    def call(scan=None, wx=2, wy=1, ht=1, step=0.02, K=3, r=ranges.ctypes.data, t=poses.ctypes.data, mem=abi.MEM_HOST):
        mp = abi.GridMapMatchParams()
        mp.half_window_x, mp.half_window_y, mp.half_steps_theta, mp.theta_step = wx, wy, ht, step
        return lib.srrg2_gridmap_match_scans(m._h, C.c_void_p(r), K, C.c_void_p(t), mem, C.byref(m.scan if scan is None else scan),
                                             C.byref(mp), res, C.c_void_p(vol.ctypes.data), abi.MEM_HOST)

    far = abi.GridMapScanParams.from_buffer_copy(bytes(m.scan))
    far.range_max = 1601.0
    beamless = abi.GridMapScanParams.from_buffer_copy(bytes(m.scan))
    beamless.num_beams = 0  # (its guesses are still read: null ones are refused, in host and in device memory)
    for kw in (dict(wx=-1), dict(step=float("nan")), dict(step=0.0), dict(K=-1), dict(scan=far), dict(t=0), dict(scan=beamless, r=0, t=0),
               dict(scan=beamless, r=0, t=0, mem=abi.MEM_DEVICE), dict(scan=beamless, r=0, t=poses.ctypes.data + 2)):
        assert call(**kw) == E_INVALID and b"gridmap_match_scans" in lib.srrg2_amd_last_error(), kw
        assert bytes(res) == before and (vol == 0x5a5a5a5a).all()
    lut = sm.default_lut(2)
    for args in ((1, 50, 17), (1, 101, 2)):
        assert lib.srrg2_gridmap_build_likelihood(m._h, *args, C.c_void_p(lut.ctypes.data)) == E_INVALID
    img = np.full((64, 64), 0xaa, np.uint8)
    assert lib.srrg2_gridmap_get_likelihood(m._h, C.c_void_p(img.ctypes.data), 63, abi.MEM_HOST) == E_INVALID
    assert lib.srrg2_gridmap_get_likelihood(m._h, None, 64, abi.MEM_HOST) == E_INVALID and (img == 0xaa).all()
    assert np.array_equal(m.likelihood(), field) and np.array_equal(m.counts()[0], h) and np.array_equal(m.counts()[1], w)
    assert call() == 0 and bytes(res) != before and np.array_equal(vol.reshape(want["scores"].shape), want["scores"])
    # scans without beams and without ranges get their guesses back
    assert call(scan=beamless, r=0) == 0 and not vol.any()
    assert [(e.dx, e.dy, e.jtheta, e.score, e.num_scored_beams) for e in res] == [(0, 0, 0, 0, 0)] * 3
    assert np.array([list(e.robot_in_world) for e in res], F).tobytes() == sm.rotated_guesses(poses, 0, 0.02, 1).tobytes()
    # taking a scan out makes the field stale again, so does a reset; a rebuild is of the planes as they are then
    m.remove(ranges[:1], poses[:1])
    with pytest.raises(RuntimeError, match="stale"):
        m.match_scans(ranges, poses, (1, 1))
    h2, w2 = h.copy(), w.copy()
    gr.integrate(h2, w2, ranges[:1], poses[:1], sc, g, -1)
    m.build_likelihood(2, 40, 4)
    assert np.array_equal(m.likelihood(), sm.likelihood(h2, w2, 2, 40, 4, sm.default_lut(4)))
    m.reset(5, 7, 0.1, (0.0, 0.0))
    with pytest.raises(RuntimeError, match="stale"):
        m.likelihood()
    # an empty grid: every call is taken, the scores are zero and the guesses come back
    e = product.OccupancyGrid(0)
    e.reset(0, 9)
    e.set_scan_model(sc["angle_min"], sc["angle_increment"], 65, 0.02, 20.0)
    e.build_likelihood()
    assert e.likelihood().shape == (0, 9)
    got = e.match_scans(ranges, poses, (2, 1), 1, 0.02, want_scores=True)
    _same(got, sm.match(np.zeros((0, 9), np.uint8), ranges, poses, sc, gr.grid(0, 9), 2, 1, 1, 0.02), "empty grid")
    assert not got["scores"].any() and not got["dx"].any() and got["num_scored_beams"].min() > 0


def test_recovery_through_the_stack(product):
    """the recovery setting, 0.5 m and 9 degrees off: the matcher's pose is bit for bit the restatement's, and the SE(2) P2P
    aligner (gate 0.3 m) started from it on the scene of the map reaches SUCCESS and ends nearer the truth than the raw guess was"""
    rm = smc.recovery_map()
    g, sc = rm["g"], rm["sc"]
    m = _grid_of(product, g, sc)
    m.integrate(rm["ranges"], rm["poses"], want_result=False)
    m.build_likelihood(1, 50, 4)
    assert np.array_equal(m.likelihood(), rm["field"])
    truth = gc.pose(3.1, 5.2, 0.7)
    scan = smc.box_scans(rm["room"], rm["boxes"], truth[None], sc, sigma=0.004, seed=77)
    guess = gc.pose(3.1 + 0.5, 5.2 - 0.5, 0.7 + math.radians(9.0))
    step = math.radians(1.0)
    want = sm.match(rm["field"], scan, guess[None], sc, g, 14, 14, 12, step)
    got = m.match_scans(scan, guess[None], (14, 14), 12, step, want_scores=True)
    _same(got, want)
    matched = got["robot_in_world"][0]
    ex, ey, eth = smc.pose_error(matched, truth)
    assert ex <= 0.05 and ey <= 0.05 and eth <= step
    scene = mapping.Scene(product.scene_binding(0), 2)
    assert m.to_scene(scene, 1, 50) > 300
    points = ar.adapt_laser_scan(scan[0], sc["angle_min"], sc["angle_increment"], half_window=0)["points"]
    reached = {}
    for name, start in (("raw guess", guess), ("matched pose", matched)):
        al = product.MultiAligner(abi.SE2_RIGHT, device=0)
        si = al.add_slice(cue_config(abi.SE2_RIGHT, abi.SLICE_P2P, 0.3))
        fp, fn, nf = scene.device_arrays()
        al.set_cloud_device("set_fixed", si, fp, 16, None, 16, nf)
        al.set_moving(si, points)
        al.set_moving_in_fixed(np.asarray(start, F))
        al.compute()
        reached[name] = (al.status(), smc.pose_error(al.moving_in_fixed(), truth))
        print("aligner from the %s: status %d, |error| = %.3f m %.3f m %.2f deg (start: %.3f m %.3f m %.2f deg)" %
              ((name, reached[name][0]) + reached[name][1][:2] + (math.degrees(reached[name][1][2]),) +
               smc.pose_error(start, truth)[:2] + (math.degrees(smc.pose_error(start, truth)[2]),)))
    status, err = reached["matched pose"]
    raw = smc.pose_error(guess, truth)
    assert status == abi.SUCCESS
    assert math.hypot(err[0], err[1]) < math.hypot(raw[0], raw[1]) and err[2] < raw[2]
