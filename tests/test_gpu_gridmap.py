"""GPU: srrg2_gridmap_* (csrc/gridmap.hip) against the numpy restatement of its contract (tests/gridmap_restatement.py), BIT FOR
BIT: both count planes, the result's counters, the rendered image and the exported scene, at the smallest shapes where the kernel
can go wrong (tests/gridmap_cases.py); takes a batch out again, splits it, queues it; refusals leave planes and destinations as
they were; and through the stack: the scene of the map aligns a scan to the same bits as the same points handed in by the host."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import adaptor_restatement as ar
import gridmap_cases as gc
import gridmap_restatement as gr
from helpers import cue_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu
F = np.float32
PI = math.pi
E_INVALID = -1


def _grid_of(product, g, sc):
    m = product.OccupancyGrid(0)
    m.reset(g["rows"], g["cols"], float(g["res"]), (float(g["ox"]), float(g["oy"])))
    m.set_scan_model(sc["angle_min"], sc["angle_increment"], sc["num_beams"], float(sc["range_min"]), float(sc["range_max"]),
                     sc["sensor_in_robot"], sc["clear_beyond_max"])
    return m


def _same_planes(m, h, w, what=""):
    hits, misses = m.counts()
    assert hits.dtype == np.int32 and hits.shape == h.shape
    assert np.array_equal(hits, h), "hits " + what
    assert np.array_equal(misses, w), "misses " + what


def _same_products(product, m, g, h, w, what=""):
    """the image at two thresholds and the scene against the restatement of the planes (h, w)"""
    for need in (1, 3):
        assert np.array_equal(m.render(need), gr.render(h, w, need)), "image %d %s" % (need, what)
    scene = mapping.Scene(product.scene_binding(0), 2)
    for need, pct in ((1, 50), (2, 1)):
        pts, idx = gr.to_scene(h, w, g, need, pct)
        assert m.to_scene(scene, need, pct) == len(idx), what
        got, _ = scene.get()
        assert np.asarray(got, F).reshape(-1, 2).tobytes() == pts.tobytes(), "scene points " + what
        assert np.array_equal(scene.global_indices(), idx), "scene indices " + what
        assert scene.device_arrays()[1] is None  # no normals


@functools.lru_cache(maxsize=None)
def _reference(shape):
    g, sc, poses, ranges = gc.shape_case(shape, seed=3)
    ranges = gc.mixed(ranges, seed=4)
    h, w = gr.new_planes(g)
    out = gr.integrate(h, w, ranges, poses, sc, g)
    for a in (poses, ranges, h, w):
        a.setflags(write=False)
    return g, sc, poses, ranges, h, w, out


@pytest.mark.parametrize("shape", gc.SHAPES, ids=str)
def test_shapes_bit_for_bit(product, shape):
    """grids 1 x 1 .. 129 x 257, K = 0 .. 65, num_beams = 0 .. 1 081 (K = 0 and num_beams = 0: legal, nothing happens)"""
    g, sc, poses, ranges, h, w, want = _reference(shape)
    m = _grid_of(product, g, sc)
    assert m.integrate(ranges, poses) == want, shape
    _same_planes(m, h, w, str(shape))
    _same_products(product, m, g, h, w, str(shape))
    if shape[1] * shape[2] == 0:
        assert not h.any() and not w.any() and want["num_beams_total"] == 0
    elif shape[0] != (1, 1):
        assert want["num_hits_in_grid"] > 0 and want["num_miss_updates"] > 0 and want["num_skipped"] > 0


def test_rays_of_every_direction_inside_outside_and_through_a_corner(product):
    """16 beams per scan: the four axes, the four diagonals and one beam inside every octant; sensors in the middle, on the edge,
    outside looking in and outside looking past a corner; ranges from n = 0 to far beyond the grid"""
    for rows, cols in ((7, 5), (64, 64)):
        g = gr.grid(rows, cols, 0.1, (0.0, 0.0))
        sc = gr.scanner(0.0, PI / 8, 16, range_min=0.001, range_max=20.0)
        w_, h_ = cols * 0.1, rows * 0.1
        spots = [(0.5 * w_ + 0.003, 0.5 * h_ - 0.002, 0.0), (0.05, 0.05, 0.0), (w_ - 0.01, h_ - 0.01, 0.0), (-0.35, 0.5 * h_, 0.0),
                 (0.5 * w_, h_ + 0.72, 0.0), (-0.15, -0.15, 0.0), (-0.15, 0.25, 0.1), (w_ + 0.2, -0.1, PI / 16), (-3.0, -3.0, 0.3)]
        poses = np.stack([gc.pose(*s) for s in spots])
        for reach in (0.004, 0.33, 1.0, 3.1, 15.0):
            ranges = np.full((len(spots), 16), reach, F)
            h, w = gr.new_planes(g)
            want = gr.integrate(h, w, ranges, poses, sc, g)
            m = _grid_of(product, g, sc)
            assert m.integrate(ranges, poses) == want, (rows, cols, reach)
            _same_planes(m, h, w, "%dx%d reach %g" % (rows, cols, reach))
        assert want["num_miss_updates"] > 0


def test_contention_every_beam_of_65_scans_in_one_cell(product):
    """65 x 361 beams that all end in the sensor's cell (n = 0), then 65 x 361 that all leave it (one miss each in that cell):
    same-address adds from every lane of every wave, and the counts are exact"""
    g = gr.grid(7, 5, 0.05, (0.0, 0.0))
    sc = gr.scanner(-PI, 2 * PI / 360, 361, range_min=0.001, range_max=5.0)
    poses = np.repeat(gc.pose(0.125, 0.175, 0.0)[None], 65, axis=0)
    m = _grid_of(product, g, sc)
    near = np.full((65, 361), 0.01, F)
    out = m.integrate(near, poses)
    hits, misses = m.counts()
    assert hits[3, 2] == 65 * 361 == hits.sum() == out["num_hits_in_grid"] and not misses.any()
    far = np.full((65, 361), 0.2, F)
    out = m.integrate(far, poses)
    hits, misses = m.counts()
    assert misses[3, 2] == 65 * 361 and out["num_miss_updates"] == misses.sum()
    h, w = gr.new_planes(g)
    gr.integrate(h, w, near, poses, sc, g)
    gr.integrate(h, w, far, poses, sc, g)
    assert np.array_equal(hits, h) and np.array_equal(misses, w)


@pytest.mark.parametrize("clear", (True, False))
def test_beam_classes_a_clockwise_scanner_and_a_mounted_sensor(product, clear):
    mount = gc.pose(0.21, -0.13, -0.6)
    a0, inc = gc.fan(361, clockwise=True)
    assert inc < 0
    g = gr.grid(64, 64, 0.05, (-1.0, 0.5))
    sc = gr.scanner(a0, inc, 361, range_min=0.1, range_max=1.1, sensor_in_robot=mount, clear_beyond_max=clear)
    room = gc.room_of(g)
    poses = gc.trajectory(room, 3, seed=12)
    ranges = gc.mixed(gc.room_scans(room, poses, sc), seed=13)
    h, w = gr.new_planes(g)
    want = gr.integrate(h, w, ranges, poses, sc, g)
    assert want["num_returns"] > 0 and want["num_skipped"] > 0 and (want["num_cleared_only"] > 0) == clear
    m = _grid_of(product, g, sc)
    assert m.integrate(ranges, poses) == want
    _same_planes(m, h, w)
    _same_products(product, m, g, h, w)
    # the same scans through the identity mount land elsewhere
    m2 = _grid_of(product, g, dict(sc, sensor_in_robot=np.eye(3, dtype=F)))
    m2.integrate(ranges, poses)
    assert not np.array_equal(m2.counts()[0], h)


def test_weights_batches_and_queued_calls(product):
    """+1 then -1 bit-restores a non-empty map; one batch of 65 = 65 single calls = two halves; calls that only queue
    (want_result=False) followed by counts(); ranges and poses in host and in device memory"""
    import torch

    g, sc, poses, ranges, h, w, want = _reference(((64, 64), 65, 361))
    first = gc.shape_case(((64, 64), 3, 361), seed=40)
    h0, w0 = gr.new_planes(g)
    gr.integrate(h0, w0, first[3], first[2], sc, g)
    m = _grid_of(product, g, sc)
    m.integrate(first[3], first[2])
    _same_planes(m, h0, w0, "non-empty start")
    assert m.integrate(ranges, poses) == want
    assert m.remove(ranges, poses) == want
    _same_planes(m, h0, w0, "+1 then -1")
    # 65 single calls, none of which waits
    for k in range(65):
        assert m.integrate(ranges[k:k + 1], poses[k:k + 1], want_result=False) is None
    _same_planes(m, h0 + h, w0 + w, "65 queued single calls")
    # two halves taken out, from device memory
    dr, dp = torch.from_numpy(np.array(ranges)).cuda(), torch.from_numpy(np.array(poses)).cuda()
    torch.cuda.synchronize()
    a = m.remove(dr[:32], dp[:32])
    b = m.remove(dr[32:], dp[32:], want_result=False)
    assert b is None
    _same_planes(m, h0, w0, "two halves out")
    rest = gr.integrate(*gr.new_planes(g), ranges[:32], poses[:32], sc, g)
    assert a == rest
    # and the whole batch from device memory with its counters
    assert m.integrate(dr, dp) == want
    _same_planes(m, h0 + h, w0 + w, "device batch")
    hp, mp = m.device_arrays()
    assert hp and mp == hp + 4 * 64 * 64
    # the counts into device memory (one plane may be left out)
    dh, dm_ = torch.zeros((64, 64), dtype=torch.int32, device="cuda:0"), torch.full((64, 64), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    m._check(m._lib.srrg2_gridmap_get_counts(m._h, C.c_void_p(dh.data_ptr()), None, abi.MEM_DEVICE))
    assert np.array_equal(dh.cpu().numpy(), h0 + h) and (dm_.cpu().numpy() == -7).all()
    m._check(m._lib.srrg2_gridmap_get_counts(m._h, None, C.c_void_p(dm_.data_ptr()), abi.MEM_DEVICE))
    assert np.array_equal(dm_.cpu().numpy(), w0 + w)


def test_past_the_launch_cap(product):
    """the integrate kernel launches at most 1 024 workgroups of 256 lanes and strides over the beams beyond 262 144:
    260 scans x 1 081 beams = 281 060 beams take the second trip of the grid-stride loop"""
    K, nb = 260, 1081
    assert K * nb > 1024 * 256
    g = gr.grid(64, 64, 0.05, (-1.0, 0.5))
    a0, inc = gc.fan(nb)
    sc = gr.scanner(a0, inc, nb, range_min=0.02, range_max=1.2)
    room = gc.room_of(g)
    poses = gc.trajectory(room, K, seed=50)
    ranges = gc.room_scans(room, poses, sc, sigma=0.003, seed=51)
    h, w = gr.new_planes(g)
    want = gr.integrate(h, w, ranges, poses, sc, g)
    assert want["num_cleared_only"] > 0 and want["num_returns"] > 0
    m = _grid_of(product, g, sc)
    assert m.integrate(ranges, poses) == want
    _same_planes(m, h, w)
    # the last scan alone lies wholly beyond the cap's first trip
    tail = gr.integrate(*gr.new_planes(g), ranges[-1:], poses[-1:], sc, g)
    assert tail["num_miss_updates"] > 0


def test_render_padded_stride_and_misaligned_destination(product):
    import torch

    g, sc, poses, ranges, h, w, _ = _reference(((129, 257), 3, 1081))
    m = _grid_of(product, g, sc)
    m.integrate(ranges, poses, want_result=False)
    want = gr.render(h, w, 1)
    assert len(np.unique(want)) > 3
    # host: rows at a padded stride, the first byte misaligned; the padding stays
    buf = np.full((129, 300), 0xaa, np.uint8)
    view = buf[:, 3:3 + 257]
    assert view.ctypes.data % 4 == 3
    assert m.render(1, out=view) is view
    assert np.array_equal(view, want) and (buf[:, :3] == 0xaa).all() and (buf[:, 260:] == 0xaa).all()
    # device: the same layout
    dev = torch.full((129 * 300 + 8,), 0xaa, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    m.render(1, out=(dev.data_ptr() + 3, 300))
    got = dev.cpu().numpy()[:129 * 300].reshape(129, 300)
    assert np.array_equal(got[:, 3:260], want) and (got[:, :3] == 0xaa).all() and (got[:, 260:] == 0xaa).all()
    # an aligned, packed destination (whole words are stored) and a one-column grid
    assert np.array_equal(m.render(3), gr.render(h, w, 3))
    g1 = gr.grid(9, 1, 0.05, (0.0, 0.0))
    m1 = _grid_of(product, g1, gr.scanner(PI / 2, 0.1, 1, range_min=0.01, range_max=1.0))
    m1.integrate(np.array([[0.3]], F), gc.pose(0.025, 0.025, 0.0)[None])
    h1, w1 = gr.new_planes(g1)
    gr.integrate(h1, w1, np.array([[0.3]], F), gc.pose(0.025, 0.025, 0.0)[None], gr.scanner(PI / 2, 0.1, 1, 0.01, 1.0), g1)
    assert np.array_equal(m1.render(), gr.render(h1, w1)) and list(m1.render()[:, 0]) == [0] * 6 + [100, 255, 255]


def test_the_scene_of_the_map_aligns_a_scan_like_the_same_points_from_the_host(product):
    """scan-to-map: the exported scene's device arrays handed to set_fixed give the estimate, bit for bit, that the same points
    give when they come from the host through Scene.set"""
    g = gr.grid(129, 257, 0.05, (-1.0, 0.5))
    a0, inc = gc.fan(361)
    sc = gr.scanner(a0, inc, 361, range_min=0.05, range_max=20.0)
    room = gc.room_of(g)
    poses = gc.trajectory(room, 12, seed=60)
    m = _grid_of(product, g, sc)
    m.integrate(gc.room_scans(room, poses, sc), poses)
    b = product.scene_binding(0)
    from_map, from_host = mapping.Scene(b, 2), mapping.Scene(b, 2)
    n = m.to_scene(from_map, 2, 60)
    assert n > 300
    pts, _ = from_map.get()
    from_host.set(np.asarray(pts, F).reshape(-1, 2))
    # a scan from a pose of the trajectory, guessed 8 cm and 3 degrees off
    robot = poses[5].astype(np.float64)
    scan = ar.adapt_laser_scan(gc.room_scans(room, poses[5:6], sc)[0], a0, inc, half_window=0)["points"]
    guess = (robot @ syn.se2(0.08, -0.06, np.deg2rad(3.0))).astype(F)
    X = []
    for fixed in (from_map, from_host):
        al = product.MultiAligner(abi.SE2_RIGHT, device=0)
        si = al.add_slice(cue_config(abi.SE2_RIGHT, abi.SLICE_P2P, 0.3))
        fp, fn, nf = fixed.device_arrays()
        assert nf == n and fn is None
        al.set_cloud_device("set_fixed", si, fp, 16, None, 16, nf)
        al.set_moving(si, scan)
        al.set_moving_in_fixed(guess)
        al.compute()
        assert al.status() == abi.SUCCESS
        X.append(al.moving_in_fixed().copy())
    assert X[0].tobytes() == X[1].tobytes()
    err, err0 = np.abs(X[0].astype(np.float64) - robot).max(), np.abs(guess.astype(np.float64) - robot).max()
    print("scan-to-map: max |X - X_true| = %.3g (guess %.3g)" % (err, err0))
    assert err < err0


def test_misuse_leaves_the_planes_and_every_destination_untouched(product):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    g, sc, poses, ranges, h, w, want = _reference(((7, 5), 3, 64))
    fresh = product.OccupancyGrid(0)
    fresh.set_scan_model(sc["angle_min"], sc["angle_increment"], 64, 0.02, 20.0)
    with pytest.raises(RuntimeError, match="no grid"):
        fresh.integrate(ranges, poses)
    with pytest.raises(RuntimeError, match="no grid"):
        fresh.counts()
    m = _grid_of(product, g, sc)
    m.integrate(ranges, poses)
    out = abi.GridMapResult()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    before = bytes(out)

    def call(scan, weight=1, mem=abi.MEM_HOST, K=3):
        return lib.srrg2_gridmap_integrate_scans(m._h, C.c_void_p(ranges.ctypes.data), K, C.c_void_p(poses.ctypes.data), mem,
                                                 C.byref(scan), weight, C.byref(out))

    def scan_with(**kw):
        s = abi.GridMapScanParams.from_buffer_copy(bytes(m.scan))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    for s, kw in ((scan_with(), dict(weight=0)), (scan_with(), dict(weight=2)), (scan_with(), dict(mem=2)), (scan_with(), dict(K=-1)),
                  (scan_with(range_max=1601.0), {}), (scan_with(range_max=float("inf")), {}), (scan_with(angle_increment=0.0), {}),
                  (scan_with(clear_beyond_max=3), {}), (scan_with(range_min=0.0), {}), (scan_with(num_beams=-1), {})):
        assert call(s, **kw) == E_INVALID, kw
        assert b"gridmap_integrate_scans" in lib.srrg2_amd_last_error() and bytes(out) == before
    _same_planes(m, h, w, "after the refusals")
    assert call(scan_with(range_max=1599.0)) == 0 and bytes(out) != before  # (31 980 cells of 0.05 m pass the cap of 32 000)
    assert out.num_beams_total == 192
    assert call(scan_with(range_max=1599.0), weight=-1) == 0
    _same_planes(m, h, w, "in and out again")
    # render: a stride below a row, a null image; the scene export: a 3-D scene, a percentage out of range
    img = np.full((7, 8), 0xaa, np.uint8)
    assert lib.srrg2_gridmap_render(m._h, 1, C.c_void_p(img.ctypes.data), 4, abi.MEM_HOST) == E_INVALID
    assert lib.srrg2_gridmap_render(m._h, 1, None, 5, abi.MEM_HOST) == E_INVALID
    assert (img == 0xaa).all()
    b = product.scene_binding(0)
    s3, s2 = mapping.Scene(b, 3), mapping.Scene(b, 2)
    s3.set(np.ones((4, 3), F))
    s2.set(np.ones((5, 2), F))
    with pytest.raises(RuntimeError, match="2-D scene"):
        m.to_scene(s3)
    with pytest.raises(RuntimeError, match="occupied_percent"):
        m.to_scene(s2, 1, 101)
    assert s3.size() == 4 and s2.size() == 5
    assert m.to_scene(s2) == len(gr.to_scene(h, w, g)[1])  # (and a good call replaces the content)
    # an empty grid takes every call and does nothing
    e = product.OccupancyGrid(0)
    e.reset(0, 9)
    e.set_scan_model(sc["angle_min"], sc["angle_increment"], 64, 0.02, 20.0)
    res = e.integrate(ranges, poses)
    assert res["num_beams_total"] == 192 and res["num_hits_in_grid"] == 0 and res["num_miss_updates"] == 0
    assert res["num_returns"] == want["num_returns"]
    assert e.counts()[0].shape == (0, 9) and e.render().shape == (0, 9) and e.to_scene(s2) == 0 and s2.size() == 0
    # reset gives an empty map of the new shape
    m.reset(5, 7, 0.1, (0.0, 0.0))
    assert m.counts()[0].shape == (5, 7) and not m.counts()[0].any() and not m.counts()[1].any()
