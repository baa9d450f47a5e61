"""CPU: the numpy restatement of the measurement adaptors (tests/adaptor_restatement.py, DESIGN.md section 4 "Measurement
adaptors") against the analytic scenes of synthetic.py and against hand-made cases for every rule; the srrg2_adapt_* exports
and the layout of their structs.  The GPU suite (test_gpu_adaptors.py) holds the library to this restatement bit for bit.

Bounds: a numpy draft of the contract gave 4.8e-7 m / 0.034 deg (float32 depth, gap 1, normals on 91.6 % of the valid
pixels), p99 1.47 deg / max 2.04 deg (uint16 millimetres, gap 3; gap 1: max 6.4 deg), and for the scan normals on 99.2 % of
the beams with median and p99 0.000 deg; the asserted bounds are those with margin for a conforming restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import adaptor_restatement as ar
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _angles_deg(a, b):
    c = np.clip(np.sum(a.astype(np.float64) * b.astype(np.float64), axis=1), -1.0, 1.0)
    return np.degrees(np.arccos(c))


def _rgbd():
    d = syn.rgbd_pair()
    depth = np.ascontiguousarray(d["fixed"][:, 2].reshape(d["rows"], d["cols"]), F)
    return d, depth


def test_float_depth_reproduces_the_analytic_cloud():
    d, depth = _rgbd()
    r = ar.adapt_depth_image(depth, d["K"], depth_min=d["depth_min"], depth_max=d["depth_max"], col_gap=1, row_gap=1,
                             max_distance_squared=0.0625, drop_points_without_normal=False)
    finite = np.isfinite(d["fixed"]).all(axis=1)
    assert np.array_equal(r["depth_valid"], finite) and np.array_equal(r["valid"], finite)
    err = np.max(np.abs(r["points"][finite].astype(np.float64) - d["fixed"][finite]))
    hn = r["has_normal"]
    ang = _angles_deg(r["normals"][hn], d["fixed_normals"][hn])
    share = hn.sum() / finite.sum()
    print("coords max err %.3g m, normals max %.4f deg, share %.4f" % (err, ang.max(), share))
    assert err < 1e-6
    assert ang.max() < 0.1
    assert share >= 0.90
    assert np.all(np.isnan(r["normals"][~hn]))
    assert r["num_raw"] == depth.size and r["num_in_range"] == finite.sum() == r["num_valid"]
    # unit normals that face the sensor
    n, p = r["normals"][hn].astype(np.float64), r["points"][hn].astype(np.float64)
    assert np.max(np.abs(np.linalg.norm(n, axis=1) - 1.0)) < 1e-6 and np.all(np.sum(n * p, axis=1) <= 0)


def test_quantised_depth_shows_why_the_gap_exists():
    d, depth = _rgbd()
    mm = np.where(np.isfinite(depth), np.rint(depth.astype(np.float64) * 1000.0), 0).astype(np.uint16)
    worst = {}
    for gap in (1, 3):
        r = ar.adapt_depth_image(mm, d["K"], depth_scale=0.001, depth_min=d["depth_min"], depth_max=d["depth_max"], col_gap=gap,
                                 row_gap=gap, max_distance_squared=0.0625, drop_points_without_normal=False)
        hn = r["has_normal"]
        ang = _angles_deg(r["normals"][hn], d["fixed_normals"][hn])
        worst[gap] = ang.max()
        print("gap %d: p99 %.3f deg, max %.3f deg, normals on %d pixels" % (gap, np.percentile(ang, 99), ang.max(), hn.sum()))
    assert worst[3] < 3.0
    assert worst[3] < worst[1]


def test_scan_reproduces_the_analytic_normals():
    pts, normals = syn.scan_2d(syn.se2(0, 0, 0), beams=1000)
    assert pts.shape[0] == 1000  # (a closed room: every beam hits)
    ranges = np.linalg.norm(pts, axis=1).astype(F)
    bearings = np.deg2rad(np.linspace(-135.0, 135.0, 1000))
    r = ar.adapt_laser_scan(ranges, bearings[0], bearings[1] - bearings[0], range_min=0.05, range_max=30.0, half_window=1,
                            max_distance_squared=0.01, drop_points_without_normal=False)
    hn = r["has_normal"]
    ang = _angles_deg(r["normals"][hn], normals[hn].astype(F))
    share = hn.sum() / 1000.0
    print("scan: share %.4f, median %.4f deg, p99 %.4f deg, max %.2f deg" % (share, np.median(ang), np.percentile(ang, 99), ang.max()))
    assert share >= 0.98
    assert np.percentile(ang, 99) < 0.1
    assert np.max(np.abs(r["points"].astype(np.float64) - pts)) < 1e-5


def test_sincos_restatement_matches_libm():
    x = np.linspace(-7.0, 7.0, 20001)
    s, c = ar.sincos(x)
    assert np.max(np.abs(s - np.sin(x))) < 1e-15 * 4 and np.max(np.abs(c - np.cos(x))) < 1e-15 * 4


# ---- hand-made cases: one rule each -----------------------------------------------------------------------------------------
K5 = np.array([[2.0, 0, 2.0], [0, 2.0, 2.0], [0, 0, 1.0]], F)


def _flat(z=1.0, rows=5, cols=5):
    return np.full((rows, cols), z, F)


def _run5(depth, **kw):
    args = dict(depth_min=0.5, depth_max=4.0, col_gap=1, row_gap=1, max_distance_squared=1.0, drop_points_without_normal=True)
    args.update(kw)
    return ar.adapt_depth_image(depth, K5, **args)


def test_flat_wall_interior_and_border():
    r = _run5(_flat())
    hn = r["has_normal"].reshape(5, 5)
    assert hn[1:4, 1:4].all() and hn.sum() == 9  # a neighbour outside the image: no normal
    assert np.array_equal(r["valid"], r["has_normal"]) and r["num_in_range"] == 25 and r["num_valid"] == 9
    n = r["normals"].reshape(5, 5, 3)[2, 2]
    assert np.array_equal(n, np.array([0, 0, -1], F))  # flipped to face the sensor (dc x dr = +z)
    p = r["points"].reshape(5, 5, 3)
    assert np.array_equal(p[2, 3], np.array([0.5, 0.0, 1.0], F)) and np.isnan(p[0, 0]).all()
    keep = _run5(_flat(), drop_points_without_normal=False)
    assert keep["num_valid"] == 25 and np.isnan(keep["normals"].reshape(5, 5, 3)[0, 0]).all()
    assert np.array_equal(keep["points"].reshape(5, 5, 3)[0, 0], np.array([-1.0, -1.0, 1.0], F))


def test_raw_zero_bounds_nan_and_inf():
    mm = np.full((5, 5), 1000, np.uint16)
    mm[2, 2] = 0  # no reading
    mm[0, 0], mm[0, 1], mm[0, 2], mm[0, 3] = 500, 4000, 499, 4001
    r = ar.adapt_depth_image(mm, K5, depth_scale=0.001, depth_min=0.5, depth_max=4.0, col_gap=0, row_gap=0)
    dv = r["depth_valid"].reshape(5, 5)
    assert not dv[2, 2] and dv[0, 0] and dv[0, 1] and not dv[0, 2] and not dv[0, 3]  # both bounds inclusive
    assert r["normals"] is None and r["num_valid"] == 22
    f = _flat()
    f[1, 1], f[1, 2], f[1, 3] = np.nan, np.inf, -np.inf
    assert not _run5(f, col_gap=0, row_gap=0)["depth_valid"].reshape(5, 5)[1, 1:4].any()


def test_depth_step_beyond_the_gate():
    f = _flat()
    f[:, 3:] = 3.0  # a 2 m step between columns 2 and 3
    hn = _run5(f, max_distance_squared=1.0)["has_normal"].reshape(5, 5)
    assert hn[1:4, 1].all() and not hn[1:4, 2].any() and not hn[1:4, 3].any()
    assert _run5(f, max_distance_squared=100.0)["has_normal"].reshape(5, 5)[1:4, 1:4].all()


def test_no_cascade_when_a_point_is_dropped():
    f = _flat(rows=7, cols=7)
    f[3, 3] = np.nan
    r = ar.adapt_depth_image(f, K5, depth_min=0.5, depth_max=4.0, max_distance_squared=1.0)
    hn = r["has_normal"].reshape(7, 7)
    # the hole knocks out its four neighbours' normals, and they are dropped -- but they stay depth-valid for THEIR neighbours
    for rr, cc in ((2, 3), (4, 3), (3, 2), (3, 4)):
        assert not hn[rr, cc] and not r["valid"].reshape(7, 7)[rr, cc]
    assert hn[2, 2] and hn[1, 3] and hn[3, 1] and hn.sum() == 25 - 5


def test_compact_order_and_global_indices():
    f = _flat()
    f[2, 2] = np.nan
    org = _run5(f, col_gap=0, row_gap=0, intensity=np.arange(25, dtype=np.uint8).reshape(5, 5))
    cmp_ = _run5(f, col_gap=0, row_gap=0, compact=True, intensity=np.arange(25, dtype=np.uint8).reshape(5, 5))
    g = cmp_["global_indices"]
    assert np.array_equal(g, np.array([i for i in range(25) if i != 12], np.int32))
    assert ar.same_bits(cmp_["points"], org["points"][g]) and np.array_equal(cmp_["intensity"], g.astype(F))
    assert org["intensity"].shape == (25,) and cmp_["num_valid"] == 24 == len(g)


def test_seven_beam_scan_rules():
    inc = np.deg2rad(1.0)
    rng = np.array([2.0, 2.0, 2.0, np.nan, 2.0, 0.04, 30.5], F)
    r = ar.adapt_laser_scan(rng, -3 * inc, inc, range_min=0.05, range_max=30.0, half_window=1, max_distance_squared=0.01)
    assert np.array_equal(r["depth_valid"], [True, True, True, False, True, False, False])
    assert np.array_equal(r["has_normal"], [False, True, False, False, False, False, False])  # ends, and neighbours of bad beams
    assert r["num_valid"] == 1 and np.isnan(r["points"][0]).all()
    n, p = r["normals"][1], r["points"][1]
    assert abs(np.hypot(*n) - 1) < 1e-6 and n @ p < 0 and abs(n[0] + np.cos(2 * inc)) < 1e-3
    # the chord gate, the inclusive range bounds, compaction
    far = ar.adapt_laser_scan(np.array([2.0, 2.0, 9.0], F), 0.0, inc, half_window=1, max_distance_squared=0.01)
    assert not far["has_normal"].any()
    edge = ar.adapt_laser_scan(np.array([0.05, 30.0, np.inf], F), 0.0, inc, half_window=0)
    assert np.array_equal(edge["depth_valid"], [True, True, False]) and edge["normals"] is None
    keep = ar.adapt_laser_scan(rng, -3 * inc, inc, half_window=1, drop_points_without_normal=False, compact=True)
    assert np.array_equal(keep["global_indices"], [0, 1, 2, 4]) and keep["points"].shape == (4, 2)
    assert np.isnan(keep["normals"][0]).all() and np.isfinite(keep["normals"][1]).all()
    w3 = ar.adapt_laser_scan(np.full(7, 2.0, F), -3 * inc, inc, half_window=3, max_distance_squared=1.0)
    assert np.array_equal(w3["has_normal"], [False, False, False, True, False, False, False])
    assert abs(w3["normals"][3][0] + 1) < 1e-6 and abs(w3["normals"][3][1]) < 1e-6


# ---- the exports ---------------------------------------------------------------------------------------------------------
def test_adapt_symbols_are_exported_and_structs_match(tmp_path):
    from srrg2_slam_interfaces_amd import _capi

    lib = _capi.lib()
    for n in ("srrg2_adapt_default_depth_params", "srrg2_adapt_default_scan_params", "srrg2_adapt_depth_image", "srrg2_adapt_laser_scan"):
        assert hasattr(lib, n), "missing export: " + n
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "srrg2_slam_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(srrg2_depth_adaptor_params), sizeof(srrg2_scan_adaptor_params), sizeof(srrg2_adapt_result)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(abi.DepthAdaptorParams), C.sizeof(abi.ScanAdaptorParams), C.sizeof(abi.AdaptResult)]
    assert sizes == [9 * 4 + 10 * 4, 2 * 8 + 6 * 4, 5 * 4]
    # the defaults come from the library (no GPU needed)
    from srrg2_slam_interfaces_amd import adaptors

    d, s = adaptors.default_depth_params(), adaptors.default_scan_params()
    assert (d.depth_scale, d.normal_col_gap, d.normal_row_gap, d.drop_points_without_normal, d.compact) == (F(0.001), 1, 1, 1, 0)
    assert (d.depth_min, d.depth_max, d.normal_max_distance_squared) == (F(0.4), 8.0, 0.0625)
    assert (s.normal_half_window, s.drop_points_without_normal, s.compact, s.normal_max_distance_squared) == (1, 1, 0, F(0.01))
    # no adaptor export begins with srrg2_aligner_ (those need an oracle twin)
    hdr = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    assert not re.findall(r"\bsrrg2_aligner_adapt", hdr)
