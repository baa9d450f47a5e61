#!/usr/bin/env python3
"""Side bench of the lidar frame: srrg2_adapt_lidar_sweep and srrg2_scene_clip_spherical on synthetic sweeps of a room
(tests/lidar_cases.py: 64 x 2048, about 130 k returns, and 32 x 1024).  Per sweep it reports
  adapt_ms          the adaptor, organised and compact, from a host and from a device cloud: median HOST WALL CLOCK of a blocking
                    call with a result on a reused handle (as tools/bench_normals.py: device time plus one round trip)
  pca_path_ms       what a lidar user had before: Scene.set of the point list + estimate_normals at a radius that gives about 10
                    neighbours (+ the same set_fixed); set_ms and normals_ms are its two parts
  set_fixed_ms      the aligner's set_fixed from the adapted scene's device arrays: paid on either path
and per map (points sampled on the room's surfaces and on the wall next door, 100 k and 1 M)
  clip_ms           clip_spherical, field of view only and with a 0.1 m occlusion margin, against clip_ball (range_max of the
                    model), each with the kept count and the set_moving + compute() that follows it.
Every *_ms figure has a twin *_minmax: [min, max] over the same calls, the run-to-run spread of that figure.
Unless --plain-only is given, each sweep also gets "real_sensor": a sweep of the same shape taken by a MOVING sensor whose rings
follow a two-block table (tests/lidar_motion_cases.py: 64 rows = an HDL-64's two blocks of 32), adapted with the table alone,
with table + de-skew from per-point times (separate arrays, and XYZIT records from the host) and with table + de-skew from the
raw azimuth; and each map "spherical_rings_*": the clip through the 64-entry table.  One JSON line on stdout.

    python tools/bench_lidar.py [--calls 20] [--maps 100000,1000000] [--tag NAME] [--plain-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import lidar_cases as lc  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping, synthetic as syn  # noqa: E402

F = np.float32
POSE = lc.pose(3.2, 2.9, 1.1, yaw_deg=20.0, pitch_deg=1.5)


def times_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def median_ms(fn, calls, warmup=3):
    return float(np.median(times_ms(fn, calls, warmup)))


def stats_ms(fn, calls, warmup=3):
    """-> (median, [min, max]), rounded"""
    t = times_ms(fn, calls, warmup)
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def radius_for(pts, k, seed=1):
    """the radius at which a point of the cloud has k neighbours in the median (brute force on a sample of queries)"""
    rng = np.random.default_rng(seed)
    P = pts.astype(np.float64)
    q = P[rng.choice(len(P), min(300, len(P)), replace=False)]
    return float(np.sqrt(np.median([np.partition(((P - x) ** 2).sum(1), k - 1)[k - 1] for x in q])))


def set_model(dst, m):
    dst.azimuth_min, dst.azimuth_increment = float(m.azimuth_min), float(m.azimuth_increment)
    dst.elevation_min, dst.elevation_increment = float(m.elevation_min), float(m.elevation_increment)
    dst.rows, dst.cols, dst.range_min, dst.range_max = m.rows, m.cols, float(m.range_min), float(m.range_max)


def room_map(n, seed):
    """n points on the floor, the ceiling, the four walls, the pillar's faces and the wall next door, in room coordinates"""
    rng = np.random.default_rng(seed)
    X, Y, Z = lc.ROOM
    u, v, face = rng.uniform(size=n), rng.uniform(size=n), rng.integers(0, 8, n)
    x0, x1, y0, y1 = lc.PILLAR
    side = rng.integers(0, 4, n)
    pillar = np.stack([np.choose(side, [x0 + u * (x1 - x0), x0 + u * (x1 - x0), np.full(n, x0), np.full(n, x1)]),
                       np.choose(side, [np.full(n, y0), np.full(n, y1), y0 + u * (y1 - y0), y0 + u * (y1 - y0)]), v * Z], axis=1)
    faces = [np.stack([u * X, v * Y, np.zeros(n)], 1), np.stack([u * X, v * Y, np.full(n, Z)], 1),
             np.stack([np.zeros(n), u * Y, v * Z], 1), np.stack([np.full(n, X), u * Y, v * Z], 1),
             np.stack([u * X, np.zeros(n), v * Z], 1), np.stack([u * X, np.full(n, Y), v * Z], 1), pillar,
             np.stack([np.full(n, X + 0.6), u * Y, v * Z], 1)]
    pts = np.choose(face[:, None], faces).astype(F)
    nrm = np.tile(np.array([0, 0, 1], F), (n, 1))
    return pts, nrm


def bench_adaptor(b, rows, cols, calls):
    sweep = lc.room_sweep(rows, cols, POSE, seed=rows)
    pts, inten, m = sweep["points"], sweep["intensity"], sweep["model"]
    n = len(pts)
    dev = torch.from_numpy(pts).cuda()
    torch.cuda.synchronize()
    scene, plain = mapping.Scene(b, 3), mapping.Scene(b, 3)
    row = {"rows": rows, "cols": cols, "returns": n, "adapt_ms": {}, "adapt_minmax": {}}
    for compact in (0, 1):
        for where in ("host", "device"):
            ad = adaptors.MeasurementAdaptorLidarSweep()
            set_model(ad.params.model, m)
            ad.params.compact = compact
            ad.set_meas(scene)
            ad.set_raw_data(pts if where == "host" else (dev.data_ptr(), 12, n))
            key = "%s_%s" % ("compact" if compact else "organised", where)
            row["adapt_ms"][key], row["adapt_minmax"][key] = stats_ms(ad.compute, calls)
            row["adapt_result"] = dict(ad.last)
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind, c.finder_max_distance = abi.SLICE_P2PLANE, 0.3
    si = al.add_slice(c)

    def set_fixed_from(s):
        cp, cn, k = s.device_arrays()
        al.set_cloud_device("set_fixed", si, cp, 16, cn, 16, k)

    row["set_fixed_ms"] = round(median_ms(lambda: set_fixed_from(scene), calls), 4)
    radius = radius_for(pts, 10)
    res = {}
    row["set_ms"] = round(median_ms(lambda: plain.set(pts), calls), 4)
    row["normals_ms"] = round(median_ms(lambda: res.update(plain.estimate_normals(radius, drop=False)), calls), 4)

    def pca_path():
        plain.set(pts)
        plain.estimate_normals(radius, drop=True)

    row["pca_path_ms"] = round(median_ms(pca_path, calls), 4)
    row["pca_radius"], row["pca_result"] = round(radius, 4), dict(res)
    row["pca_over_adapt_compact_host"] = round(row["pca_path_ms"] / row["adapt_ms"]["compact_host"], 2)
    return row, scene, m


def ring_table(rows):
    import lidar_motion_cases as mc

    return mc.hdl64_table() if rows == 64 else mc.blocks_table(rows, descending=True, first_deg=-20.0)


def bench_real_sensor(b, rows, cols, calls):
    """the same shapes for a moving sensor with a two-block ring table: table alone, table + de-skew (times / XYZIT / azimuth)"""
    import lidar_motion_cases as mc

    e = ring_table(rows)
    sweep = mc.moving_sweep(rows, cols, mc.START, mc.motion(), seed=rows, ring_elevations=e)
    pts, inten, tm, m = sweep["points"], sweep["intensity"], sweep["times"], sweep["model"]
    n = len(pts)
    xyzit = np.ascontiguousarray(np.concatenate([pts, inten[:, None], tm[:, None]], axis=1), F)
    dev, dev_t = torch.from_numpy(pts).cuda(), torch.from_numpy(tm).cuda()
    torch.cuda.synchronize()
    scene = mapping.Scene(b, 3)
    row = {"rows": rows, "cols": cols, "returns": n, "table": "%d entries, %.2f .. %.2f deg" % (rows, np.degrees(e[0]), np.degrees(e[-1])),
           "adapt_ms": {}, "adapt_minmax": {}, "adapt_result": {}}
    variants = (("rings", False, "times"), ("rings_deskew_times", True, "times"), ("rings_deskew_xyzit", True, "xyzit"),
                ("rings_deskew_azimuth", True, None), ("deskew_times_uniform_rows", True, "uniform"))
    for name, deskew, times in variants:
        for compact in (0, 1):
            for where in ("host", "device"):
                if times == "xyzit" and where == "device":
                    continue
                ad = adaptors.MeasurementAdaptorLidarSweep()
                set_model(ad.params.model, m)
                ad.params.compact = compact
                ad.set_meas(scene)
                if times != "uniform":
                    ad.set_ring_elevations(e)
                if deskew:
                    ad.set_motion(sweep["motion"], 1.0, 0.0, 1.0)
                if times == "xyzit":
                    ad.set_raw_data(xyzit)
                elif where == "host":
                    ad.set_raw_data(pts, None, tm if times else None)
                else:
                    ad.set_raw_data((dev.data_ptr(), 12, n), None, (dev_t.data_ptr(), 4) if times else None)
                key = "%s_%s_%s" % (name, "compact" if compact else "organised", where)
                row["adapt_ms"][key], row["adapt_minmax"][key] = stats_ms(ad.compute, calls)
                row["adapt_result"][name] = dict(ad.last)
    return row


def bench_clipper(b, meas, m, n_map, calls, rings=None):
    pts, nrm = room_map(n_map, n_map)
    full, clipped = mapping.Scene(b, 3), mapping.Scene(b, 3)
    full.set(pts, nrm)
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind, c.finder_max_distance = abi.SLICE_P2PLANE, 0.3
    si = al.add_slice(c)
    fp, fn, nf = meas.device_arrays()
    al.set_cloud_device("set_fixed", si, fp, 16, fn, 16, nf)
    row = {"map_points": n_map, "clip_ms": {}}

    def align():
        mp, mn, nm = clipped.device_arrays()
        al.set_cloud_device("set_moving", si, mp, 16, mn, 16, nm)
        al.set_moving_in_fixed(syn.identity(3))
        al.compute()

    clippers = {}
    for name, margin in (("spherical_fov", -1.0), ("spherical_margin_0.1", 0.1)):
        cl = mapping.SceneClipperSpherical(b)
        set_model(cl.params.model, m)
        cl.params.occlusion_margin = margin
        clippers[name] = cl
    clippers["ball"] = mapping.SceneClipperBall(b, range_max=float(m.range_max))
    if rings is not None:
        for name, margin in (("spherical_rings_fov", -1.0), ("spherical_rings_margin_0.1", 0.1)):
            cl = mapping.SceneClipperSpherical(b)
            set_model(cl.params.model, m)
            cl.set_ring_elevations(rings)
            cl.params.occlusion_margin = margin
            clippers[name] = cl
    for name, cl in clippers.items():
        cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(POSE)
        ms, spread = stats_ms(cl.compute, calls)
        row["clip_ms"][name] = {"clip_ms": ms, "clip_minmax": spread, "kept": clipped.size(), "set_moving_compute_ms": round(median_ms(align, max(3, calls // 4)), 4),
                                "correspondences": al.iteration_stats()[-1]["num_correspondences"]}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--maps", default="100000,1000000")
    ap.add_argument("--tag", default="")
    ap.add_argument("--plain-only", action="store_true", help="only the calls an idealised sensor makes (no table, no de-skew)")
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "lidar", "tag": args.tag, "calls": args.calls, "sweeps": [], "maps": []}
    meas = model = None
    for rows, cols in ((64, 2048), (32, 1024)):
        row, scene, m = bench_adaptor(b, rows, cols, args.calls)
        if not args.plain_only:
            row["real_sensor"] = bench_real_sensor(b, rows, cols, args.calls)
        out["sweeps"].append(row)
        if meas is None:
            meas, model = scene, m  # (the 64 x 2048 measurement, compact, from the last adapt)
    for n_map in [int(s) for s in args.maps.split(",") if s]:
        out["maps"].append(bench_clipper(b, meas, model, n_map, args.calls, None if args.plain_only else ring_table(model.rows)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
