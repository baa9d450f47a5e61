#!/usr/bin/env python3
"""Side bench of the TSDF volume: srrg2_tsdf_integrate_frames, srrg2_tsdf_raycast and srrg2_tsdf_to_scene on a seeded box room
(4.8 m x 4.0 m x 5.0 m, rendered analytically: tests/tsdf_cases.py) seen by a 640 x 480 camera from seeded poses near its front.
Per volume side N (N^3 voxels over 5.12 m) it reports
  integrate_k{1,100}_{host,device}_ms   median HOST WALL CLOCK of the blocking call (with its result) on a reused handle, the F32
                       images in host / in device memory; *_minmax is [min, max] over the calls.  Calls ALTERNATE: host +1,
                       device -1, device +1, host -1, so the volume returns to its state and every call sees the same neighbours.
                       K = 1 is the per-frame update, K = 100 the re-integration after an optimisation
  integrate_k*_floor_ms   the traffic floor: the sum and weight planes read and written once (16 bytes per voxel) plus the call's
                       images read once, at the 6.29 TB/s a float4 copy measures on this chip
  k100_over_100_k1     the K = 100 device call next to 100 x the K = 1 device call of the same session
  raycast_skip_ms / raycast_plain_ms   the raycast (depth image and organised scene with normals) from the first pose with and
                       without the block mask, alternating; the two depth images must be the same bits
  to_scene_ms          the export (min_weight 1) into a reused scene
  planes_sha256        of the sum and weight planes after the K = 100 batch: the kept kernel and the plain one must agree
`library` names the library that ran: the default one keeps a voxel's sums in registers over the frames of a call and skips runs
the frustum misses (csrc/tsdf.hip); the plain kernel it was measured against is a build with -DSRRG2_TSDF_PLAIN=1 loaded through
SRRG2_AMD_LIB (profiles/tsdf_bench_plain.json).  One JSON line on stdout, also written to profiles/tsdf_bench.json.

    python tools/bench_tsdf.py [--calls 6] [--sides 256,512] [--frames 100] [--tag NAME] [--out PATH]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import tsdf_cases as tc  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _capi, mapping  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: float4 copy measured on MI355X
ROWS, COLS, EXTENT = 480, 640, 5.12
LO, HI = np.array([-2.4, -2.0, -0.4]), np.array([2.4, 2.0, 4.6])


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(t):
    """-> (median, [min, max]), rounded"""
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def frames(n, seed):
    K = tc.intrinsics(ROWS, COLS, 525.0)
    poses = tc.room_trajectory(n, seed)
    return K, poses, np.stack([tc.render_room(T, K, ROWS, COLS, LO, HI) for T in poses])


def bench_side(side, K, poses, depth, calls, warmup=1):
    vs = EXTENT / side
    t = pkg.TsdfVolume(0)
    t.reset(side, side, side, vs, (-0.5 * EXTENT, -0.5 * EXTENT, -0.4))
    t.set_camera(K, ROWS, COLS, 0.001, 0.4, 8.0)
    t.frame.mu, t.ray.step = 3 * vs, vs
    row = {"side": side, "voxel_size": vs, "mu": 3 * vs, "rows": ROWS, "cols": COLS}
    ddepth = torch.from_numpy(depth).cuda()
    torch.cuda.synchronize()
    voxels = side ** 3
    for n in (1, len(poses)):
        res = {}

        def host(w, n=n):
            res["host"] = t.integrate(depth[:n], poses[:n], weight=w)

        def device(w, n=n):
            res["device"] = t.integrate(ddepth[:n], poses[:n], weight=w)

        order = (("host", lambda: host(+1)), ("device", lambda: device(-1)), ("device", lambda: device(+1)), ("host", lambda: host(-1)))
        for _ in range(warmup):
            for _, fn in order:
                fn()
        times = {"host": [], "device": []}
        for _ in range(calls):
            for k, fn in order:
                times[k].append(timed_ms(fn))
        if res["host"] != res["device"]:
            raise SystemExit("bench_tsdf: the host call's counters %s, the device call's %s" % (res["host"], res["device"]))
        for k, v in times.items():
            row["integrate_k%d_%s_ms" % (n, k)], row["integrate_k%d_%s_minmax" % (n, k)] = summary(v)
        row["integrate_k%d_result" % n] = res["host"]
        row["integrate_k%d_floor_ms" % n] = round((16 * voxels + 4 * n * ROWS * COLS) / COPY_RATE * 1e3, 5)
    row["k100_over_100_k1"] = round(row["integrate_k%d_device_ms" % len(poses)] / (len(poses) * row["integrate_k1_device_ms"]), 4)
    # the model the readers work on: the whole batch
    t.integrate(ddepth, poses)
    planes = t.planes()
    h = hashlib.sha256()
    h.update(planes[0].tobytes())
    h.update(planes[1].tobytes())
    row["planes_sha256"] = h.hexdigest()
    del planes
    scene, cloud = mapping.Scene(pkg.scene_binding(0), 3), mapping.Scene(pkg.scene_binding(0), 3)
    images = {}

    def raycast(skip):
        t.ray.skip_empty = skip
        images[skip], res["raycast"] = t.raycast(poses[0], scene)

    order = (("raycast_skip", lambda: raycast(1)), ("raycast_plain", lambda: raycast(0)), ("to_scene", lambda: t.to_scene(cloud, 1)))
    for _ in range(warmup):
        for _, fn in order:
            fn()
    times = {k: [] for k, _ in order}
    for _ in range(calls):
        for k, fn in order:
            times[k].append(timed_ms(fn))
    if images[0].tobytes() != images[1].tobytes():
        raise SystemExit("bench_tsdf: the raycast with the block mask differs from the plain march")
    for k, v in times.items():
        row[k + "_ms"], row[k + "_minmax"] = summary(v)
    row["raycast_result"] = res["raycast"]
    row["scene_points"] = cloud.size()
    row["to_scene_floor_ms"] = round(8 * voxels / COPY_RATE * 1e3, 5)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--sides", default="256,512")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    args = ap.parse_args()
    K, poses, depth = frames(args.frames, seed=7)
    out = {"bench": "tsdf", "tag": args.tag, "calls": args.calls, "frames": args.frames, "device": torch.cuda.get_device_name(0),
           "copy_rate_bytes_per_s": COPY_RATE, "library": os.path.basename(_capi.LIB_PATH), "cases": []}
    for side in args.sides.split(","):
        out["cases"].append(bench_side(int(side), K, poses, depth, args.calls))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
