#!/usr/bin/env python3
"""Side bench of the occupancy grid: srrg2_gridmap_integrate_scans, srrg2_gridmap_render and srrg2_gridmap_to_scene on seeded
indoor floors -- a lattice of closed 10 m x 8 m rooms drawn at 0.05 m, a scanner of 1 081 beams over 270 degrees and 30 m, seeded
poses in the middle of seeded rooms, 5 mm range noise.  Per case (K scans into a rows x cols grid) it reports
  integrate_host_ms / integrate_device_ms   median HOST WALL CLOCK of the blocking call (with its result) on a reused handle, ranges
                       and poses in host / in device memory; *_minmax is [min, max] over the calls.  Calls ALTERNATE: host +1,
                       device -1, device +1, host -1, so the map returns to its state and every call sees the same neighbours
  updates              cell updates of one call (hits + misses inside the grid, from the call's result)
  updates_per_s        updates / median, host and device.  CONTEXT, a different instruction: the chip's measured rate for no-return
                       FLOAT atomic adds is 1.3 TB/s of added bytes = 3.25e11 dword adds / s; integer no-return adds are not
                       measured anywhere but here
  render_host_ms / render_device_ms / to_scene_ms   the same clock on the same maps (render: destination in host / device memory)
  render_traffic_ms    the floor of render: both planes read once and the image written once at the 6.29 TB/s a float4 copy
                       measures on this chip; planes_zero_read_ms: zeroing and reading the two planes at that rate
  restatement_s        tests/gridmap_restatement.py (numpy, one thread) on the same batch, ONCE, and only for cases of at most
                       --restate-max scans (default 1 000: the K = 5 000 case is left out, it would take minutes); same bits required
`library` names the library that ran: the default one walks the rays wave-merged (csrc/gridmap.hip); the plain walk it was measured
against is a build with -DSRRG2_GRIDMAP_WAVE_MERGE=0 loaded through SRRG2_AMD_LIB (profiles/gridmap_bench_plain.json).
One JSON line on stdout, also written to profiles/gridmap_bench.json.

    python tools/bench_gridmap.py [--calls 10] [--cases 1:2000x2000,1000:2000x2000,5000:4000x4000] [--tag NAME] [--restate-max 1000]
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

import gridmap_cases as gc  # noqa: E402
import gridmap_restatement as gr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _capi, mapping  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: float4 copy measured on MI355X
FLOAT_ATOMIC_RATE = 1.3e12   # bytes / s of no-return float atomic adds (a different instruction: context only)
RES, BEAMS, RANGE_MAX = 0.05, 1081, 30.0
ROOM_W, ROOM_H, WALL = 10.0, 8.0, 0.3


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(t):
    """-> (median, [min, max]), rounded"""
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def floor_scans(rows, cols, K, sc, seed):
    """K poses in seeded rooms of the lattice that fills the grid, and the scans taken there"""
    rng = np.random.default_rng(seed)
    nx, ny = max(int(cols * RES / ROOM_W), 1), max(int(rows * RES / ROOM_H), 1)
    which = rng.integers(0, nx * ny, K)
    poses, ranges = np.zeros((K, 3, 3), np.float32), np.zeros((K, BEAMS), np.float32)
    for r in np.unique(which):
        ix, iy = int(r % nx), int(r // nx)
        room = (ix * ROOM_W + WALL, (ix + 1) * ROOM_W - WALL, iy * ROOM_H + WALL, (iy + 1) * ROOM_H - WALL)
        sel = np.flatnonzero(which == r)
        p = gc.trajectory(room, len(sel), seed * 1000003 + int(r))
        poses[sel] = p
        ranges[sel] = gc.room_scans(room, p, sc, sigma=0.005, seed=seed + int(r))
    return poses, ranges


def bench_case(K, rows, cols, calls, restate, warmup=2):
    g = gr.grid(rows, cols, RES, (0.0, 0.0))
    a0, inc = gc.fan(BEAMS)
    sc = gr.scanner(a0, inc, BEAMS, range_min=0.05, range_max=RANGE_MAX)
    poses, ranges = floor_scans(rows, cols, K, sc, seed=7)
    m = pkg.OccupancyGrid(0)
    m.reset(rows, cols, RES)
    m.set_scan_model(a0, inc, BEAMS, 0.05, RANGE_MAX)
    # the map the per-frame update and the readers work on: a background of 200 scans
    bg_poses, bg_ranges = floor_scans(rows, cols, 200, sc, seed=8)
    m.integrate(bg_ranges, bg_poses)
    dr, dp = torch.from_numpy(ranges).cuda(), torch.from_numpy(poses).cuda()
    torch.cuda.synchronize()
    res = {}

    def host(w):
        res["host"] = m.integrate(ranges, poses, w)

    def device(w):
        res["device"] = m.integrate(dr, dp, w)

    image = np.zeros((rows, cols), np.uint8)
    dimage = torch.empty((rows, cols), dtype=torch.uint8, device="cuda:0")
    scene = mapping.Scene(pkg.scene_binding(0), 2)
    order = (("integrate_host", lambda: host(+1)), ("integrate_device", lambda: device(-1)), ("integrate_device", lambda: device(+1)),
             ("integrate_host", lambda: host(-1)), ("render_host", lambda: m.render(1, out=image)),
             ("render_device", lambda: m.render(1, out=(dimage.data_ptr(), cols))), ("to_scene", lambda: m.to_scene(scene, 2, 60)))
    for _ in range(warmup):
        for _, fn in order:
            fn()
    times = {k: [] for k, _ in order}
    for _ in range(calls):
        for k, fn in order:
            times[k].append(timed_ms(fn))
    row = {"scans": K, "rows": rows, "cols": cols, "beams": BEAMS, "resolution": RES}
    for k, v in times.items():
        row[k + "_ms"], row[k + "_minmax"] = summary(v)
    if res["host"] != res["device"]:
        raise SystemExit("bench_gridmap: the host call's counters %s, the device call's %s" % (res["host"], res["device"]))
    row["result"] = res["host"]
    row["updates"] = res["host"]["num_hits_in_grid"] + res["host"]["num_miss_updates"]
    for k in ("host", "device"):
        row["updates_per_s_" + k] = float("%.4g" % (row["updates"] / (row["integrate_%s_ms" % k] * 1e-3)))
    row["scene_points"] = scene.size()
    cells = rows * cols
    row["render_traffic_ms"] = round(9 * cells / COPY_RATE * 1e3, 5)
    row["planes_zero_read_ms"] = round(16 * cells / COPY_RATE * 1e3, 5)
    if restate:
        h, w = gr.new_planes(g)
        gr.integrate(h, w, bg_ranges, bg_poses, sc, g)
        t0 = time.perf_counter()
        want = gr.integrate(h, w, ranges, poses, sc, g, +1)
        row["restatement_s"] = round(time.perf_counter() - t0, 2)
        m.integrate(ranges, poses, +1)
        hits, misses = m.counts()
        if want != res["host"] or not np.array_equal(hits, h) or not np.array_equal(misses, w) or \
                not np.array_equal(m.render(1), gr.render(h, w, 1)):
            raise SystemExit("bench_gridmap: the planes, the counters or the image differ from the restatement's")
        row["same_as_restatement"] = True
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cases", default="1:2000x2000,1000:2000x2000,5000:4000x4000", help="K:rows x cols, comma separated")
    ap.add_argument("--restate-max", type=int, default=1000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridmap_bench.json"))
    args = ap.parse_args()
    out = {"bench": "gridmap", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "copy_rate_bytes_per_s": COPY_RATE, "float_atomic_rate_bytes_per_s_context_only": FLOAT_ATOMIC_RATE,
           "float_atomic_dword_adds_per_s_context_only": FLOAT_ATOMIC_RATE / 4, "library": os.path.basename(_capi.LIB_PATH), "cases": []}
    for case in args.cases.split(","):
        K, size = case.split(":")
        rows, cols = (int(v) for v in size.split("x"))
        out["cases"].append(bench_case(int(K), rows, cols, args.calls, int(K) <= args.restate_max))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
