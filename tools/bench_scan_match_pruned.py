#!/usr/bin/env python3
"""Side bench of pruned scan matching: srrg2_gridmap_build_bounds and srrg2_gridmap_match_scans_pruned against
srrg2_gridmap_match_scans on the same window in the same session, on the floors of tools/bench_scan_match.py -- 2 000 x 2 000
cells of 0.05 m, a scanner of 1 081 beams over 270 degrees, a background of 200 scans drawn into the map, a field of radius 4.
It reports
  build_bounds_L4_ms / _L6_ms   median HOST WALL CLOCK of srrg2_gridmap_build_bounds followed by a wait for the grid's stream,
                       [min, max] over the calls
  window settings      K = 1 and K = 32 at +-2 m / +-20 degrees / 0.5 degrees, the guess a seeded offset from the true pose:
                       pruned_ms (4 levels) and exhaustive_ms, the blocking calls with ranges and guesses in host memory,
                       ALTERNATING call by call
  whole-map settings   K = 1, the window of ``localize`` at 1 degree (2 001 x 2 001 x 361 candidates), the level count swept
                       from 1 to 6; the exhaustive call on that window runs --whole-map-calls times (it takes a third of a second)
  stats                srrg2_gridmap_prune_stats of scan 0 next to the times; speedup = exhaustive median / pruned median
Every pruned result must equal the exhaustive one or the bench stops.  Per-kernel times are not measured here: every figure is
a whole call.  One JSON line on stdout, also written to --out (default profiles/scan_match_pruned_bench.json).

    python tools/bench_scan_match_pruned.py [--calls 10] [--whole-map-calls 3] [--tag NAME] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import bench_gridmap as bg  # noqa: E402
import gridmap_cases as gc  # noqa: E402
import gridmap_restatement as gr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _capi  # noqa: E402

ROWS = COLS = 2000
MEMBERS = ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")


def same(a, b, what):
    if a["robot_in_world"].tobytes() != b["robot_in_world"].tobytes() or any(not np.array_equal(a[k], b[k]) for k in MEMBERS):
        raise SystemExit("bench_scan_match_pruned: the pruned result differs from the exhaustive one (%s)" % what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--whole-map-calls", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_match_pruned_bench.json"))
    args = ap.parse_args()
    a0, inc = gc.fan(bg.BEAMS)
    sc = gr.scanner(a0, inc, bg.BEAMS, range_min=0.05, range_max=bg.RANGE_MAX)
    m = pkg.OccupancyGrid(0)
    m.reset(ROWS, COLS, bg.RES)
    m.set_scan_model(a0, inc, bg.BEAMS, 0.05, bg.RANGE_MAX)
    bg_poses, bg_ranges = bg.floor_scans(ROWS, COLS, 200, sc, seed=8)
    m.integrate(bg_ranges, bg_poses)
    m.build_likelihood(1, 50, 4)
    out = {"bench": "scan_match_pruned", "tag": args.tag, "calls": args.calls, "whole_map_calls": args.whole_map_calls,
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(_capi.LIB_PATH), "rows": ROWS, "cols": COLS,
           "resolution": bg.RES, "beams": bg.BEAMS, "per_kernel_times": "not measured", "settings": []}

    def build(levels):
        m.build_bounds(levels)
        m.device_arrays()  # (waits for the grid's stream, copies nothing)

    for _ in range(2):
        build(4), build(6)
    times = {4: [], 6: []}
    for _ in range(args.calls):
        for levels in (4, 6):
            times[levels].append(bg.timed_ms(lambda: build(levels)))
    for levels in (4, 6):
        out["build_bounds_L%d_ms" % levels], out["build_bounds_L%d_minmax" % levels] = bg.summary(times[levels])
    out["bounds_bytes_L6"] = int(sum((ROWS + 2 ** l - 1) * (COLS + 2 ** l - 1) for l in range(1, 7)))

    def setting(name, ranges, guesses, window, ht, step, levels, calls_pruned, calls_full, full=None):
        res = {}

        def pruned():
            res["pruned"] = m.match_scans_pruned(ranges, guesses, window, ht, step, levels, want_stats=True)

        def exhaustive():
            res["full"] = m.match_scans(ranges, guesses, window, ht, step)

        t = {"pruned": [], "full": []}
        pruned()  # warm-up
        if full is None:
            exhaustive()
        else:
            res["full"] = full["res"]
        for i in range(max(calls_pruned, calls_full if full is None else 0)):  # alternating call by call
            if i < calls_pruned:
                t["pruned"].append(bg.timed_ms(pruned))
            if full is None and i < calls_full:
                t["full"].append(bg.timed_ms(exhaustive))
        same(res["pruned"], res["full"], name)
        row = {"setting": name, "scans": int(len(guesses)), "half_window_cells": list(window), "half_steps_theta": ht,
               "theta_step_degrees": round(math.degrees(step), 3), "levels": levels, "same_as_exhaustive": True}
        row["pruned_ms"], row["pruned_minmax"] = bg.summary(t["pruned"])
        if full is None:
            row["exhaustive_ms"], row["exhaustive_minmax"] = bg.summary(t["full"])
            row["exhaustive_calls"] = calls_full
        else:
            row["exhaustive_ms"], row["exhaustive_minmax"], row["exhaustive_calls"] = full["ms"], full["minmax"], full["calls"]
        row["speedup"] = float("%.4g" % (row["exhaustive_ms"] / row["pruned_ms"]))
        row["stats_scan0"] = res["pruned"]["stats"][0]
        row["fell_back"] = int(sum(s["fell_back"] for s in res["pruned"]["stats"]))
        row["best"] = {k: [int(v) for v in res["full"][k][:4]] for k in ("dx", "dy", "jtheta", "score", "score_at_guess")}
        out["settings"].append(row)
        return {"res": res["full"], "ms": row["exhaustive_ms"], "minmax": row["exhaustive_minmax"], "calls": row["exhaustive_calls"]}

    build(6)
    rng = np.random.default_rng(10)
    for K in (1, 32):
        poses, ranges = bg.floor_scans(ROWS, COLS, K, sc, seed=9)
        off = rng.uniform(-1.0, 1.0, (K, 3)) * (1.5, 1.5, math.radians(15.0))
        guesses = np.stack([p @ gc.pose(*o) for p, o in zip(poses, off)]).astype(np.float32)
        setting("window", ranges, guesses, (40, 40), 40, math.radians(0.5), 4, args.calls, args.calls)
    poses, ranges = bg.floor_scans(ROWS, COLS, 1, sc, seed=11)
    step = math.radians(1.0)
    guesses = m.centre_pose()[None]
    full = None
    for levels in (6, 5, 4, 3, 2, 1):
        full = setting("whole_map", ranges, guesses, (COLS // 2, ROWS // 2), int(math.ceil(math.pi / step)), step, levels, args.calls,
                       args.whole_map_calls, full)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
