#!/usr/bin/env python3
"""Side bench of correlative scan matching: srrg2_gridmap_build_likelihood and srrg2_gridmap_match_scans on the seeded floors of
tools/bench_gridmap.py -- 2 000 x 2 000 cells of 0.05 m, a scanner of 1 081 beams over 270 degrees, a background of 200 scans
drawn into the map, the scans to match taken at seeded poses and handed in with their true pose as the guess (the work does not
depend on where the maximum lies).  It reports
  build_R4_ms / build_R16_ms   median HOST WALL CLOCK of srrg2_gridmap_build_likelihood followed by a wait for the grid's stream
                       (srrg2_gridmap_device_arrays: the call itself only queues), [min, max] over the calls; field_traffic_ms: both planes read and the
                       field written once at the 6.29 TB/s a float4 copy measures on this chip
  per setting (K scans, half windows in cells, rotations): match_{host,device}[_volume]_ms, the blocking call with its results,
                       ranges and guesses in host / device memory, without and with the whole score volume (to host memory for
                       the host variant, to device memory for the device one); the four ALTERNATE call by call
  lookups              candidates x scored beams, summed over the scans; lookups_per_s_* = lookups / median
  traffic_ms           the floor of a call that looked every byte up once: the field read once plus the volume written once at
                       the copy rate (the volume's share is volume_traffic_ms)
  restatement_s        tests/scan_match_restatement.py (numpy, one thread) on the smallest setting, ONCE; same bits required
`library` names the library that ran: the default one scores by tiles of the window (csrc/scan_match.hip); the plain kernel it is
measured against is a build with -DSRRG2_SCAN_MATCH_PLAIN=1 loaded through SRRG2_AMD_LIB (profiles/scan_match_bench_plain.json).
Per-kernel times are not measured here: every figure is a whole call.
One JSON line on stdout, also written to --out (default profiles/scan_match_bench.json).

    python tools/bench_scan_match.py [--calls 10] [--tag NAME] [--out FILE] [--no-restatement]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import bench_gridmap as bg  # noqa: E402
import gridmap_cases as gc  # noqa: E402
import gridmap_restatement as gr  # noqa: E402
import scan_match_restatement as sm  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _capi  # noqa: E402

ROWS = COLS = 2000
STEP = math.radians(0.5)
# (K, half window in cells, half steps): +-0.5 m / +-10 degrees, +-2 m / +-20 degrees, at 0.5 degrees
SETTINGS = ((1, 10, 20), (1, 40, 40), (32, 40, 40))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_match_bench.json"))
    args = ap.parse_args()
    g = gr.grid(ROWS, COLS, bg.RES, (0.0, 0.0))
    a0, inc = gc.fan(bg.BEAMS)
    sc = gr.scanner(a0, inc, bg.BEAMS, range_min=0.05, range_max=bg.RANGE_MAX)
    m = pkg.OccupancyGrid(0)
    m.reset(ROWS, COLS, bg.RES)
    m.set_scan_model(a0, inc, bg.BEAMS, 0.05, bg.RANGE_MAX)
    bg_poses, bg_ranges = bg.floor_scans(ROWS, COLS, 200, sc, seed=8)
    m.integrate(bg_ranges, bg_poses)
    out = {"bench": "scan_match", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "copy_rate_bytes_per_s": bg.COPY_RATE, "library": os.path.basename(_capi.LIB_PATH), "rows": ROWS, "cols": COLS,
           "resolution": bg.RES, "beams": bg.BEAMS, "theta_step_degrees": 0.5, "per_kernel_times": "not measured", "settings": []}
    cells = ROWS * COLS

    def build(R):
        m.build_likelihood(1, 50, R)
        m.device_arrays()  # (waits for the grid's stream, copies nothing)

    for _ in range(2):
        build(4), build(16)
    times = {4: [], 16: []}
    for _ in range(args.calls):
        for R in (4, 16):
            times[R].append(bg.timed_ms(lambda: build(R)))
    for R in (4, 16):
        out["build_R%d_ms" % R], out["build_R%d_minmax" % R] = bg.summary(times[R])
    out["field_traffic_ms"] = round(9 * cells / bg.COPY_RATE * 1e3, 5)
    build(4)
    for K, w, ht in SETTINGS:
        poses, ranges = bg.floor_scans(ROWS, COLS, K, sc, seed=9)
        dr, dp = torch.from_numpy(ranges).cuda(), torch.from_numpy(poses).cuda()
        nc = (2 * w + 1) ** 2 * (2 * ht + 1)
        dvol = torch.empty((K * nc,), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        res = {}

        def run(name, r, p, scores):
            res[name] = m.match_scans(r, p, (w, w), ht, STEP, want_scores=scores)

        order = (("match_host", lambda: run("host", ranges, poses, False)), ("match_device_volume", lambda: run("device_volume", dr, dp, dvol)),
                 ("match_device", lambda: run("device", dr, dp, False)), ("match_host_volume", lambda: run("host_volume", ranges, poses, True)))
        for _ in range(2):
            for _, fn in order:
                fn()
        t = {k: [] for k, _ in order}
        for _ in range(args.calls):
            for k, fn in order:
                t[k].append(bg.timed_ms(fn))
        row = {"scans": K, "half_window_cells": w, "half_steps_theta": ht, "candidates_per_scan": nc}
        for k, v in t.items():
            row[k + "_ms"], row[k + "_minmax"] = bg.summary(v)
        for a in ("device", "device_volume", "host_volume"):
            for k in ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams"):
                if not np.array_equal(res["host"][k], res[a][k]):
                    raise SystemExit("bench_scan_match: %s differs between the host call and the %s call" % (k, a))
        if not np.array_equal(res["host_volume"]["scores"].reshape(-1), dvol.cpu().numpy()):
            raise SystemExit("bench_scan_match: the volume in host memory differs from the one in device memory")
        row["lookups"] = int(res["host"]["num_scored_beams"].astype(np.int64).sum()) * nc
        for k, _ in order:
            row["lookups_per_s_" + k[6:]] = float("%.4g" % (row["lookups"] / (row[k + "_ms"] * 1e-3)))
        row["best"] = {k: [int(v) for v in res["host"][k][:4]] for k in ("dx", "dy", "jtheta", "score", "score_at_guess")}
        row["volume_traffic_ms"] = round(4 * K * nc / bg.COPY_RATE * 1e3, 5)
        row["traffic_ms"] = round((cells + 4 * K * nc) / bg.COPY_RATE * 1e3, 5)
        if not args.no_restatement and (K, w, ht) == SETTINGS[0]:
            h, miss = m.counts()
            t0 = time.perf_counter()
            field = sm.likelihood(h, miss, 1, 50, 4, sm.default_lut(4))
            want = sm.match(field, ranges, poses, sc, g, w, w, ht, STEP)
            row["restatement_s"] = round(time.perf_counter() - t0, 2)
            got = res["host_volume"]
            if not np.array_equal(m.likelihood(), field) or not np.array_equal(got["scores"], want["scores"]) or \
                    got["robot_in_world"].tobytes() != want["robot_in_world"].tobytes() or \
                    any(not np.array_equal(got[k], want[k]) for k in ("dx", "dy", "jtheta", "score", "score_at_guess", "num_scored_beams")):
                raise SystemExit("bench_scan_match: field, results or volume differ from the restatement's")
            row["same_as_restatement"] = True
        out["settings"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
