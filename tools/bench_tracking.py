#!/usr/bin/env python3
"""Side bench of the feature tracker: srrg2_scene_track_features on seeded frames (tests/features_cases.py rectangles) of 640 x 480
and 1280 x 720.  The measurement is the image adaptor's extraction on the device, capped at 1000 keypoints and uncapped; the
landmarks are that extraction's own keypoints at seeded depths, seen from a pose a few pixels off, their descriptors with up to 30
bits flipped, shuffled -- as many landmarks as keypoints.  Per frame, size, search radius (8, 32, 128) and cross check (on, off):
  track_ms           median HOST WALL CLOCK of the blocking call with result and records on reused scenes (device time plus the
                     call's one host wait); track_minmax is [min, max] over the calls
  unwindowed_ms      DescriptorDatabase.match_scene of the same keypoints against the landmarks as ONE map (no window, no pose):
                     the matcher a caller would otherwise reach for; per frame and size, it has no radius
  restatement_ms     tests/tracking_restatement.py (numpy, one thread) on the same inputs, once -- with the cap only (its
                     all-pairs table is too large for the uncapped counts); the counters must agree
  pairs, band_fill   evaluated (landmark, keypoint) pairs per call, and their share of the keypoints in the landmarks' row bands
                     (what the lanes walk): the case for or against a column-binned cell table
One JSON line on stdout, also written to profiles/tracking_bench.json.

    python tools/bench_tracking.py [--calls 20] [--sizes 480x640,720x1280] [--tag NAME] [--no-restatement]
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

import features_cases as fc  # noqa: E402
import tracking_cases as tc  # noqa: E402
import tracking_restatement as tr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import adaptors, mapping  # noqa: E402

RADII = (8, 32, 128)
F = np.float32


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(t):
    """-> (median, [min, max]), rounded"""
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def band_fill(points, pose, K, rows, cols, pixels, radius):
    """(evaluated pairs, keypoints in the row bands) summed over the in-view landmarks, from count tables (no all-pairs table)"""
    in_view, rv, cu = tr.project(points, pose, K, rows, cols, 0.4, 8.0)
    rv, cu = rv[in_view], cu[in_view]
    count = np.zeros((rows + 1, cols + 1), np.int64)
    np.add.at(count, (pixels // cols + 1, pixels % cols + 1), 1)
    S = count.cumsum(0).cumsum(1)
    r0, r1 = np.maximum(rv - radius, 0), np.minimum(rv + radius, rows - 1) + 1
    c0, c1 = np.maximum(cu - radius, 0), np.minimum(cu + radius, cols - 1) + 1
    pairs = S[r1, c1] - S[r0, c1] - S[r1, c0] + S[r0, c0]
    band = S[r1, cols] - S[r0, cols]
    return int(pairs.sum()), int(band.sum())


def bench_frame(b, rows, cols, calls, restate, warmup=3):
    img = fc.rectangles(rows, cols, rows + cols)
    K = (0.8 * cols, 0.0, (cols - 1) / 2.0, 0.0, 0.8 * cols, (rows - 1) / 2.0, 0.0, 0.0, 1.0)
    row = {"rows": rows, "cols": cols, "sizes": []}
    for max_features in (1000, 0):
        meas = mapping.Scene(b, 3)
        ad = adaptors.MeasurementAdaptorImageFeatures()
        ad.set_camera_matrix(K)
        ad.params.max_features = max_features
        ad.set_meas(meas)
        ad.set_raw_data(img)
        ad.compute()
        pix, fd = meas.global_indices().astype(np.int64), meas.features()[0]
        n = len(pix)
        rng = np.random.default_rng(rows + cols + max_features)
        T = tc.pose(rows)
        order = rng.permutation(n)
        P = tc.landmarks_at(pix[order], cols, K, rng.uniform(1.0, 4.0, n), T)
        md = fd[order].copy()
        for k in range(n):
            md[k] = tc.flipped(md[k], rng.integers(0, 31))
        seen = T.copy()
        seen[:, 3] += np.array([0.01, -0.008, 0.005], F)  # a few pixels at these depths
        moving = mapping.Scene(b, 3)
        moving.set(P)
        moving.set_features(md)
        size = {"max_features": max_features, "num_landmarks": n, "num_keypoints": n, "settings": []}
        db = pkg.DescriptorDatabase()
        db.add_scene(moving)
        for _ in range(warmup):
            db.match_scene(meas, max_distance=48.0)
        tu = [timed_ms(lambda: db.match_scene(meas, max_distance=48.0)) for _ in range(calls)]
        size["unwindowed_ms"], size["unwindowed_minmax"] = summary(tu)
        db.close()
        for radius in RADII:
            for cross in (1, 0):
                p = mapping.default_track_params()
                for i, v in enumerate(K):
                    p.camera_matrix[i] = v
                p.image_rows, p.image_cols, p.search_radius, p.cross_check = rows, cols, radius, cross
                ft = mapping.FeatureTracker(b, p)
                ft.set_fixed(meas)
                ft.set_moving(moving)
                ft.set_moving_in_sensor(seen)
                for _ in range(warmup):
                    ft.compute()
                ts = [timed_ms(ft.compute) for _ in range(calls)]
                pairs, band = band_fill(P, seen, K, rows, cols, pix, radius)
                s = {"search_radius": radius, "cross_check": cross, "result": dict(ft.result), "pairs": pairs, "band_keypoints": band,
                     "band_fill": round(pairs / band, 4) if band else None}
                s["track_ms"], s["track_minmax"] = summary(ts)
                if restate and max_features > 0:
                    t0 = time.perf_counter()
                    want = tr.track(P, md, pix, fd, seen, K, rows, cols, search_radius=radius, max_distance=p.max_distance,
                                    min_margin=p.min_margin, cross_check=bool(cross))
                    s["restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    got = {k: ft.result[k] for k in tr.COUNTERS}
                    if got != {k: want[k] for k in tr.COUNTERS} or want["details"]["num_pairs"] != pairs:
                        raise SystemExit("bench_tracking: counters %s, the restatement's %s" % (got, {k: want[k] for k in tr.COUNTERS}))
                    s["same_counters_as_restatement"] = True
                size["settings"].append(s)
        row["sizes"].append(size)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "tracking", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0), "frames": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        out["frames"].append(bench_frame(b, rows, cols, args.calls, not args.no_restatement))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
