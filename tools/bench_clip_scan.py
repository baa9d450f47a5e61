#!/usr/bin/env python3
"""Side bench of the scan clipper: the clip step of a 2-D laser tracker frame, ball policy against scan policy.

The local map is a floor of 3 x 3 rooms (the C1 room of synthetic.scan_2d in the middle, with its interior boxes, and eight copies
around it behind 0.4 m walls), its walls sampled evenly to about 100 k and 1 M points with normals, in a fixed shuffled order.  The
robot stands in the middle room: everything in the other rooms is within range and hidden.  The scanner has 1081 beams over 270
degrees.  Per size and per policy -- clip_ball with range = range_max, clip_scan sector only, clip_scan with a 0.05 m occlusion
margin -- it reports
  clip_ms        median of the timed calls after warm-up, the `clipped` handle reused (steady state: one wait per clip)
  kept           points in the clipped scene
  align_ms       the following set_moving (device arrays) + compute() of C1's point-to-plane aligner (nearest neighbour finder,
                 10 iterations) on the clipped cloud against the adapted scan, median
  frame_ms       clip_ms + align_ms
and the ratios of the scan clips to the ball clip.  One JSON line on stdout.

    python tools/bench_clip_scan.py [--calls 30] [--align-calls 7] [--sizes 100000,1000000] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: F401,E402  (before the library: tests/conftest.py says why)

import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping, synthetic as syn  # noqa: E402

F = np.float32
MARGIN = 0.05
BEAMS, FOV_DEG = 1081, 270.0
RANGE_MAX = 30.0
# where the robot is, and where the tracker believes it is: the clipped cloud is off the measurement by the difference, which the
# aligner has to find
ROBOT = syn.se2(0.10, 0.05, np.deg2rad(3.0))
BELIEVED = syn.se2(0.08, 0.04, np.deg2rad(2.5)).astype(F)


def local_map(target, seed=11):
    """about `target` wall points (+ normals facing into their room / out of their box) of the 3 x 3 rooms, shuffled"""
    segs = syn._room_segments()  # (S, 2, 2): the outer walls first, then two boxes, four segments each
    inward = np.array([1.0] * 4 + [-1.0] * 8)
    centres = np.array([[0.0, 0.0]] * 4 + [[2.0, 1.6]] * 4 + [[-2.6, -1.9]] * 4)
    all_segs, all_c, all_s = [], [], []
    for ix in (-1, 0, 1):
        for iy in (-1, 0, 1):
            off = np.array([10.4 * ix, 8.4 * iy])
            all_segs.append(segs + off)
            all_c.append(centres + off)
            all_s.append(inward)
    segs, centres, inward = np.concatenate(all_segs), np.concatenate(all_c), np.concatenate(all_s)
    length = np.linalg.norm(segs[:, 1] - segs[:, 0], axis=1)
    per = np.maximum(2, np.round(target * length / length.sum()).astype(int))
    pts, nrm = [], []
    for (a, b), c, s, k in zip(segs, centres, inward, per):
        u = (np.arange(k) + 0.5) / k
        p = a + u[:, None] * (b - a)
        e = (b - a) / np.linalg.norm(b - a)
        nv = np.array([-e[1], e[0]])
        if np.dot(nv, c - 0.5 * (a + b)) * s < 0:
            nv = -nv
        pts.append(p)
        nrm.append(np.tile(nv, (k, 1)))
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    order = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[order], F), np.ascontiguousarray(nrm[order], F)


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--align-calls", type=int, default=7)
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--tag", default="", help="copied into the result (which build of the library this is)")
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    ang = np.deg2rad(np.linspace(-FOV_DEG / 2, FOV_DEG / 2, BEAMS))
    a0, inc = float(ang[0]), float(ang[1] - ang[0])
    ranges = np.linalg.norm(syn.scan_2d(ROBOT, beams=BEAMS, fov_deg=FOV_DEG)[0], axis=1).astype(F)
    meas = mapping.Scene(b, 2)
    p = adaptors.default_scan_params()
    p.angle_min, p.angle_increment, p.compact = a0, inc, 1
    ad = adaptors.MeasurementAdaptorLaserScan(p)
    ad.set_meas(meas); ad.set_raw_data(ranges); ad.compute(False)
    al = pkg.MultiAligner(abi.SE2_RIGHT, device=0)
    al.set_params(max_iterations=10, min_num_inliers=10)
    c = abi.default_slice_config(abi.SE2_RIGHT)
    c.kind, c.finder, c.finder_max_distance, c.robustifier, c.robustifier_chi_threshold = abi.SLICE_P2PLANE, abi.FINDER_NN_GATED, 0.5, abi.ROBUST_CAUCHY, 0.05
    si = al.add_slice(c)
    mp, mn, m = meas.device_arrays()
    al.set_cloud_device("set_fixed", si, mp, 16, mn, 16, m, kept=True)
    X_true = np.linalg.inv(ROBOT) @ BELIEVED.astype(np.float64)
    out = {"bench": "clip_scan", "tag": args.tag, "beams": BEAMS, "fov_deg": FOV_DEG, "calls": max(args.calls, 20), "margin": MARGIN,
           "sizes": []}
    for target in [int(s) for s in args.sizes.split(",")]:
        pts, nrm = local_map(target)
        full = mapping.Scene(b, 2)
        full.set(pts, nrm)
        row = {"points": int(len(pts))}
        for name in ("ball", "sector", "occlusion"):
            clipped = mapping.Scene(b, 2)
            if name == "ball":
                cl = mapping.SceneClipperBall(b, range_max=RANGE_MAX)
            else:
                cl = mapping.SceneClipperScan(b)
                cl.params.angle_min, cl.params.angle_increment, cl.params.num_beams = a0, inc, BEAMS
                cl.params.range_max = RANGE_MAX
                cl.params.occlusion_margin = MARGIN if name == "occlusion" else -1.0
            cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(BELIEVED)
            clip_ms = median_ms(cl.compute, max(args.calls, 20), 5)

            def align():
                cp, cn, n = clipped.device_arrays()
                al.set_cloud_device("set_moving", si, cp, 16, cn, 16, n, kept=True)
                al.set_moving_in_fixed(syn.identity(2))
                al.compute()

            align_ms = median_ms(align, args.align_calls, 2)
            err = float(np.max(np.abs(al.moving_in_fixed() - X_true)))
            row[name] = {"clip_ms": round(clip_ms, 4), "kept": clipped.size(), "align_ms": round(align_ms, 4),
                         "frame_ms": round(clip_ms + align_ms, 4), "status": al.status(),
                         "correspondences": al.iteration_stats()[-1]["num_correspondences"], "max_abs_X_minus_expected": round(err, 6)}
        for name in ("sector", "occlusion"):
            row[name]["clip_vs_ball"] = round(row[name]["clip_ms"] / row["ball"]["clip_ms"], 3)
            row[name]["frame_vs_ball"] = round(row[name]["frame_ms"] / row["ball"]["frame_ms"], 3)
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
