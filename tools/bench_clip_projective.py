#!/usr/bin/env python3
"""Side bench of the projective clipper: the clip step of an RGB-D tracker frame, ball policy against projective policy.

The local map is the C3 generator's surface (synthetic.render_depth) seen from a few poses around the measurement's camera and
merged into one cloud in the robot frame, plus the same renders 0.3 m further along the viewing rays (surfaces the camera
cannot see), cut to about 100 k, 271 k and 1 M points.  Per size and per policy -- clip_ball with range = depth_max,
clip_projective frustum only, clip_projective with a 0.05 m occlusion margin -- it reports
  clip_ms        median of the timed calls after warm-up, the `clipped` handle reused (steady state: one wait per clip)
  kept           points in the clipped scene
  align_ms       the following set_moving (device arrays) + compute() of C3's two-slice aligner (projective point-to-plane
                 next to reprojection, 10 iterations) on the clipped cloud, median
  frame_ms       clip_ms + align_ms
and the ratios of the projective clips to the ball clip.  One JSON line on stdout.

    python tools/bench_clip_projective.py [--calls 30] [--align-calls 7] [--sizes 100000,271000,1000000]
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
from srrg2_slam_interfaces_amd import _abi as abi, mapping, synthetic as syn  # noqa: E402

F = np.float32
MARGIN = 0.05
# the robot has moved a little since the map's frame was set: the clipped cloud is off the measurement by this, which the aligner
# has to find (moving_in_fixed = robot_in_local_map)
ROBOT_IN_LOCAL_MAP = syn.se3(np.array([0.03, 0.01, -0.02]), np.deg2rad(np.array([0.5, 1.0, -0.5]))).astype(F)


def local_map(data, target, seed=11):
    """about `target` points (+ normals) in the frame of camera 1 = the robot: renders from poses around camera 1, each with a
    hidden copy behind it, in a fixed shuffled order"""
    rows, cols, K = data["rows"], data["cols"], data["K"].astype(np.float64)
    T1 = np.zeros((3, 4))
    T1[:, :3] = np.diag([1.0, -1.0, -1.0])
    T1[:, 3] = [0.0, 0.0, 4.0]
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    renders = max(3, int(np.ceil(target / (2.0 * 0.95 * rows * cols))))
    for k in range(renders):
        X = syn.se3(rng.uniform(-0.5, 0.5, 3) * (k > 0) + [0.03, 0.01, -0.02], np.deg2rad(rng.uniform(-8, 8, 3) * (k > 0) + [0.5, 1.0, -0.5]))
        P, N = syn.render_depth(syn.se3_mul(T1, X), K, rows, cols)
        ok = (P[:, 2] >= data["depth_min"]) & (P[:, 2] <= data["depth_max"])
        P, N = P[ok], N[ok]
        for Q in (P, P * (1.0 + 0.3 / P[:, 2:3])):  # the render, and the same rays 0.3 m deeper
            pts.append(Q @ X[:, :3].T + X[:, 3])
            nrm.append(N @ X[:, :3].T)
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    sel = np.sort(rng.choice(len(pts), min(target, len(pts)), replace=False))
    return np.ascontiguousarray(pts[sel], F), np.ascontiguousarray(nrm[sel], F)


def make_aligner(data):
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
    al.set_params(max_iterations=10, min_num_inliers=10)
    for sk in (abi.SLICE_P2PLANE, abi.SLICE_REPROJECTION):
        c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
        c.kind, c.finder, c.finder_max_distance = sk, abi.FINDER_PROJECTIVE, 0.05
        for i, v in enumerate(data["K"].reshape(-1)):
            c.camera_matrix[i] = v
        c.image_rows, c.image_cols = data["rows"], data["cols"]
        c.depth_min, c.depth_max = data["depth_min"], data["depth_max"]
        si = al.add_slice(c)
        if si == 0:
            al.set_fixed(si, data["fixed"], data["fixed_normals"])
        else:
            al.share_clouds(si, 0)
    return al


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
    ap.add_argument("--sizes", default="100000,271000,1000000")
    args = ap.parse_args()
    data = syn.rgbd_pair(seed=3000)
    b = pkg.scene_binding(0)
    al = make_aligner(data)
    out = {"bench": "clip_projective", "image": [data["rows"], data["cols"]], "calls": max(args.calls, 20), "margin": MARGIN, "sizes": []}
    for target in [int(s) for s in args.sizes.split(",")]:
        pts, nrm = local_map(data, target)
        full = mapping.Scene(b, 3)
        full.set(pts, nrm)
        row = {"points": int(len(pts))}
        for name in ("ball", "frustum", "occlusion"):
            clipped = mapping.Scene(b, 3)
            if name == "ball":
                cl = mapping.SceneClipperBall(b, range_max=float(data["depth_max"]))
            else:
                cl = mapping.SceneClipperProjective(b)
                cl.set_camera_matrix(data["K"])
                cl.params.image_rows, cl.params.image_cols = data["rows"], data["cols"]
                cl.params.depth_min, cl.params.depth_max = data["depth_min"], data["depth_max"]
                cl.params.occlusion_margin = MARGIN if name == "occlusion" else -1.0
            cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(ROBOT_IN_LOCAL_MAP)
            clip_ms = median_ms(cl.compute, max(args.calls, 20), 5)

            def align():
                cp, cn, n = clipped.device_arrays()
                al.set_cloud_device("set_moving", 0, cp, 16, cn, 16, n, kept=True)
                al.set_moving_in_fixed(syn.identity(3))
                al.compute()

            align_ms = median_ms(align, args.align_calls, 2)
            err = float(np.max(np.abs(al.moving_in_fixed() - ROBOT_IN_LOCAL_MAP)))
            row[name] = {"clip_ms": round(clip_ms, 4), "kept": clipped.size(), "align_ms": round(align_ms, 4),
                         "frame_ms": round(clip_ms + align_ms, 4), "status": al.status(),
                         "correspondences": al.iteration_stats()[-1]["num_correspondences"], "max_abs_X_minus_expected": round(err, 6)}
        for name in ("frustum", "occlusion"):
            row[name]["clip_vs_ball"] = round(row[name]["clip_ms"] / row["ball"]["clip_ms"], 3)
            row[name]["frame_vs_ball"] = round(row[name]["frame_ms"] / row["ball"]["frame_ms"], 3)
        out["sizes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
