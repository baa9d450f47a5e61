#!/usr/bin/env python
"""Multi-cue batches (srrg2_align_batch_slices): K alignments against the bound fixed clouds, every cue slice with a moving cloud
of its own per alignment, clouds resident in HBM.  Times the serial loop set_moving (per slice) / set_moving_in_fixed / compute()
against ONE srrg2_align_batch_slices call, and checks sampled alignments bit for bit against the loop, in two configurations:
  c3   C3's projective point-to-plane + reprojection slices sharing their clouds, the 640 x 480 measurement fixed and K candidate
       clouds moving (the relocaliser's shape: random 90 % subsets of the moving render);
  nn2  two nearest-neighbour SE(3) slices (C2's point-to-plane slice + a point-to-point slice) with clouds of their own, 50 k
       points each, the same motion seen by both.
Prints one JSON line.
usage: python tools/bench_multi_cue.py [--ks 8,32] [--configs c3,nn2] [--points 50000] [--reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # (before the product library: see tests/conftest.py)

import srrg2_slam_interfaces_amd as pkg
from srrg2_slam_interfaces_amd import _abi as abi, synthetic as syn

ITERATIONS = 10


def setup_c3(K, points):
    """C3's aligner (bench.py) and K candidate clouds: {slice: (coords list, normals list)}, guesses"""
    data = syn.rgbd_pair(seed=3000)
    rng = np.random.default_rng(3001)
    n = data["moving"].shape[0]
    sels = [np.sort(rng.choice(n, int(0.9 * n), replace=False)) for _ in range(K)]
    moving = {0: ([data["moving"][s] for s in sels], [data["moving_normals"][s] for s in sels])}

    def make():
        al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
        al.set_params(max_iterations=ITERATIONS, min_num_inliers=10)
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

    return make, moving, [syn.identity(3)] * K


def setup_nn2(K, points):
    """two nearest-neighbour slices, each with its own fixed scene; candidate k moves both by the same X_gt"""
    b = syn.batch_3d(K=K, n=points, seed=4000, shared_fixed_group=K)
    F1, _ = syn.scene_3d(points, 7000)
    m1 = []
    for k in range(K):
        P, _ = syn.scene_3d(points, 7001 + k)
        Xi = syn.se3_inv(b[k]["X_gt"])
        m1.append(np.ascontiguousarray(P @ Xi[:, :3].T + Xi[:, 3], np.float32))
    moving = {0: ([p["moving"] for p in b], [p["moving_normals"] for p in b]), 1: (m1, None)}
    F1 = np.ascontiguousarray(F1, np.float32)

    def make():
        al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
        al.set_params(max_iterations=ITERATIONS, min_num_inliers=10)
        c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
        c.kind, c.finder, c.finder_max_distance = abi.SLICE_P2PLANE, abi.FINDER_NN_GATED, 0.25
        c.finder_normal_cos, c.robustifier, c.robustifier_chi_threshold = 0.8, abi.ROBUST_CAUCHY, 0.05
        al.add_slice(c)
        c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
        c.kind, c.finder, c.finder_max_distance = abi.SLICE_P2P, abi.FINDER_NN_GATED, 0.25
        al.add_slice(c)
        al.set_fixed(0, b[0]["fixed"], b[0]["fixed_normals"])
        al.set_fixed(1, F1)
        return al

    return make, moving, [syn.identity(3)] * K


def record(al):
    n, last = al.last_iteration_stats()
    return (al.moving_in_fixed().tobytes(), al.status(), n, last, al.num_correspondences(), al.information().tobytes())


def run(name, K, points, reps):
    make, moving, guesses = {"c3": setup_c3, "nn2": setup_nn2}[name](K, points)
    dev = {}
    for si, (cs, ns) in moving.items():
        offs = np.concatenate([[0], np.cumsum([c.shape[0] for c in cs])]).astype(np.int32)
        c = torch.from_numpy(np.ascontiguousarray(np.concatenate(cs, axis=0), np.float32)).cuda()
        n = None if ns is None else torch.from_numpy(np.ascontiguousarray(np.concatenate(ns, axis=0), np.float32)).cuda()
        dev[si] = (c, n, offs)
    torch.cuda.synchronize()
    loop_al, batch_al = make(), make()
    g = np.stack(guesses)

    def loop(keep=None):
        ok = True
        for k in range(K):
            for si, (c, n, offs) in dev.items():
                o0, o1 = int(offs[k]), int(offs[k + 1])
                loop_al.set_cloud_device("set_moving", si, c.data_ptr() + 12 * o0, 12,
                                         0 if n is None else n.data_ptr() + 12 * o0, 12, o1 - o0)
            loop_al.set_moving_in_fixed(guesses[k])
            ok = (loop_al.compute() == abi.SUCCESS) and ok
            if keep is not None and k in keep:
                keep[k] = record(loop_al)
        return ok

    entries = {si: (c.data_ptr(), 12, 0 if n is None else n.data_ptr(), 12, offs) for si, (c, n, offs) in dev.items()}

    def batch():
        return batch_al.compute_batch_slices_device(entries, g)

    picks = {k: None for k in sorted({0, K // 3, K // 2, K - 1})}
    loop(picks)
    res = batch()
    bits_equal = all(
        (res[k]["moving_in_fixed"].tobytes(), res[k]["status"], res[k]["num_iterations"], res[k]["last"],
         res[k]["num_correspondences"], res[k]["information"].tobytes()) == rec for k, rec in picks.items())
    t_loop, t_batch, ok_loop, ok_batch = [], [], True, True
    for _ in range(reps):
        t0 = time.perf_counter()
        ok_loop = loop() and ok_loop
        t_loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = batch()
        t_batch.append(time.perf_counter() - t0)
        ok_batch = ok_batch and bool(np.all(r.status == abi.SUCCESS))
    dl, db = float(np.median(t_loop)), float(np.median(t_batch))
    return {"config": name, "K": K, "moving_points": [int(v[2][-1]) // K for v in dev.values()],
            "loop": {"ms_per_alignment": dl / K * 1e3, "all_success": bool(ok_loop)},
            "batch": {"ms_per_alignment": db / K * 1e3, "all_success": bool(ok_batch)},
            "speedup": dl / db, "bits_equal_sampled": bool(bits_equal), "sampled": sorted(picks)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ks", default="8,32")
    ap.add_argument("--configs", default="c3,nn2")
    ap.add_argument("--points", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = [run(c, int(k), a.points, a.reps) for c in a.configs.split(",") for k in a.ks.split(",")]
    print(json.dumps({"metric": "multi-cue batches (srrg2_align_batch_slices) against the serial set_moving / compute() loop",
                      "iterations": ITERATIONS, "runs": out,
                      "bits_equal": all(r["bits_equal_sampled"] for r in out)}))


if __name__ == "__main__":
    main()
