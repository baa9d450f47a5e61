#!/usr/bin/env python
"""Pair batches (srrg2_align_pairs; SURVEY.md section 8d's all-distinct C4 variant): K alignments of 50 000 points, each against its
OWN fixed cloud (synthetic.batch_3d(..., shared_fixed_group=1)), clouds resident in HBM.  Times the serial loop
set_fixed / set_moving / set_moving_in_fixed / compute() per alignment (bench.py's measure_c4_distinct) against ONE
srrg2_align_pairs call, and checks a few pairs bit for bit against the loop.  Prints one JSON line.
usage: python tools/bench_pairs.py [--ks 8,32,256] [--points 50000] [--reps 5]"""
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


def make_aligner():
    """C2's slice (bench.py's make_aligner)"""
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
    al.set_params(max_iterations=ITERATIONS, min_num_inliers=10)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind = abi.SLICE_P2PLANE
    c.finder = abi.FINDER_NN_GATED
    c.finder_max_distance = 0.25
    c.finder_normal_cos = 0.8
    c.robustifier = abi.ROBUST_CAUCHY
    c.robustifier_chi_threshold = 0.05
    al.add_slice(c)
    return al


def record(al):
    n, last = al.last_iteration_stats()
    return (al.moving_in_fixed().tobytes(), al.status(), n, last, al.num_correspondences(), al.information().tobytes())


def run(K, points, reps):
    probs = syn.batch_3d(K=K, n=points, seed=4000, shared_fixed_group=1)
    ident = syn.identity(3)
    guesses = np.stack([ident] * K)
    cat = {k: torch.from_numpy(np.ascontiguousarray(np.concatenate([p[k] for p in probs], axis=0))).cuda()
           for k in ("fixed", "fixed_normals", "moving", "moving_normals")}
    foff = np.concatenate([[0], np.cumsum([p["fixed"].shape[0] for p in probs])]).astype(np.int32)
    moff = np.concatenate([[0], np.cumsum([p["moving"].shape[0] for p in probs])]).astype(np.int32)
    torch.cuda.synchronize()
    loop_al, pair_al = make_aligner(), make_aligner()

    def loop(keep=None):
        ok = True
        for k in range(K):
            f0, f1, m0, m1 = int(foff[k]), int(foff[k + 1]), int(moff[k]), int(moff[k + 1])
            fc, fn, mc, mn = (cat[key] for key in ("fixed", "fixed_normals", "moving", "moving_normals"))
            loop_al.set_cloud_device("set_fixed", 0, fc[f0].data_ptr(), 12, fn[f0].data_ptr(), 12, f1 - f0)
            loop_al.set_cloud_device("set_moving", 0, mc[m0].data_ptr(), 12, mn[m0].data_ptr(), 12, m1 - m0)
            loop_al.set_moving_in_fixed(ident)
            ok = (loop_al.compute() == abi.SUCCESS) and ok
            if keep is not None and k in keep:
                keep[k] = record(loop_al)
        return ok

    def pairs():
        return pair_al.compute_batch_pairs_device(cat["fixed"].data_ptr(), 12, cat["fixed_normals"].data_ptr(), 12, foff,
                                                  cat["moving"].data_ptr(), 12, cat["moving_normals"].data_ptr(), 12, moff, guesses)

    picks = {k: None for k in sorted({0, K // 3, K // 2, K - 1})}
    loop(picks)
    res = pairs()
    bits_equal = all(
        (res[k]["moving_in_fixed"].tobytes(), res[k]["status"], res[k]["num_iterations"], res[k]["last"],
         res[k]["num_correspondences"], res[k]["information"].tobytes()) == rec for k, rec in picks.items())
    t_loop, t_pairs, ok_loop, ok_pairs = [], [], True, True
    for _ in range(reps):
        t0 = time.perf_counter()
        ok_loop = loop() and ok_loop
        t_loop.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r = pairs()
        t_pairs.append(time.perf_counter() - t0)
        ok_pairs = ok_pairs and bool(np.all(r.status == abi.SUCCESS))
    dl, dp = float(np.median(t_loop)), float(np.median(t_pairs))
    return {"K": K, "points": points,
            "loop": {"it_per_s": ITERATIONS * K / dl, "ms_per_alignment": dl / K * 1e3, "all_success": bool(ok_loop)},
            "pairs": {"it_per_s": ITERATIONS * K / dp, "ms_per_alignment": dp / K * 1e3, "all_success": bool(ok_pairs)},
            "speedup": dl / dp, "bits_equal_sampled": bool(bits_equal), "sampled": sorted(picks)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ks", default="8,32,256")
    ap.add_argument("--points", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    out = [run(int(k), a.points, a.reps) for k in a.ks.split(",")]
    print(json.dumps({"metric": "pair batches (srrg2_align_pairs) against the serial set_fixed / set_moving / compute() loop",
                      "iterations": ITERATIONS, "runs": out,
                      "all_success": all(r["pairs"]["all_success"] for r in out),
                      "bits_equal": all(r["bits_equal_sampled"] for r in out)}))


if __name__ == "__main__":
    main()
