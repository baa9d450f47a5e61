"""C5 (50 000 SE(3) poses / 200 000 factors, Omega = I, 10 Gauss-Newton iterations, PCG tolerance 1e-6) with CAUCHY
(chi threshold 0.01, ~30 x a correct closure's mean chi) on every loop closure, CG capped at 5 000 iterations: the clean
graph, and the graph with 0.5 % of its loop closures corrupted (0.5 m / 0.2 rad).  Prints one JSON line per run: median solve time, CG iterations per
Gauss-Newton iteration, the largest position error against poses_gt; both with the default hierarchy reuse (lag_below 0.05)
and with a fresh hierarchy set-up every iteration (lag_below 0); then the time of evaluate_factors on the 200 000 factors.

    python tools/bench_posegraph_robust.py [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import posegraph as pgm  # noqa: E402
from srrg2_slam_interfaces_amd import synthetic as syn  # noqa: E402

THR = 0.01
PCG_MAX = 5000  # (the first robust iteration needs more than the default 600 CG iterations)


def corrupted_c5(fraction=0.005, seed=7):
    V = 50_000
    g = syn.pose_graph_3d(V=V, E=200_000, seed=5000)
    Et = g["ij"].shape[0]
    loop = np.arange(V - 1, Et)
    rng = np.random.default_rng(seed)
    bad = np.sort(rng.choice(loop, size=int(round(fraction * loop.size)), replace=False))
    Z = g["Z"].copy()
    for e in bad:
        off = syn.se3(rng.normal(size=3) * 0.5, rng.normal(size=3) * 0.2)
        Z[e] = (off @ np.vstack([Z[e], [0, 0, 0, 1]]))[:3].astype(np.float32)
    return g, Z, loop, bad


def max_err(P, gt):
    return float(np.max(np.linalg.norm(P[:, :, 3] - gt[:, :, 3], axis=1)))


def run(name, g, Z, kinds, lag, steps, warmup):
    pg = pkg.PoseGraph(abi.SE3_QUAT_RIGHT)
    pg.set_tuning(lag_below=lag)
    times, st = [], None
    for _ in range(warmup + steps):
        pg.set_graph(g["poses_init"], g["ij"], Z)
        if kinds is not None:
            pg.set_robustifiers(kinds, np.full(kinds.size, THR, np.float32))
        params = pgm.default_params()
        params.pcg_max_iterations = PCG_MAX
        t0 = time.perf_counter()
        st = pg.solve(params)
        times.append(time.perf_counter() - t0)
    line = {"run": name, "lag_below": lag, "solve_ms_median": round(1e3 * float(np.median(times[warmup:])), 2),
            "cg_per_gn": [s["pcg_iterations"] for s in st], "max_residual": max(s["pcg_residual"] for s in st),
            "status": [s["solver_status"] for s in st], "max_error_m": round(max_err(pg.poses(), g["poses_gt"]), 4)}
    print(json.dumps(line), flush=True)
    return pg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    g, Z, loop, bad = corrupted_c5()
    kinds = np.zeros(g["ij"].shape[0], np.int32)
    kinds[loop] = abi.ROBUST_CAUCHY
    run("clean, no robustifier", g, g["Z"], None, 0.05, a.steps, a.warmup)
    run("corrupted, no robustifier", g, Z, None, 0.05, a.steps, a.warmup)
    for lag in (0.05, 0.0):
        run("clean, cauchy on loop closures", g, g["Z"], kinds, lag, a.steps, a.warmup)
        pg = run("corrupted, cauchy on loop closures", g, Z, kinds, lag, a.steps, a.warmup)
    ts = []
    for _ in range(a.warmup + max(a.steps, 5)):
        t0 = time.perf_counter()
        chi, w = pg.evaluate_factors()
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"run": "evaluate_factors", "factors": int(chi.size), "ms_median": round(1e3 * float(np.median(ts[a.warmup:])), 3),
                      "corrupted_with_w_below_0.5": int((w[bad] < 0.5).sum()), "corrupted": int(bad.size),
                      "correct_with_w_below_0.5": int((w < 0.5).sum() - (w[bad] < 0.5).sum())}), flush=True)


if __name__ == "__main__":
    main()
