#!/usr/bin/env python3
"""Side bench of srrg2_scene_estimate_normals: the C2 cloud (100 k points) and a 271 k-point cloud of synthetic.scene_3d, at radii
that give roughly 10, 30 and 100 neighbours.  Per cloud it reports
  set_ms / set_fixed_ms   Scene.set of the cloud and the aligner's set_fixed of it: what a caller already pays per cloud
  normals_ms              per radius: median HOST WALL CLOCK of a blocking call with a result on a reused handle (it ends with
                          the call's one host wait: device time plus one round trip -- not HIP-event time: the scene's stream
                          is private to the library and it records no events of its own), the radius, and the counts
  cpu_ms                  scipy cKDTree.query_ball_point + numpy.linalg.eigh on this host, once per radius -- or, without scipy,
                          the numpy restatement on 10 k points, labelled as such
One JSON line on stdout.

    python tools/bench_normals.py [--calls 20] [--sizes 100000,271000] [--no-cpu] [--tag NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: F401,E402  (before the library: tests/conftest.py says why)

import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, mapping, synthetic as syn  # noqa: E402

F = np.float32
TARGETS = (10, 30, 100)


def median_ms(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def radius_for(pts, k, sample=2000, seed=1):
    """the radius at which a point of the cloud has k neighbours in the median (brute force on a sample of queries)"""
    rng = np.random.default_rng(seed)
    q = pts[rng.choice(len(pts), min(sample, len(pts)), replace=False)].astype(np.float64)
    P = pts.astype(np.float64)
    kth = [np.partition(((P - x) ** 2).sum(1), k - 1)[k - 1] for x in q[:300]]
    return float(np.sqrt(np.median(kth)))


def cpu_normals(pts, radius):
    try:
        from scipy.spatial import cKDTree
    except Exception:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import normals_restatement as nr

        sub = pts[:10_000]
        t0 = time.perf_counter()
        nr.estimate_normals(sub, radius, drop=False)
        return {"what": "numpy restatement on 10 k points (no scipy)", "ms": round((time.perf_counter() - t0) * 1e3, 1)}
    t0 = time.perf_counter()
    P = pts.astype(np.float64)
    nb = cKDTree(P).query_ball_point(P, radius)
    cov = np.zeros((len(P), 3, 3))
    for i, idx in enumerate(nb):
        if len(idx) >= 5:
            d = P[idx] - P[i]
            cov[i] = d.T @ d / len(idx) - np.outer(d.mean(0), d.mean(0))
    np.linalg.eigh(cov)
    return {"what": "scipy cKDTree.query_ball_point + numpy.linalg.eigh, one thread", "ms": round((time.perf_counter() - t0) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="100000,271000")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "normals", "tag": args.tag, "calls": args.calls, "clouds": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        pts = (syn.cloud_pair_3d(n=n, seed=2000)["fixed"] if n == 100_000 else syn.scene_3d(n, 2100)[0]).astype(F)
        nrm = np.tile(np.array([0, 0, 1], F), (len(pts), 1))
        scene = mapping.Scene(b, 3)
        al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
        c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
        c.kind, c.finder_max_distance = abi.SLICE_P2PLANE, 0.25
        si = al.add_slice(c)
        row = {"points": int(len(pts)), "set_ms": round(median_ms(lambda: scene.set(pts), args.calls), 4),
               "set_fixed_ms": round(median_ms(lambda: al.set_fixed(si, pts, nrm), args.calls), 4), "radii": []}
        for k in TARGETS:
            radius = radius_for(pts, k)
            res = {}

            def call():
                res.update(scene.estimate_normals(radius, drop=False))

            ms = median_ms(call, args.calls)
            entry = {"target_neighbours": k, "radius": round(radius, 5), "normals_ms": round(ms, 4), "result": dict(res),
                     "vs_set_fixed": round(ms / row["set_fixed_ms"], 2)}
            if not args.no_cpu:
                entry["cpu"] = cpu_normals(pts, radius)
            row["radii"].append(entry)
        out["clouds"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
