#!/usr/bin/env python3
"""Side bench of srrg2_scene_voxelize: the C2 cloud (100 k points) and a 271 k-point cloud of synthetic.scene_3d, at leaves that
keep about 1/2, 1/8 and 1/30 of the points, in both modes.  Per cloud it reports
  set_ms / set_fixed_ms   Scene.set of the cloud and the aligner's set_fixed of it: what a caller already pays per cloud
  full                    estimate_normals (radius: ~10 neighbours on the full cloud) + set_fixed from the scene's device arrays
                          on the FULL cloud
  per leaf and mode       voxelize_ms: median HOST WALL CLOCK of a blocking call with a result on reused handles (it ends with the
                          call's one host wait: device time plus one round trip -- not HIP-event time: the scene's stream is
                          private to the library), the counts, and what follows on the DECIMATED cloud: estimate_normals at the
                          radius of the full cloud and at 3 leaves (whichever is larger) + set_fixed from its device arrays
  cpu_ms                  per leaf: np.unique on the cell triples + np.add.at, one thread, on this host -- a restatement of the
                          centroid mode, not a tuned CPU voxel filter
One JSON line on stdout.

    python tools/bench_voxelize.py [--calls 20] [--sizes 100000,271000] [--no-cpu] [--tag NAME]
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
from tools.bench_normals import median_ms, radius_for  # noqa: E402

F = np.float32
KEEP = (2, 8, 30)


def occupied(pts, leaf):
    c = np.floor(pts.astype(np.float64) / np.float64(F(leaf))).astype(np.int64)
    c -= c.min(0)
    m = c.max(0) + 1
    return len(np.unique((c[:, 0] * m[1] + c[:, 1]) * m[2] + c[:, 2]))


def leaf_for(pts, keep):
    """the leaf at which about 1 / keep of the points survive (bisection on the number of occupied cells)"""
    lo, hi = 1e-4, 10.0
    for _ in range(18):
        mid = float(np.sqrt(lo * hi))
        if occupied(pts, mid) * keep > len(pts):
            lo = mid
        else:
            hi = mid
    return float(F(np.sqrt(lo * hi)))


def cpu_voxelize(pts, leaf):
    t0 = time.perf_counter()
    P = pts.astype(np.float64)
    uc, inv, cnt = np.unique(np.floor(P / np.float64(F(leaf))), axis=0, return_inverse=True, return_counts=True)
    s = np.zeros((len(uc), 3))
    np.add.at(s, inv.reshape(-1), P)
    (s / cnt[:, None]).astype(F)
    return {"what": "numpy: np.unique on the cell triples + np.add.at, one thread (a restatement, not a tuned CPU voxel filter)",
            "ms": round((time.perf_counter() - t0) * 1e3, 1)}


def follow_up(scene, al, si, radius, calls):
    """estimate_normals(drop = 0, with a result) on the scene, then set_fixed from its device arrays: (normals_ms, set_fixed_ms)"""
    nm = median_ms(lambda: scene.estimate_normals(radius, drop=False), calls)

    def fixed():
        cp, cn, n = scene.device_arrays()
        al.set_cloud_device("set_fixed", si, cp, 16, cn, 16, n)

    return round(nm, 4), round(median_ms(fixed, calls), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="100000,271000")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "voxelize", "tag": args.tag, "calls": args.calls, "clouds": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        pts = (syn.cloud_pair_3d(n=n, seed=2000)["fixed"] if n == 100_000 else syn.scene_3d(n, 2100)[0]).astype(F)
        nrm = np.tile(np.array([0, 0, 1], F), (len(pts), 1))
        scene, dec = mapping.Scene(b, 3), mapping.Scene(b, 3)
        al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
        c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
        c.kind, c.finder_max_distance = abi.SLICE_P2PLANE, 0.25
        si = al.add_slice(c)
        row = {"points": int(len(pts)), "set_ms": round(median_ms(lambda: scene.set(pts), args.calls), 4),
               "set_fixed_ms": round(median_ms(lambda: al.set_fixed(si, pts, nrm), args.calls), 4), "leaves": []}
        radius10 = radius_for(pts, 10)
        fn, ff = follow_up(scene, al, si, radius10, args.calls)
        row["full"] = {"radius": round(radius10, 5), "normals_ms": fn, "set_fixed_device_ms": ff, "sum_ms": round(fn + ff, 4)}
        for keep in KEEP:
            leaf = leaf_for(pts, keep)
            entry = {"keep_about": "1/%d" % keep, "leaf": round(leaf, 5), "modes": {}}
            for mode in ("centroid", "first"):
                scene.set(pts, nrm)  # (with normals: the centroid mode averages them too)
                res = {}

                def call():
                    res.update(scene.voxelize(dec, leaf, mode=mode))

                ms = median_ms(call, args.calls)
                radius = max(radius10, 3.0 * leaf)
                dn, df = follow_up(dec, al, si, radius, args.calls)
                entry["modes"][mode] = {"voxelize_ms": round(ms, 4), "result": dict(res), "then_radius": round(radius, 5),
                                        "then_normals_ms": dn, "then_set_fixed_device_ms": df,
                                        "voxelize_plus_then_ms": round(ms + dn + df, 4), "vs_full": round((ms + dn + df) / row["full"]["sum_ms"], 2)}
            if not args.no_cpu:
                entry["cpu"] = cpu_voxelize(pts, leaf)
            row["leaves"].append(entry)
        out["clouds"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
