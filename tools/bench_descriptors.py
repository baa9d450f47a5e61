#!/usr/bin/env python
"""Descriptor matching of the HBST loop detector on the device database ("Descriptor matching"):
one JSON line with the database and query sizes, the median match() time (HIP events: upload + search + compaction;
wall clock: the whole call with the readback), pairs/s and the share of the VALU bound, the numpy restatement on a
sample of maps scaled to the whole database (numpy, not HBST), and one MultiLoopDetectorHBST.compute() end to end.
--from-scene adds the same query matched from a Scene that carries the descriptors (match_scene: staged on the device).
  usage: python tools/bench_descriptors.py [--maps 1000] [--per-map 1000] [--query 2000] [--reps 20] [--sample 16] [--from-scene]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:
    import torch  # noqa: F401  (before the library: one HIP runtime for both, tests/conftest.py)
except Exception:
    pass

import hbst_restatement as hr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import loop_detector as ld  # noqa: E402

# VALU bound: 256 CUs x 4 SIMDs x 32 lanes per cycle (a wave64 VALU instruction issues over 2 cycles) x 2.4 GHz, and
# the inner loop's 20 VALU instructions per pair (8 v_xor_b32 + 8 v_bcnt_u32_b32 + compare + carry-add + v_lshl_or_b32 +
# v_min_u32; the loop's ds_read_b128 and scalar bookkeeping are shared by four pairs)
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_PAIR = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=1000)
    ap.add_argument("--per-map", type=int, default=1000)
    ap.add_argument("--query", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--from-scene", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    maps = [hr.random_descriptors(rng, a.per_map) for _ in range(a.maps)]
    q = hr.random_descriptors(rng, a.query)
    closures = [a.maps // 4, a.maps // 2]  # near-duplicates of two maps: two candidates
    slot = 0
    for r in closures:
        for j in rng.choice(a.per_map, min(a.per_map, a.query // 4), replace=False):
            q[slot] = hr.flip_bits(rng, maps[r][j], int(rng.integers(0, 9)))
            slot += 1
    db = pkg.DescriptorDatabase()
    for m in maps:
        db.add(m)
    nmaps, ndesc = db.size()
    min_matches = min(500, a.query // 8)
    db.match(q, min_matches=min_matches)  # warm-up
    dev, wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = db.match(q, min_matches=min_matches)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(res.device_ms)
    dev_ms, wall_ms = float(np.median(dev)), float(np.median(wall))
    scene_ms = None
    if a.from_scene:
        from srrg2_slam_interfaces_amd import mapping

        qs = mapping.Scene(pkg.scene_binding(0), 3)
        qs.set(rng.uniform(-5, 5, (a.query, 3)).astype(np.float32))
        qs.set_features(q)
        ref = db.match_scene(qs, min_matches=min_matches)  # warm-up
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ref.correspondences, res.correspondences))
        sdev, swall = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = db.match_scene(qs, min_matches=min_matches)
            swall.append((time.perf_counter() - t0) * 1e3)
            sdev.append(r.device_ms)
        scene_ms = {"match_scene_ms_events": round(float(np.median(sdev)), 4), "match_scene_ms_wall": round(float(np.median(swall)), 4)}
    pairs = float(ndesc) * a.query
    bound_ms = pairs * OPS_PER_PAIR / VALU_LANE_OPS * 1e3

    sample = sorted(set(rng.choice(a.maps, min(a.sample, a.maps), replace=False).tolist()))
    ref = hr.RestatedDatabase()
    for m in maps:
        ref.maps.append((m, np.arange(len(m), dtype=np.int32)))
    t0 = time.perf_counter()
    ref.match(q, query_index=nmaps, min_matches=min_matches, only_maps=sample)
    numpy_ms = (time.perf_counter() - t0) * 1e3 * a.maps / len(sample)

    # one compute() end to end: the same database behind a detector, the query's points a rigid copy of the two
    # closures' reference points (K candidates, one batched locked solve)
    pts = [rng.uniform(-5, 5, (a.per_map, 3)).astype(np.float32) for _ in range(a.maps)]
    qpts = rng.uniform(-5, 5, (a.query, 3)).astype(np.float32)
    res = db.match(q, min_matches=min_matches)
    for r, c in zip(res.indices, res.correspondences):
        qpts[c["fixed_idx"]] = pts[r][c["moving_idx"]] + np.float32(0.1)
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind, c.finder, c.robustifier, c.robustifier_chi_threshold = (abi.SLICE_P2P, abi.FINDER_CORRESPONDENCES,
                                                                    abi.ROBUST_CAUCHY, 0.05)
    al.add_slice(c)
    det = ld.MultiLoopDetectorHBST(al, relocalize_min_inliers=min_matches, database=db)
    det._local_maps_in_database = [(r, pts[r], None) for r in range(a.maps)]
    det.compute(-1, qpts, None, q)  # warm-up
    t0 = time.perf_counter()
    closures_found = det.compute(-1, qpts, None, q)
    compute_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({
        "metric": "descriptor_match", "maps": nmaps, "descriptors": ndesc, "query": a.query,
        "match_ms_events": round(dev_ms, 4), "match_ms_wall": round(wall_ms, 4),
        "pairs_per_s": pairs / (dev_ms * 1e-3), "valu_bound_ms": round(bound_ms, 4),
        "fraction_of_valu_bound": round(bound_ms / dev_ms, 3),
        "numpy_restatement_ms_scaled": round(numpy_ms, 1), "numpy_sample_maps": len(sample),
        "compute_ms": round(compute_ms, 3), "compute_candidates": len(det.indices()),
        "compute_closures": len(closures_found), **(scene_ms or {})}))


if __name__ == "__main__":
    main()
