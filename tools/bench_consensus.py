#!/usr/bin/env python3
"""Side bench of the consensus pose: srrg2_consensus_compute on seeded candidates (tests/consensus_cases.py: planted poses met
from the opposite direction, 2 mm noise), K = 1 / 8 / 32 candidates x N = 500 / 2 000 matches x H = 256 / 1 024 hypotheses, at 30 %
and 60 % wrong matches.  Per setting:
  host_ms, device_ms   median HOST WALL CLOCK of the blocking call with results, offsets and inlier records, clouds in host memory
                       (they ride in the call's one upload) and in device memory; *_minmax is [min, max] over the calls
  scored, pairs        scored hypotheses and evaluated (hypothesis, pair) products, summed over the candidates
  found                candidates with status FOUND
  restatement_ms       tests/consensus_restatement.py (numpy, one thread) on the same inputs, once; its results must agree
  solve_raw_ms         compute_batch_correspondences on the same candidates as the detector runs it today: every match, from the
                       identity; solve_raw_ok = alignments with status SUCCESS
  solve_verified_ms    the same call behind the verification: the consensus poses as guesses, the inlier lists as matches (FOUND
                       candidates only); solve_verified_ok likewise.  host_ms + solve_verified_ms against solve_raw_ms is what a
                       caller pays for, or saves with, the verification
One JSON line on stdout, also written to profiles/consensus_bench.json.

    python tools/bench_consensus.py [--calls 30] [--solve-calls 5] [--tag NAME] [--no-restatement]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (before the library: tests/conftest.py says why)

import consensus_cases as cc  # noqa: E402
import consensus_restatement as cr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import synthetic as syn  # noqa: E402


def timed_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(t):
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def device_copy(lib, a):
    lib.srrg2_amd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.srrg2_amd_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    lib.srrg2_amd_device_free.argtypes = [C.c_void_p]
    p = C.c_void_p()
    if lib.srrg2_amd_device_malloc(C.c_size_t(max(a.nbytes, 16)), C.byref(p)) or \
            lib.srrg2_amd_memcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1, None):
        raise RuntimeError("device copy failed")
    return p


def aligner():
    al = pkg.MultiAligner(abi.SE3_QUAT_RIGHT)
    al.set_params(max_iterations=15)
    c = abi.default_slice_config(abi.SE3_QUAT_RIGHT)
    c.kind, c.finder = abi.SLICE_P2P, abi.FINDER_CORRESPONDENCES
    c.robustifier, c.robustifier_chi_threshold = abi.ROBUST_CAUCHY, 0.05
    al.add_slice(c)
    return al


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--solve-calls", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    v = pkg.ConsensusVerifier(3)
    lib = v._lib
    al = aligner()
    rows = []
    for wrong in (0.3, 0.6):
        for N in (500, 2000):
            # one query cloud; every candidate sees it from a pose of its own (all of them from the opposite direction)
            cands = [cc.planted(1000 + k, 3, N, wrong, yaw_deg=180.0) for k in range(32)]
            for K in (1, 8, 32):
                fixed = np.ascontiguousarray(cands[0][0])
                # (planted() draws the landmarks from its seed: give every candidate the first one's, moved by its own pose)
                movings, corrs = [], []
                for k in range(K):
                    X = cands[k][3]
                    Xi = syn.se3_inv(X)
                    rng = np.random.default_rng(7000 + k)
                    m = fixed.astype(np.float64) @ Xi[:, :3].T + Xi[:, 3] + rng.normal(scale=0.002, size=fixed.shape)
                    movings.append(m.astype(np.float32))
                    corrs.append(cands[k][2])
                moving = np.ascontiguousarray(np.concatenate(movings))
                moff = np.arange(K + 1, dtype=np.int32) * N
                coff = np.arange(K + 1, dtype=np.int32) * N
                recs = np.concatenate(corrs)
                df, dm = device_copy(lib, fixed), device_copy(lib, moving)
                for H in (256, 1024):
                    p = v.params(num_hypotheses=H, seed=1)
                    host = lambda: v.compute_raw(fixed.ctypes.data, 12, N, moving.ctypes.data, 12, moff, abi.MEM_HOST, recs, coff, p)  # noqa: E731
                    dev = lambda: v.compute_raw(df.value, 12, N, dm.value, 12, moff, abi.MEM_DEVICE, recs, coff, p)  # noqa: E731
                    host(), dev()
                    th = [timed_ms(host)[0] for _ in range(a.calls)]
                    td = [timed_ms(dev)[0] for _ in range(a.calls)]
                    res = v._unpack(*host())
                    row = dict(K=K, N=N, H=H, wrong=wrong)
                    row["host_ms"], row["host_minmax"] = summary(th)
                    row["device_ms"], row["device_minmax"] = summary(td)
                    row["scored"] = int(sum(r["num_scored"] for r in res))
                    row["pairs"] = int(sum(r["num_scored"] * r["num_pairs"] for r in res))
                    row["found"] = int(sum(r["status"] == abi.CONSENSUS_FOUND for r in res))
                    if not a.no_restatement:
                        ms, want = timed_ms(lambda: cr.consensus(3, fixed, movings, corrs, num_hypotheses=H, seed=1))
                        row["restatement_ms"] = round(ms, 2)
                        row["restatement_agrees"] = all(
                            w["num_inliers"] == r["num_inliers"] and w["best_hypothesis"] == r["best_hypothesis"]
                            and w["moving_in_fixed"].tobytes() == r["moving_in_fixed"].tobytes()
                            and w["inliers"].tobytes() == r["inliers"].tobytes() for w, r in zip(want, res))
                    al.set_fixed(0, fixed, None)
                    ident = [syn.identity(3)] * K
                    raw = lambda: al.compute_batch_correspondences(movings, corrs, ident, None)  # noqa: E731
                    raw()
                    t, out = zip(*[timed_ms(raw) for _ in range(a.solve_calls)])
                    row["solve_raw_ms"], row["solve_raw_minmax"] = summary(t)
                    row["solve_raw_ok"] = int(sum(r["status"] == abi.SUCCESS for r in out[-1]))
                    keep = [k for k in range(K) if res[k]["status"] == abi.CONSENSUS_FOUND]
                    if keep:
                        ver = lambda: al.compute_batch_correspondences([movings[k] for k in keep], [res[k]["inliers"] for k in keep],  # noqa: E731
                                                                       [res[k]["moving_in_fixed"] for k in keep], None)
                        ver()
                        t, out = zip(*[timed_ms(ver) for _ in range(a.solve_calls)])
                        row["solve_verified_ms"], row["solve_verified_minmax"] = summary(t)
                        row["solve_verified_ok"] = int(sum(r["status"] == abi.SUCCESS for r in out[-1]))
                    rows.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                lib.srrg2_amd_device_free(df)
                lib.srrg2_amd_device_free(dm)
    out = dict(bench="consensus", tag=a.tag, calls=a.calls, solve_calls=a.solve_calls, date=time.strftime("%Y-%m-%d"),
               command="python tools/bench_consensus.py --calls %d --solve-calls %d" % (a.calls, a.solve_calls), rows=rows)
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "consensus_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
