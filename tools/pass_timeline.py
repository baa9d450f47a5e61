#!/usr/bin/env python
"""Where the time of a fused pass launch of ONE alignment goes (C2), from a -DSRRG2_PASS_TIMELINE build:
  make -C srrg2_slam_interfaces_amd/csrc OUT=../lib/libsrrg2_slam_amd_timeline.so EXTRA=-DSRRG2_PASS_TIMELINE
  SRRG2_AMD_LIB=srrg2_slam_interfaces_amd/lib/libsrrg2_slam_amd_timeline.so python tools/pass_timeline.py [n]
Per launch epoch: first / last workgroup start, control step done, record seen (first / last workgroup), first / last end,
in microseconds after the end of the previous launch (100 MHz constant-rate clock: 10 ns steps), and how many workgroups
started only after the first one had ended: the launch's second round, workgroups that were not resident at its start.
Converged passes: the censuses of the failed certificates, of the staged neighbours and of the staged winners (kept / changed
neighbours, near-tie-only staging, points decided by their owner alone), when the workgroups with a changed neighbour or an
owner's decision end, and what the workgroups are that end more than 1 us after the median one."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import srrg2_slam_interfaces_amd as pkg
from srrg2_slam_interfaces_amd import _abi as abi, _capi, synthetic as syn

scan2d = "--scan2d" in sys.argv  # a 2-D scan pair, SE(2) point-to-point, a NEW fixed scan before every compute() (no lists)
args = [x for x in sys.argv[1:] if not x.startswith("--")]
n = int(args[0]) if args else (3000 if scan2d else 100000)
lib = _capi.lib()
kind = abi.SE2_RIGHT if scan2d else abi.SE3_QUAT_RIGHT
al = pkg.MultiAligner(kind)
al.set_params(max_iterations=10, min_num_inliers=10)
c = abi.default_slice_config(kind)
if scan2d:
    c.kind, c.finder, c.finder_max_distance = abi.SLICE_P2P, abi.FINDER_NN_GATED, 0.5
    pr = syn.scan_pair_2d(beams=n, sigma=0.01, seed=1234)
else:
    c.kind, c.finder, c.finder_max_distance, c.finder_normal_cos = abi.SLICE_P2PLANE, abi.FINDER_NN_GATED, 0.25, 0.8
    pr = syn.batch_3d(K=1, n=n, seed=2000, shared_fixed_group=1)[0]
c.robustifier, c.robustifier_chi_threshold = abi.ROBUST_CAUCHY, 0.05
al.add_slice(c)
al.set_fixed(0, pr["fixed"], pr.get("fixed_normals"))
al.set_moving(0, pr["moving"], pr.get("moving_normals"))
WGS = 2048  # (PASS_TS_WGS of kernels.hip: every workgroup of the launch; the last slot holds the census)
buf = (C.c_uint64 * (16 * WGS * 8))()
for rep in range(4):  # (the second compute() builds the lists; the later ones run on them)
    if scan2d:
        al.set_fixed(0, pr["fixed"], pr.get("fixed_normals"))
    al.set_moving_in_fixed(syn.identity(2 if scan2d else 3))
    lib.srrg2_amd_debug_pass_timeline(buf, 1)
    al.compute()
lib.srrg2_amd_debug_pass_timeline(buf, 0)
ts = np.frombuffer(buf, dtype=np.uint64).reshape(16, WGS, 8).astype(np.int64)
prev_end = None
print("epoch | workgroups | start: first  last | control done | record seen: first  median  last | end: first  median  last | launch   [us after the end of the previous launch]")
for e in range(16):
    used = ts[e, :, 0] > 0
    used[WGS - 3:] = False  # (the last three slots hold the censuses)
    census = ts[e, WGS - 1, :7].copy()
    staged = ts[e, WGS - 2, :6].copy()
    winners = ts[e, WGS - 3, :5].copy()
    if not used.any():
        continue
    st, ctl, seen, end = ts[e, used, 0], ts[e, 0, 1], ts[e, used, 2], ts[e, used, 3]
    seen, end = seen[seen > 0], end[end > 0]
    if not len(end):
        continue
    if not len(seen):  # (a first pass with the prologue inside derives its record from the kernel arguments: no such stamp)
        seen = st
    t0 = prev_end if prev_end is not None else st.min()
    f = lambda x: "%6.2f" % ((x - t0) / 100.0)
    print("%5d | %10d | %s  %s | %s | %s  %s  %s | %s  %s  %s | %6.2f" % (
        e, used.sum(), f(st.min()), f(st.max()), f(ctl) if ctl else "     -", f(seen.min()), f(np.median(seen)), f(seen.max()),
        f(end.min()), f(np.median(end)), f(end.max()), (end.max() - st.min()) / 100.0))
    ended = ts[e, used, 3]
    late = int((st > ended[ended > 0].min()).sum())
    print("      %d of %d workgroups started after the first one had ended%s" % (late, used.sum(), " (a second round)" if late else ""))
    if ts[e, 0, 5] and ctl:
        print("      control step: sums and H / b in the lanes at %s, dx solved at %s, X and the transforms at %s, published at %s" % (f(ts[e, 0, 5]), f(ts[e, 0, 6]), f(ts[e, 0, 7]), f(ctl)))
    if census[0]:
        print("      failed certificates: %d points (no previous neighbour %d; margin < 1e-4 cells %d, < 0.0202 cells %d, larger %d; moved > 1e-3 cells %d; no radius %d)" % tuple(census))
    if staged.any():
        print("      staged neighbours: %d thin lanes staged, %d decided, rejected %d (more than the cap) + %d (not covered), "
              "%d certificates failed unstaged, %d waves with more than four thin lanes" % tuple(staged))
    if winners.any():
        print("      staged winners: %d kept their neighbour, %d changed it and were served from the staged set, %d changed it and fetched; "
              "%d lanes staged under the near-tie-only rule; %d decided by their owner alone" % tuple(winners))
    rest = used.copy()
    rest[0] = False  # (workgroup 0 keeps the control step's stamps in these slots)
    # behind the reduction a wave that changed a neighbour (and fetched it) stamps slot 6, one with a point its owner decided alone slot 7
    wend = ts[e, :, 3]
    for slot, what in ((6, "a changed neighbour"), (7, "a point decided by its owner alone")):
        ch = rest & (ts[e, :, slot] > 0) & (wend > 0)
        if ch.any():
            print("      workgroups with %s: %d, end first / median / last %s / %s / %s" % (
                what, ch.sum(), f(wend[ch].min()), f(np.median(wend[ch])), f(wend[ch].max())))
    tail = rest & (wend > np.median(end) + 100)  # (more than 1 us behind the median workgroup)
    if tail.any():
        print("      workgroups that end more than 1 us after the median: %d (first at %s), of them %d fetched a changed neighbour, "
              "%d had a point decided by its owner alone, %d staged" % (tail.sum(), f(wend[tail].min()), (tail & (ts[e, :, 6] > 0)).sum(),
                                                                        (tail & (ts[e, :, 7] > 0)).sum(), (tail & (ts[e, :, 5] > 0)).sum()))
    sdone = ts[e, rest, 5]
    sdone = sdone[sdone > 0]
    if len(sdone):
        print("      staging done in %d workgroups: first %s, median %s, last %s (record seen: median %s)" % (
            len(sdone), f(sdone.min()), f(np.median(sdone)), f(sdone.max()), f(np.median(seen))))
    p2 = ts[e, used, 4]
    p2 = p2[p2 > 0]
    if len(p2) and staged.any():  # (a kernel that stages has no second phase: its waves with failed certificates stamp their searches' end)
        print("      failed certificates settled (staged decisions and searches) in %d workgroups: first %s, median %s, last %s" % (
            len(p2), f(p2.min()), f(np.median(p2)), f(p2.max())))
        prev_end = end.max()
    elif len(p2):
        print("      second phase (failed certificates) in %d workgroups, last one done at %s" % (len(p2), f(p2.max())))
        prev_end = max(end.max(), p2.max())
    else:
        prev_end = end.max()
