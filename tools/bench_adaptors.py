#!/usr/bin/env python
"""Cost of the adapt step (srrg2_adapt_*) against what it replaces: the finished cloud handed to Scene.set from the host.
One JSON line, milliseconds per call, medians over --reps alternating repetitions after a warm-up.  The clock is the host's
around blocking C-ABI calls (the library's stream is its own: a caller cannot put events on it), so every figure contains
the launch and the wait, as a tracker pays them.  "numpy_restatement_ms" is the time of the untuned numpy restatement on one
host thread: it is NOT a baseline (nobody would ship it), it only says what a caller without the adaptor has to do somewhere."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

try:
    import torch  # noqa: E402,F401  (before the library: tests/conftest.py says why)
except Exception:
    torch = None

import adaptor_restatement as ar  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi  # noqa: E402
from srrg2_slam_interfaces_amd import adaptors, mapping  # noqa: E402
from srrg2_slam_interfaces_amd import synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    d = syn.rgbd_pair()
    z = np.ascontiguousarray(d["fixed"][:, 2].reshape(d["rows"], d["cols"]), np.float32)
    mm = np.where(np.isfinite(z), np.rint(z.astype(np.float64) * 1000.0), 0).astype(np.uint16)
    pts, _ = syn.scan_2d(syn.se2(0, 0, 0), beams=1000)
    ranges = np.linalg.norm(pts, axis=1).astype(np.float32)
    ang = np.deg2rad(np.linspace(-135.0, 135.0, 1000))

    def depth_adaptor(scene, compact, raw):
        p = adaptors.default_depth_params()
        for i, v in enumerate(np.asarray(d["K"], np.float32).reshape(9)):
            p.camera_matrix[i] = float(v)
        p.depth_min, p.depth_max, p.compact = d["depth_min"], d["depth_max"], int(compact)
        p.rows, p.cols = mm.shape
        a = adaptors.MeasurementAdaptorDepthImage(p)
        a.set_meas(scene)
        a.set_raw_data(raw, depth_type=abi.IMAGE_U16)
        return a

    s_host, s_dev, s_cmp, s_scan, s_set, s_set2 = (mapping.Scene(b, k) for k in (3, 3, 3, 2, 3, 2))
    cases = {}
    cases["adapt_depth_u16_host_ms"] = depth_adaptor(s_host, False, mm).compute
    a_queue = depth_adaptor(s_host, False, mm)
    cases["adapt_depth_u16_host_queued_ms"] = lambda: a_queue.compute(False)  # (returns when queued; the next call waits)
    keep = None
    if torch is not None and torch.cuda.is_available():
        keep = torch.from_numpy(mm).cuda()
        torch.cuda.synchronize()
        cases["adapt_depth_u16_device_ms"] = depth_adaptor(s_dev, False, (keep.data_ptr(), mm.strides[0])).compute
    # compact: ~100 k points (every third row of the image)
    third = np.ascontiguousarray(mm[::3])
    a_cmp = depth_adaptor(s_cmp, True, third)
    cases["adapt_depth_u16_host_compact_ms"] = a_cmp.compute
    sp = adaptors.default_scan_params()
    sp.angle_min, sp.angle_increment = float(ang[0]), float(ang[1] - ang[0])
    a_scan = adaptors.MeasurementAdaptorLaserScan(sp)
    a_scan.set_meas(s_scan)
    a_scan.set_raw_data(ranges)
    cases["adapt_scan_1000_host_ms"] = a_scan.compute
    # what the parent offers for the same scenes: the finished arrays uploaded by Scene.set (upload + ingest only)
    t0 = time.perf_counter()
    r = ar.adapt_depth_image(mm, d["K"], depth_min=d["depth_min"], depth_max=d["depth_max"])
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    rs = ar.adapt_laser_scan(ranges, float(ang[0]), float(ang[1] - ang[0]))
    cases["scene_set_depth_cloud_ms"] = lambda: s_set.set(r["points"], r["normals"])
    cases["scene_set_scan_cloud_ms"] = lambda: s_set2.set(rs["points"], rs["normals"])
    times = {k: [] for k in cases}
    for rep in range(args.warmup + args.reps):
        for name, fn in cases.items():  # alternating
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= args.warmup:
                times[name].append(1e3 * dt)
    out = {k: float(np.median(v)) for k, v in times.items()}
    out.update(reps=args.reps, clock="host wall clock around blocking calls", numpy_restatement_ms_not_a_baseline=numpy_ms,
               depth_points=int(s_host.size()), compact_points=int(s_cmp.size()), scan_points=int(s_scan.size()),
               bytes_in_depth=int(mm.nbytes), bytes_out_depth=int(2 * 16 * mm.size))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
