#!/usr/bin/env python3
"""Side bench of the dense stereo adaptor: srrg2_adapt_stereo_dense on seeded synthetic pairs (a features_cases image and its copy
shifted by a disparity that is constant per band of 40 rows, tests/stereo_cases.py) of 640 x 480 and 1280 x 720, with 64 and 128
disparities, paths 0 and 4, from host and from device memory, organised mode.  Per pair and setting it reports
  dense_ms           the call: median HOST WALL CLOCK of a blocking call with its result on a reused handle (device time plus the
                     call's one host wait and, from the host, the uploads); *_minmax is [min, max] over the calls
  depth_adapt_ms     floor (a): srrg2_adapt_depth_image on the F32 depth image of the same frame (the dense call's own depth)
                     with the left image as intensity, from device memory -- the part of the call that is not stereo
  stereo_features_ms floor (b): srrg2_adapt_stereo_features on the same pair from the same memory -- the sparse call
                     the three ALTERNATE call by call
  bytes              what the call moves on the device, from the shapes (bytes_of below), and traffic_ms: that traffic at the
                     6.29 TB/s a float4 copy measures on this chip; over_traffic = dense_ms / traffic_ms, over_depth_adapt =
                     dense_ms / depth_adapt_ms
  restatement_ms     floor (c): tests/stereo_dense_restatement.py (numpy, one thread) at 640 x 480, 64 disparities, 4 paths,
                     once; the counters must agree
One JSON line on stdout, also written to profiles/stereo_dense_bench.json.

    python tools/bench_stereo_dense.py [--calls 20] [--sizes 480x640,720x1280] [--tag NAME] [--no-restatement]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import features_cases as fc  # noqa: E402
import stereo_cases as sc  # noqa: E402
import stereo_dense_restatement as sd  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping  # noqa: E402

BASELINE = 0.05  # z = 26.25 / disparity: the bands at 5, 12 and 20 pixels lie inside the depth gate
COPY_RATE = 6.29e12  # bytes / s: float4 copy measured on MI355X


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def summary(t):
    """-> (median, [min, max]), rounded"""
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def device_image(img):
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), img.strides[0])


def bytes_of(rows, cols, nd, max_disparity, paths):
    """bytes the call moves on the device, every array counted once per kernel that streams it (neighbour and census re-reads
    inside a kernel are cache hits by construction): census, the S volume per pass, selection, finish, the depth adaptor"""
    n = rows * cols
    h, w = max(rows - 6, 0), max(cols - 8 - max_disparity, 0)
    px, vol = h * w, h * w * nd * 2
    census = 2 * n + 16 * n
    if paths == 0:
        build = 16 * n + vol                    # both census images in, S out
    else:
        build = 4 * 16 * n + vol + 3 * 2 * vol  # per direction both census images; one store and three read-modify-writes of S
    select = vol + 8 * px + vol + 2 * h * (w + nd - 1)  # best + records, the diagonal read + dR
    finish = 8 * px + 2 * h * (w + nd - 1) + 5 * n
    adaptor = 4 * n + n + 36 * n                # Z and the left image in; points, normals, intensity out
    return census + build + select + finish + adaptor


def bench_pair(b, rows, cols, calls, restate, warmup=3):
    left = fc.rectangles(rows, cols, rows + cols)
    right = sc.shifted(left, 3 * rows + cols)
    scene, other, sparse = (mapping.Scene(b, 3) for _ in range(3))
    row = {"rows": rows, "cols": cols, "settings": []}
    tl, lpair = device_image(left)
    tr, rpair = device_image(right)
    for nd in (64, 128):
        for paths in (0, 4):
            for where in ("host", "device"):
                ad = adaptors.MeasurementAdaptorStereoDense()
                ad.set_camera_matrix(fc.CAMERA)
                ad.stereo.baseline, ad.stereo.max_disparity, ad.stereo.paths = BASELINE, nd, paths
                ad.set_meas(scene)
                st = adaptors.MeasurementAdaptorStereoFeatures()
                st.set_camera_matrix(fc.CAMERA)
                st.stereo.baseline = BASELINE
                st.set_meas(sparse)
                if where == "host":
                    ad.set_raw_data(left, right)
                    st.set_raw_data(left, right)
                else:
                    for a in (ad, st):
                        a.camera.rows, a.camera.cols = rows, cols
                        a.set_raw_data(lpair, rpair)
                # floor (a): the depth adaptor on this setting's own depth image, from device memory
                probe = adaptors.MeasurementAdaptorStereoDense(ad.stereo, ad.camera)
                probe.set_raw_data(left, right)
                probe.compute(want_result=False, want_disparity=True)
                depth = sd.depth_of(probe.disparity(), fc.CAMERA, BASELINE)
                tz = torch.from_numpy(depth).cuda()
                torch.cuda.synchronize()
                dep = adaptors.MeasurementAdaptorDepthImage()
                dep.set_camera_matrix(fc.CAMERA)
                dep.params.rows, dep.params.cols = rows, cols
                dep.set_meas(other)
                dep.set_raw_data((tz.data_ptr(), 4 * cols), lpair, depth_type=abi.IMAGE_F32, intensity_type=abi.IMAGE_U8)
                for _ in range(warmup):
                    ad.compute()
                    dep.compute()
                    st.compute()
                td, ta, tb = [], [], []
                for _ in range(calls):  # alternating: all three see the same neighbours on the machine
                    td.append(timed_ms(ad.compute))
                    ta.append(timed_ms(dep.compute))
                    tb.append(timed_ms(st.compute))
                s = {"disparities": nd, "paths": paths, "memory": where, "result": dict(ad.last),
                     "depth_adapt_result": dict(dep.last), "stereo_features_scene_size": st.last["scene_size"]}
                s["dense_ms"], s["dense_minmax"] = summary(td)
                s["depth_adapt_ms"], s["depth_adapt_minmax"] = summary(ta)
                s["stereo_features_ms"], s["stereo_features_minmax"] = summary(tb)
                s["bytes"] = bytes_of(rows, cols, nd, nd, paths)
                s["traffic_ms"] = round(s["bytes"] / COPY_RATE * 1e3, 4)
                s["over_traffic"] = round(s["dense_ms"] / s["traffic_ms"], 1)
                s["over_depth_adapt"] = round(s["dense_ms"] / s["depth_adapt_ms"], 1)
                if (ad.last["num_in_range"], ad.last["num_valid"]) != (dep.last["num_in_range"], dep.last["num_valid"]):
                    raise SystemExit("bench_stereo_dense: the scene's counters %s, the depth adaptor's %s" % (ad.last, dep.last))
                if restate and where == "host" and (rows, cols, nd, paths) == (480, 640, 64, 4):
                    t0 = time.perf_counter()
                    want = sd.adapt(left, right, fc.CAMERA, BASELINE, max_disparity=nd, paths=paths)
                    s["restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    if {k: want[k] for k in sd.COUNTERS} != dict(ad.last):
                        raise SystemExit("bench_stereo_dense: counters %s, the restatement's %s"
                                         % (ad.last, {k: want[k] for k in sd.COUNTERS}))
                    if want["disparity"].tobytes() != probe.disparity().tobytes():
                        raise SystemExit("bench_stereo_dense: the disparity image differs from the restatement's")
                    s["same_as_restatement"] = True
                row["settings"].append(s)
    del tl, tr
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_dense_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "stereo_dense", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "copy_rate_bytes_per_s": COPY_RATE, "pairs": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        out["pairs"].append(bench_pair(b, rows, cols, args.calls, not args.no_restatement))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
