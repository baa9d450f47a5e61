#!/usr/bin/env python3
"""Side bench of the image-feature adaptor: srrg2_adapt_image_features on seeded synthetic frames (tests/features_cases.py:
random rectangles + noise) of 640 x 480 and 1280 x 720, with and without a depth image, from host and from device memory.  Per
frame it reports
  features_ms        the adaptor: median HOST WALL CLOCK of a blocking call with result and keypoints on a reused handle (device
                     time plus the call's host wait and, from the host, the upload); *_minmax is [min, max] over the same calls
  depth_compact_ms   srrg2_adapt_depth_image in compact mode (normals at gap 1, intensity carried) on the same frame: what the
                     dense path costs for the same image
  restatement_ms     tests/features_restatement.py (numpy, one thread) on the same frame, once
  bytes              moved per call, computed from the shapes: the image(s) read by the score kernel (and uploaded, from the host),
                     the score / box / flag / scan arrays written and read once each, the scene written
and checks that the keypoint count of the library is the restatement's.  One JSON line on stdout, also written to
profiles/features_bench.json.

    python tools/bench_features.py [--calls 20] [--sizes 480x640,720x1280] [--max-features 1000] [--tag NAME] [--no-restatement]
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
import features_restatement as fr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping  # noqa: E402


def stats_ms(fn, calls, warmup=3):
    """-> (median, [min, max]), rounded"""
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4), [round(float(min(t)), 4), round(float(max(t)), 4)]


def bytes_per_call(rows, cols, keypoints, depth_bytes, from_host):
    """bytes the call moves, from the shapes alone (the padded images are whole 64 x 16 tiles)"""
    n = rows * cols
    padded = -(-cols // 64) * 64 * (-(-rows // 16) * 16)
    upload = (n + n * depth_bytes) if from_host else 0
    score_box = n + padded * (1 + 2)               # image read once; score U8 + box U16 written
    maxima = padded + n                            # score read, flag written
    cap = (padded + n + 4 * n) + 3 * 4 * n         # tie flags: score + flag read, tie written; its scan: read, write, read-add
    select = n + 4 * n + 4 * n + 3 * 4 * n         # flag + tie read, keep written; the compaction scan
    scatter = 2 * 4 * n + 4 * keypoints
    describe = keypoints * (709 + 512 * 2 + 4 * 256 + 16 + 16 + 4 + 32 + 16 + depth_bytes)
    return {"upload": upload, "device": score_box + maxima + cap + select + scatter + describe,
            "download": 16 * keypoints + 4 * 4 + 4}


def device_image(img):
    t = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(img.shape[0], -1)).cuda()
    torch.cuda.synchronize()
    return t, (t.data_ptr(), img.shape[1] * img.itemsize)


def bench_frame(b, rows, cols, calls, max_features, restate):
    img = fc.rectangles(rows, cols, rows + cols)
    depth = fc.depth_for(img, "u16")
    scene, dense = mapping.Scene(b, 3), mapping.Scene(b, 3)
    row = {"rows": rows, "cols": cols, "max_features": max_features, "features_ms": {}, "features_minmax": {}, "bytes": {},
           "result": {}}
    keep = []
    for with_depth in (False, True):
        for where in ("host", "device"):
            ad = adaptors.MeasurementAdaptorImageFeatures()
            ad.set_camera_matrix(fc.CAMERA)
            ad.params.max_features = max_features
            ad.set_meas(scene)
            if where == "host":
                ad.set_raw_data(img, depth if with_depth else None)
            else:
                ti, ipair = device_image(img)
                keep.append(ti)
                dpair = None
                if with_depth:
                    td, dpair = device_image(depth)
                    keep.append(td)
                ad.camera.rows, ad.camera.cols = rows, cols
                ad.set_raw_data(ipair, dpair, intensity_type=abi.IMAGE_U8, depth_type=abi.IMAGE_U16 if with_depth else None)
            key = "%s_%s" % ("depth" if with_depth else "mono", where)
            row["features_ms"][key], row["features_minmax"][key] = stats_ms(ad.compute, calls)
            row["result"]["depth" if with_depth else "mono"] = dict(ad.last)
            row["bytes"][key] = bytes_per_call(rows, cols, ad.last["scene_size"], 2 if with_depth else 0, where == "host")
    # the dense path on the same frame: depth image -> compact cloud with normals, the intensity carried along
    row["depth_compact_ms"], row["depth_compact_minmax"] = {}, {}
    for where in ("host", "device"):
        dp = adaptors.MeasurementAdaptorDepthImage()
        for i, v in enumerate(fc.CAMERA):
            dp.params.camera_matrix[i] = float(v)
        dp.params.compact = 1
        dp.set_meas(dense)
        if where == "host":
            dp.set_raw_data(depth, img)
        else:
            td, dpair = device_image(depth)
            ti, ipair = device_image(img)
            keep += [td, ti]
            dp.params.rows, dp.params.cols = rows, cols
            dp.set_raw_data(dpair, ipair, depth_type=abi.IMAGE_U16, intensity_type=abi.IMAGE_U8)
        row["depth_compact_ms"][where], row["depth_compact_minmax"][where] = stats_ms(dp.compute, calls)
        row["depth_compact_points"] = dp.last["scene_size"]
    if restate:
        t0 = time.perf_counter()
        want = fr.extract(img, K=fc.CAMERA, max_features=max_features, depth=depth)
        row["restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        row["same_count_as_restatement"] = want["scene_size"] == row["result"]["depth"]["scene_size"]
        if not row["same_count_as_restatement"]:
            raise SystemExit("bench_features: the library kept %d keypoints, the restatement %d"
                             % (row["result"]["depth"]["scene_size"], want["scene_size"]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--max-features", type=int, default=1000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "features", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0), "frames": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        out["frames"].append(bench_frame(b, rows, cols, args.calls, args.max_features, not args.no_restatement))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
