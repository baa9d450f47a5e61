#!/usr/bin/env python3
"""Side bench of the scale-pyramid feature adaptor: srrg2_adapt_image_features_pyramid on seeded synthetic frames
(tests/features_cases.py) of 640 x 480 and 1280 x 720, with 4 and 8 levels at 6/5, from host and from device memory.  Per setting
three blocking calls ALTERNATE, call by call in one session, and each reports the median [min, max] of its HOST WALL CLOCK:
  pyramid_ms      the pyramid call: every level behind ONE host wait, the levels resampled on the device
  level0_ms       floor 1: the plain srrg2_adapt_image_features call on level 0 alone (same cap)
  per_level_ms    floor 2, what a caller does without the pyramid: L plain calls, one per level, on level images resampled
                  BEFOREHAND (tests/pyramid_restatement.py; not timed) with the level's quota as cap -- L host waits
The pyramid call should sit between the two floors; it must be below floor 2.  `bytes` is what the pyramid call moves, computed
from the shapes: per level the single-scale pipeline's traffic (tools/bench_features.py), plus each resampled level read once
and written once.  Also checks the keypoint counts of the three ways against each other.  One JSON line on stdout, also written
to profiles/pyramid_bench.json.

    python tools/bench_pyramid.py [--calls 20] [--sizes 480x640,720x1280] [--levels 4,8] [--max-features 1000] [--tag NAME]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import features_cases as fc  # noqa: E402
import pyramid_restatement as pr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from bench_features import bytes_per_call, device_image  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping  # noqa: E402


def alternate_ms(fns, calls, warmup=3):
    """the calls of `fns` in turn, round by round -> per call (median, [min, max]), rounded"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    t = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [(round(float(np.median(v)), 4), [round(float(min(v)), 4), round(float(max(v)), 4)]) for v in t]


def plain_adaptor(scene, img, where, max_features, keep):
    ad = adaptors.MeasurementAdaptorImageFeatures()
    ad.set_camera_matrix(fc.CAMERA)
    ad.params.max_features = max_features
    ad.set_meas(scene)
    if where == "host":
        ad.set_raw_data(img)
    else:
        t, pair = device_image(img)
        keep.append(t)
        ad.camera.rows, ad.camera.cols = img.shape
        ad.set_raw_data(pair, None, intensity_type=abi.IMAGE_U8)
    return ad


def pyramid_bytes(sizes, kept, from_host):
    """per level the single-scale traffic; levels >= 1 are also written once by the resampler, which reads the level before"""
    total = {"upload": sizes[0][0] * sizes[0][1] if from_host else 0, "device": 0, "download": 0}
    for l, ((rows, cols), k) in enumerate(zip(sizes, kept)):
        b = bytes_per_call(rows, cols, k, 0, False)
        total["device"] += b["device"] + (rows * cols + sizes[l - 1][0] * sizes[l - 1][1] if l else 0)
        total["download"] += 32 * k + 8 * 4
    return total


def bench_setting(b, img, levels, where, calls, max_features):
    keep = []
    images = pr.build(img, levels, 6, 5)
    sizes = [im.shape for im in images]
    quota = pr.quotas(sizes, max_features)
    pyr = adaptors.MeasurementAdaptorImageFeaturesPyramid()
    pyr.set_camera_matrix(fc.CAMERA)
    pyr.params.max_features, pyr.pyramid.num_levels = max_features, levels
    pyr.set_meas(mapping.Scene(b, 3))
    if where == "host":
        pyr.set_raw_data(img)
    else:
        t, pair = device_image(img)
        keep.append(t)
        pyr.camera.rows, pyr.camera.cols = img.shape
        pyr.set_raw_data(pair, None, intensity_type=abi.IMAGE_U8)
    level0 = plain_adaptor(mapping.Scene(b, 3), img, where, max_features, keep)
    # a level whose quota is 0 keeps nothing: the caller skips it (inside the plain call 0 would mean "no cap")
    per_level = [plain_adaptor(mapping.Scene(b, 3), np.ascontiguousarray(im), where, q, keep)
                 for im, q in zip(images, quota) if not (max_features > 0 and q == 0)]

    def all_levels():
        for ad in per_level:
            ad.compute()

    (pm, pmm), (lm, lmm), (am, amm) = alternate_ms([pyr.compute, level0.compute, all_levels], calls)
    kept = pyr.last["num_with_depth"]
    apart = [ad.last["scene_size"] for ad in per_level]
    if [k for k, q in zip(kept, quota) if not (max_features > 0 and q == 0)] != apart:
        raise SystemExit("bench_pyramid: the pyramid kept %s, the per-level calls %s" % (kept, apart))
    return {"rows": img.shape[0], "cols": img.shape[1], "levels": levels, "levels_built": len(sizes), "from": where,
            "max_features": max_features, "pixels_over_level0": round(sum(r * c for r, c in sizes) / float(img.size), 3),
            "pyramid_ms": pm, "pyramid_minmax": pmm, "level0_ms": lm, "level0_minmax": lmm, "per_level_ms": am, "per_level_minmax": amm,
            "below_per_level": pm < am, "kept": kept, "bytes": pyramid_bytes(sizes, kept, where == "host")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--levels", default="4,8")
    ap.add_argument("--max-features", type=int, default=1000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "pyramid", "tag": args.tag, "calls": args.calls, "ratio": "6/5", "device": torch.cuda.get_device_name(0), "settings": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        img = fc.rectangles(rows, cols, rows + cols)
        for levels in (int(v) for v in args.levels.split(",")):
            for where in ("host", "device"):
                out["settings"].append(bench_setting(b, img, levels, where, args.calls, args.max_features))
    out["pyramid_below_per_level_everywhere"] = all(s["below_per_level"] for s in out["settings"])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
