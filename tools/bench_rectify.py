#!/usr/bin/env python3
"""Side bench of the rectification stage: srrg2_rectify_image / srrg2_rectify_pair on seeded 640 x 480 and 1280 x 720 images (a
features_cases image and its band-shifted copy, tests/stereo_cases.py) through the maps of a barrel-distorted stereo rig whose
right camera is turned by 0.02 rad, destinations in device memory.  Per size it reports
  image_ms / pair_ms   median HOST WALL CLOCK of the blocking call (order_on = NULL) on reused handles, from host and from device
                       memory; *_minmax is [min, max] over the calls
  chain_ms             raw pair in device memory -> srrg2_rectify_pair(order_on = scene), which only queues ->
                       srrg2_adapt_stereo_dense (64 disparities, 4 paths, with its result: the one wait)
  dense_alone_ms       the floor: srrg2_adapt_stereo_dense alone on the already rectified pair, same session
                       all of them ALTERNATE call by call; chain_over_dense_ms = chain_ms - dense_alone_ms
  set_ms               srrg2_rectifier_set (the map, once per camera), median of 5
  bytes_image / _pair  what a call moves on the device, from the shapes: the map (8 bytes per target pixel), the source once, the
                       target once; traffic_ms: that at the 6.29 TB/s a float4 copy measures on this chip
  restatement_ms       tests/rectify_restatement.py (numpy, one thread): build_map and remap of one image, once; same bits required
One JSON line on stdout, also written to profiles/rectify_bench.json.

    python tools/bench_rectify.py [--calls 30] [--sizes 480x640,720x1280] [--tag NAME] [--no-restatement]
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

import torch  # noqa: E402  (before the library: tests/conftest.py says why)

import features_cases as fc  # noqa: E402
import rectify_cases as rc  # noqa: E402
import rectify_restatement as rr  # noqa: E402
import stereo_cases as sc  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping  # noqa: E402

COPY_RATE = 6.29e12  # bytes / s: float4 copy measured on MI355X
DISTORTION = (-0.28, 0.07, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
BASELINE = 0.1


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


def bench_size(b, rows, cols, calls, restate, warmup=5):
    K = rc.K3(500.0 * cols / 640, 505.0 * cols / 640, 318.3 * cols / 640, 241.7 * rows / 480)
    R = rc.rotation("x", 0.02)
    t = -R @ np.array([BASELINE, 0.0, 0.0])
    left = fc.rectangles(rows, cols, rows + cols)
    right = sc.shifted(left, 3 * rows + cols)
    s = pkg.StereoRectifier()
    infos = s.set_calibration(K, DISTORTION, K, DISTORTION, R, t, (rows, cols))
    row = {"rows": rows, "cols": cols, "valid_share": [round(i["num_valid"] / i["num_pixels"], 4) for i in infos]}
    p = s.left.params
    row["set_ms"], row["set_minmax"] = summary([timed_ms(lambda: s.left._lib.srrg2_rectifier_set(s.left._h, C.byref(p), None)) for _ in range(5)])
    tl, lpair = device_image(left)
    tr, rpair = device_image(right)
    out_l, out_r = s.rectify(left, right)  # the destinations, reused by every call
    scene, floor_scene = mapping.Scene(b, 3), mapping.Scene(b, 3)

    def dense(meas, pair_l, pair_r):
        ad = adaptors.MeasurementAdaptorStereoDense()
        s.camera(ad.camera)
        ad.stereo.baseline, ad.stereo.max_disparity, ad.stereo.paths = s.baseline, 64, 4
        ad.set_meas(meas)
        ad.set_raw_data(pair_l, pair_r)
        return ad

    chain_ad = dense(scene, out_l.pair, out_r.pair)
    rect_l, rect_r = (torch.clone(o.tensor) for o in (out_l, out_r))  # the already rectified pair of the floor
    torch.cuda.synchronize()
    floor_ad = dense(floor_scene, (rect_l.data_ptr(), out_l.pair[1]), (rect_r.data_ptr(), out_r.pair[1]))

    def chain():
        s.rectify(lpair, rpair, order_on=scene, out=(out_l, out_r))
        chain_ad.compute()

    runs = {"image_host": lambda: s.left.rectify(left, out=out_l), "image_device": lambda: s.left.rectify(lpair, out=out_l, image_type=abi.IMAGE_U8),
            "pair_host": lambda: s.rectify(left, right, out=(out_l, out_r)), "pair_device": lambda: s.rectify(lpair, rpair, out=(out_l, out_r)),
            "chain": chain, "dense_alone": floor_ad.compute}
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    times = {k: [] for k in runs}
    for _ in range(calls):  # alternating: every call sees the same neighbours on the machine
        for k, fn in runs.items():
            times[k].append(timed_ms(fn))
    for k, v in times.items():
        row[k + "_ms"], row[k + "_minmax"] = summary(v)
    row["chain_over_dense_ms"] = round(row["chain_ms"] - row["dense_alone_ms"], 4)
    if dict(chain_ad.last) != dict(floor_ad.last):
        raise SystemExit("bench_rectify: the chain's counters %s, the floor's %s" % (chain_ad.last, floor_ad.last))
    row["dense_result"] = dict(chain_ad.last)
    n = rows * cols
    row["bytes_image"], row["bytes_pair"] = 10 * n, 20 * n
    row["traffic_image_ms"], row["traffic_pair_ms"] = (round(v / COPY_RATE * 1e3, 5) for v in (10 * n, 20 * n))
    if restate:
        t0 = time.perf_counter()
        uv, _ = rr.build_map(K, DISTORTION, s.R1, s.new_K, (rows, cols), (rows, cols))
        t1 = time.perf_counter()
        want = rr.remap(uv, left, 0)
        t2 = time.perf_counter()
        row["restatement_map_ms"], row["restatement_remap_ms"] = round((t1 - t0) * 1e3, 1), round((t2 - t1) * 1e3, 1)
        if not np.array_equal(s.left.map(), uv) or s.left.rectify(left).tobytes() != want.tobytes():
            raise SystemExit("bench_rectify: the map or the image differs from the restatement's")
        row["same_as_restatement"] = True
    del tl, tr
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "rectify", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0),
           "copy_rate_bytes_per_s": COPY_RATE, "sizes": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        out["sizes"].append(bench_size(b, rows, cols, args.calls, not args.no_restatement))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
