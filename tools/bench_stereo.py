#!/usr/bin/env python3
"""Side bench of the stereo-feature adaptor: srrg2_adapt_stereo_features on seeded synthetic pairs (tests/stereo_cases.py: a
features_cases image and its copy shifted by a disparity that is constant per band of 40 rows) of 640 x 480 and 1280 x 720, from
host and from device memory, with max_features 1000 and 0 (no cap).  Per pair and setting it reports
  stereo_ms          the adaptor: median HOST WALL CLOCK of a blocking call with result and records on a reused handle (device
                     time plus the call's two host waits and, from the host, the uploads); *_minmax is [min, max] over the calls
  two_extractions_ms the floor: two srrg2_adapt_image_features calls, left then right, on the same images in the same session
                     -- what extraction alone costs; the stereo call and the floor ALTERNATE call by call
  over_floor         (stereo - floor) / floor per alternation: median and [min, max] -- the share of matching + resolve (and of
                     the second wait) over the floor
  restatement_ms     tests/stereo_restatement.py (numpy, one thread) on the same pair, once -- with the cap only (its all-pairs
                     distance matrix is too large for the uncapped keypoint counts); the counters must agree
One JSON line on stdout, also written to profiles/stereo_bench.json.

    python tools/bench_stereo.py [--calls 20] [--sizes 480x640,720x1280] [--tag NAME] [--no-restatement] [--features-ab DIR]

--features-ab DIR: DIR holds the outputs of tools/bench_features.py of the parent commit (parent_*.json) and of this tree
(tree_*.json), run alternately in one session; they are embedded under "features_ab" with, per frame and key, the parent's
[min, max] over all its calls, whether each median of this tree lies inside it, and whether none lies above it.
"""
import argparse
import glob
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
import stereo_restatement as sr  # noqa: E402
import srrg2_slam_interfaces_amd as pkg  # noqa: E402
from srrg2_slam_interfaces_amd import _abi as abi, adaptors, mapping  # noqa: E402


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
    return t, (t.data_ptr(), img.shape[1])


def bench_pair(b, rows, cols, calls, restate, warmup=3):
    left = fc.rectangles(rows, cols, rows + cols)
    right = sc.shifted(left, 3 * rows + cols)
    scene, mono = mapping.Scene(b, 3), mapping.Scene(b, 3)
    row = {"rows": rows, "cols": cols, "settings": []}
    keep = []
    for max_features in (1000, 0):
        for where in ("host", "device"):
            st = adaptors.MeasurementAdaptorStereoFeatures()
            st.set_camera_matrix(sc.CAMERA)
            st.stereo.baseline = sc.BASELINE
            st.params.max_features = max_features
            st.set_meas(scene)
            singles = []
            for _ in range(2):
                ad = adaptors.MeasurementAdaptorImageFeatures()
                ad.set_camera_matrix(sc.CAMERA)
                ad.params.max_features = max_features
                ad.set_meas(mono)
                singles.append(ad)
            if where == "host":
                st.set_raw_data(left, right)
                singles[0].set_raw_data(left)
                singles[1].set_raw_data(right)
            else:
                tl, lpair = device_image(left)
                tr, rpair = device_image(right)
                keep += [tl, tr]
                for ad, p in zip(singles, (lpair, rpair)):
                    ad.camera.rows, ad.camera.cols = rows, cols
                    ad.set_raw_data(p, intensity_type=abi.IMAGE_U8)
                st.camera.rows, st.camera.cols = rows, cols
                st.set_raw_data(lpair, rpair)

            def floor():
                singles[0].compute()
                singles[1].compute()

            for _ in range(warmup):
                st.compute()
                floor()
            ts, tf = [], []
            for _ in range(calls):  # alternating: both see the same neighbours on the machine
                ts.append(timed_ms(st.compute))
                tf.append(timed_ms(floor))
            over = [(s - f) / f for s, f in zip(ts, tf)]
            s = {"max_features": max_features, "memory": where, "result": dict(st.last),
                 "extracted": [singles[0].last["scene_size"], singles[1].last["scene_size"]]}
            s["stereo_ms"], s["stereo_minmax"] = summary(ts)
            s["two_extractions_ms"], s["two_extractions_minmax"] = summary(tf)
            s["over_floor"], s["over_floor_minmax"] = summary(over)
            if (st.last["num_left"], st.last["num_right"]) != tuple(s["extracted"]):
                raise SystemExit("bench_stereo: the stereo call selected %s keypoints, the two extractions %s"
                                 % ((st.last["num_left"], st.last["num_right"]), s["extracted"]))
            if restate and max_features > 0 and where == "host":
                t0 = time.perf_counter()
                want = sr.match(left, right, sc.CAMERA, sc.BASELINE, max_features=max_features)
                s["restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                if {k: want[k] for k in sr.COUNTERS} != dict(st.last):
                    raise SystemExit("bench_stereo: counters %s, the restatement's %s" % (st.last, {k: want[k] for k in sr.COUNTERS}))
                s["same_counters_as_restatement"] = True
            row["settings"].append(s)
    return row


def features_ab(directory):
    """the alternated runs of tools/bench_features.py: per frame and key the parent's [min, max] over all its runs' calls, this
    tree's medians, and whether each of them lies inside"""
    runs = {who: [json.load(open(p)) for p in sorted(glob.glob(os.path.join(directory, who + "_*.json")))] for who in ("parent", "tree")}
    if not runs["parent"] or not runs["tree"]:
        raise SystemExit("bench_stereo: --features-ab needs parent_*.json and tree_*.json in %s" % directory)
    out = {"runs": runs, "frames": []}
    inside_all = not_slower_all = True
    for i, frame in enumerate(runs["parent"][0]["frames"]):
        rec = {"rows": frame["rows"], "cols": frame["cols"], "keys": {}}
        for key in frame["features_ms"]:
            lo = min(r["frames"][i]["features_minmax"][key][0] for r in runs["parent"])
            hi = max(r["frames"][i]["features_minmax"][key][1] for r in runs["parent"])
            medians = [r["frames"][i]["features_ms"][key] for r in runs["tree"]]
            inside = all(lo <= m <= hi for m in medians)
            not_slower = all(m <= hi for m in medians)  # (a median below the parent's fastest call is outside, not slower)
            inside_all, not_slower_all = inside_all and inside, not_slower_all and not_slower
            rec["keys"][key] = {"parent_minmax": [lo, hi], "parent_medians": [r["frames"][i]["features_ms"][key] for r in runs["parent"]],
                                "tree_medians": medians, "tree_inside_parent_spread": inside, "tree_not_above_parent_max": not_slower}
        out["frames"].append(rec)
    out["tree_inside_parent_spread"], out["tree_not_above_parent_max"] = inside_all, not_slower_all
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--sizes", default="480x640,720x1280", help="rows x cols, comma separated")
    ap.add_argument("--tag", default="")
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--features-ab", default="", help="directory with parent_*.json and tree_*.json of tools/bench_features.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_bench.json"))
    args = ap.parse_args()
    b = pkg.scene_binding(0)
    out = {"bench": "stereo", "tag": args.tag, "calls": args.calls, "device": torch.cuda.get_device_name(0), "pairs": []}
    for size in args.sizes.split(","):
        rows, cols = (int(v) for v in size.split("x"))
        out["pairs"].append(bench_pair(b, rows, cols, args.calls, not args.no_restatement))
    if args.features_ab:
        out["features_ab"] = features_ab(args.features_ab)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
