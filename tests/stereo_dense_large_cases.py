"""Dense-stereo pairs at working sizes, past the launch caps of the grid-stride kernels of csrc/stereo_dense.hip, and what the
device has to make of them.  numpy only: nothing here knows the library (tests/test_stereo_dense_large_cases.py proves on the CPU
that each case reaches the path it is here for, tests/test_gpu_stereo_dense_large.py runs the device on them).

The three capped launches all go through `blocks_of(work, cap)`: at most `cap` workgroups of 256 threads, and a thread whose
index lies past cap * 256 is served by a further trip of the kernel's grid-stride loop ("trip" t covers the indices
t * CAP .. (t + 1) * CAP - 1).  Crossing a cap is not enough: the later trips have to hold pixels of the processed rectangle
(rows 3 .. rows - 4, columns 4 + max_disparity .. cols - 5), or they write zeros only.  540 x 972 and 1080 x 972 cross the caps
by 592 and 1 184 pixels -- the last one and two rows, which lie in the margin of 3 rows -- so `caps` and `caps3` have eight rows
more than that: 548 x 972 and 1088 x 972, the smallest multiples of four rows that put whole rows of the rectangle behind each
threshold.

k_sd_paths, k_sd_best and k_sd_right have one wave per line or pixel and no capped launch: there is no loop to reach.  k_sd_count's
cap (64 * 256 = 16 384) is crossed by every 120 x 160 case of tests/stereo_dense_cases.py.
"""
import numpy as np

import rectify_cases as rc
import stereo_dense_cases as dc
import stereo_dense_restatement as sd

F = np.float32
# indices 0 .. 2 n - 1 over the pixels of the left image, then of the right one:
SD_CENSUS_CAP = 4096 * 256  # hipLaunchKernelGGL(k_sd_census, dim3(blocks_of(2 * n, 4096)), dim3(256), ...)
# indices over the n pixels of the image:
SD_FINISH_CAP = 2048 * 256  # hipLaunchKernelGGL(k_sd_finish, dim3(blocks_of(n, 2048)), dim3(256), ...)
# indices over the H * W * ND elements of the volume, d fastest (paths == 0 only):
SD_COST_CAP = 4096 * 256  # hipLaunchKernelGGL(k_sd_cost, dim3(blocks_of((long long) g.H * g.W * g.ND, 4096)), dim3(256), ...)
WAVE = 64  # lane l of k_sd_paths / k_sd_best / k_sd_right holds the disparities of index l + 64 j, j < NJ

CAMERA, BASELINE = dc.CAMERA, dc.BASELINE
CAPS_RANGE = dict(min_disparity=3, max_disparity=10)
# name -> (pair name of stereo_dense_cases.named, the true shift or None, the parameter sets the device is held to)
CASES = {
    # second trip of k_sd_finish (pixels from 524 288 on: rows 540 .. 544 of the rectangle) and of k_sd_census (census indices
    # from 1 048 576 on: right-image pixels from row 530 on)
    "caps": ("noise_548x972_s5", 5, (CAPS_RANGE,)),
    # third trip of k_sd_finish (pixels from 1 048 576 on: rows 1 079 .. 1 084) and of k_sd_census (indices from 2 097 152 on:
    # right-image pixels from row 1 069 on); the split between the images, index n = 1 057 536, lies inside trip 2
    "caps3": ("noise_1088x972_s5", 5, (CAPS_RANGE,)),
    # k_sd_cost: a volume of 194 x 228 x 64 = 2 830 848 elements, three trips
    "cost": ("noise_200x300_s20", 20, (dict(min_disparity=1, max_disparity=64, paths=0),)),
    # the workload's own shape on structured content: NJ = 1, 474 horizontal lines of 568 and 568 vertical ones of 474
    "vga": ("two_plane_480x640", None, (dict(min_disparity=1, max_disparity=64),
                                        dict(min_disparity=1, max_disparity=64, subpixel=0, lr_tolerance=0))),
    # NJ = 2 on a rectangle of 354 x 504
    "wide": ("noise_360x640_s40", 40, (dict(min_disparity=1, max_disparity=128),)),
    # NJ = 4 with vertical lines of 58 pixels, horizontal ones of 136
    "deep": ("noise_64x400_s40", 40, (dict(min_disparity=1, max_disparity=256),)),
    # in `wide` and `deep` the winner, index 39, lies in every lane's first slot; here it lies in the last one: index 99 of 128
    # (slot 1 of 2, rectangle 58 x 264) and index 199 of 256 (slot 3 of 4, rectangle 58 x 136)
    "wide_far": ("noise_64x400_s100", 100, (dict(min_disparity=1, max_disparity=128),)),
    "deep_far": ("noise_64x400_s200", 200, (dict(min_disparity=1, max_disparity=256),)),
}
# what each case's rectangle and slot count must come out as: (H, W, ND, NJ)
GEOMETRY = {"caps": (542, 954, 8, 1), "caps3": (1082, 954, 8, 1), "cost": (194, 228, 64, 1), "vga": (474, 568, 64, 1),
            "wide": (354, 504, 128, 2), "deep": (58, 136, 256, 4), "wide_far": (58, 264, 128, 2), "deep_far": (58, 136, 256, 4)}


def pair(name):
    """(left, right) of a case (treat them as read-only)"""
    return dc.named(CASES[name][0])


def runs(name):
    """the parameter sets of a case"""
    return CASES[name][2]


def want(name, **kw):
    """stereo_dense_restatement.adapt of a case under kw, computed once and shared: stereo_dense_cases.want's own cache"""
    return dc.want(CASES[name][0], **kw)


def slots(nd):
    """NJ of srrg2_adapt_stereo_dense's dispatch: queue_volume<1> up to 64 disparities, <2> up to 128, <4> beyond"""
    return 1 if nd <= WAVE else 2 if nd <= 2 * WAVE else 4


def geometry(name, kw):
    """(H, W, ND, NJ) of a case under a parameter set"""
    rows, cols = pair(name)[0].shape
    r0, r1, c0, c1 = sd.rectangle(rows, cols, kw["max_disparity"])
    nd = kw["max_disparity"] - kw["min_disparity"] + 1
    return r1 - r0, c1 - c0, nd, slots(nd)


def volume_pixels(name, kw, first, last=None):
    """flat image pixel indices of the rectangle pixels that own the volume elements first .. last - 1 (last None: the end)"""
    rows, cols = pair(name)[0].shape
    H, W, nd, _ = geometry(name, kw)
    last = H * W * nd if last is None else last
    pix = np.unique(np.arange(first, last, dtype=np.int64) // nd)
    y, x = pix // W, pix % W
    return (3 + y) * cols + (4 + kw["max_disparity"] + x)


# ---- the rectify -> dense stereo chain at VGA -----------------------------------------------------------------------------------
# two cameras of the model `vga_barrel`, the right one turned by 0.01 rad about x (2.4 rows at the image centre, f = 505) and
# set 0.05 m to the right; the ideal pair is two_plane_480x640: z = f * 0.05 / disparity, the planes at 4.2 m and 1.8 m
VGA_RIG_MODEL = "vga_barrel"
VGA_RIG_R = rc.rotation("x", 0.01)
VGA_RIG_BASELINE = 0.05
VGA_RIG_T = -VGA_RIG_R @ np.array([VGA_RIG_BASELINE, 0.0, 0.0], np.float64)
VGA_RIG_RANGE = dict(min_disparity=1, max_disparity=64)
_RIG = {}


def vga_rig():
    """as rectify_cases.rig(): the ideal pair, the calibration, the raw pair the rig delivers and the restated rectified pair"""
    if not _RIG:
        import rectify_restatement as rr

        K, dist, _, shape = rc.model(VGA_RIG_MODEL)
        left, right = dc.named("two_plane_480x640")
        R1, R2, Knew, baseline = rr.stereo_rectify(K, K, VGA_RIG_R, VGA_RIG_T)
        raw = (rc.warp_to_source(left, K, dist, R1, Knew, shape, 501), rc.warp_to_source(right, K, dist, R2, Knew, shape, 502))
        maps = tuple(rr.build_map(K, dist, R, Knew, shape, shape)[0] for R in (R1, R2))
        _RIG.update(K=K, distortion=dist, shape=shape, ideal=(left, right), R1=R1, R2=R2, Knew=Knew, baseline=baseline, raw=raw,
                    maps=maps, rectified=tuple(rr.remap(m, img, 0) for m, img in zip(maps, raw)))
    return _RIG


def vga_rig_camera():
    """(camera matrix as 9 floats, baseline): the rig's target camera and baseline rounded to float32, as the rectifier hands
    them to the adaptor"""
    g = vga_rig()
    Kn = g["Knew"]
    return tuple(float(F(v)) for v in (Kn[0, 0], 0, Kn[0, 2], 0, Kn[1, 1], Kn[1, 2], 0, 0, 1)), float(F(g["baseline"]))


def want_vga_rig(camera9=None, baseline=None):
    """the dense restatement on the restated rectified pair, under the camera and baseline the rectifier hands the adaptor
    (default: vga_rig_camera())"""
    if camera9 is None:
        camera9, baseline = vga_rig_camera()
    key = ("want", tuple(camera9), float(baseline))
    if key not in _RIG:
        _RIG[key] = sd.adapt(*vga_rig()["rectified"], camera9, baseline, **VGA_RIG_RANGE)
    return _RIG[key]
