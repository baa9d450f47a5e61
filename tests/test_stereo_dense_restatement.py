"""CPU: the numpy restatement of the dense-stereo contract (tests/stereo_dense_restatement.py) against a plain per-pixel, per-path
Python loop written from DESIGN.md section 4 "Dense stereo"; the properties the contract states (no penalties = no aggregation,
the strict uniqueness test on flat and periodic images, the smallest-d rule, the empty rectangle, ranges without a runner-up);
the two-plane quality condition; the ABI (struct sizes, defaults, the exported call).  Only the ABI tests touch the library."""
import ctypes as C

import numpy as np
import pytest

import stereo_dense_cases as dc
import stereo_dense_restatement as sd

F = np.float32


# ---- the plain loop -------------------------------------------------------------------------------------------------------
def _census_bits(I, r, c):
    return [int(I[r + dy, c + dx]) < int(I[r, c]) for dy in range(-3, 4) for dx in range(-4, 5) if (dy, dx) != (0, 0)]


def _loop(left, right, dmin, dmax, paths, p1, p2, u, lr_check, lr_tol, subpixel):
    """disparity image (float32, 0 = none) and the three masks, pixel by pixel"""
    rows, cols = left.shape
    disp = np.zeros((rows, cols), F)
    masks = [np.zeros((rows, cols), bool) for _ in range(3)]
    R0, R1, C0, C1 = 3, rows - 4, 4 + dmax, cols - 5  # inclusive
    if R1 < R0 or C1 < C0:
        return disp, masks
    inside = lambda r, c: R0 <= r <= R1 and C0 <= c <= C1
    ds = list(range(dmin, dmax + 1))
    cost = {}
    for r in range(R0, R1 + 1):
        for c in range(C0, C1 + 1):
            a = _census_bits(left, r, c)
            for d in ds:
                b = _census_bits(right, r, c - d)
                cost[r, c, d] = sum(x != y for x, y in zip(a, b))
    S = dict(cost) if paths == 0 else {k: 0 for k in cost}
    if paths == 4:
        for er, ec in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            L = {}
            rs = range(R0, R1 + 1) if er >= 0 else range(R1, R0 - 1, -1)
            cs = range(C0, C1 + 1) if ec >= 0 else range(C1, C0 - 1, -1)
            for r in rs:
                for c in cs:
                    pr, pc = r - er, c - ec
                    if not inside(pr, pc):
                        for d in ds:
                            L[r, c, d] = cost[r, c, d]
                        continue
                    M = min(L[pr, pc, k] for k in ds)
                    for d in ds:
                        terms = [L[pr, pc, d], M + p2]
                        if d - 1 >= dmin:
                            terms.append(L[pr, pc, d - 1] + p1)
                        if d + 1 <= dmax:
                            terms.append(L[pr, pc, d + 1] + p1)
                        L[r, c, d] = cost[r, c, d] + min(terms) - M
            for k in S:
                S[k] += L[k]
    best = {}
    for r in range(R0, R1 + 1):
        for c in range(C0, C1 + 1):
            best[r, c] = min(ds, key=lambda d: (S[r, c, d], d))
    for r in range(R0, R1 + 1):
        for c in range(C0, C1 + 1):
            d0 = best[r, c]
            s0 = S[r, c, d0]
            masks[0][r, c] = True
            others = [S[r, c, d] for d in ds if abs(d - d0) > 1]
            if u > 0 and others and not min(others) * (100 - u) > 100 * s0:
                continue
            masks[1][r, c] = True
            if lr_check:
                x = c - d0
                dr = min((d for d in ds if inside(r, x + d)), key=lambda d: (S[r, x + d, d], d))
                if abs(dr - d0) > lr_tol:
                    continue
            masks[2][r, c] = True
            v = F(d0)
            if subpixel and dmin < d0 < dmax:
                a, b, cc = S[r, c, d0 - 1], s0, S[r, c, d0 + 1]
                D = a - 2 * b + cc
                if D > 0:
                    v = F(F(d0) + F(a - cc) / F(2 * D))
            disp[r, c] = v
    return disp, masks


LOOP_CASES = [("noise_12x30", dict(min_disparity=2, max_disparity=9)), ("noise_9x20", dict(min_disparity=1, max_disparity=5)),
              ("noise_12x30", dict(min_disparity=2, max_disparity=9, paths=0)),
              ("noise_12x30", dict(min_disparity=3, max_disparity=6, p1=3, p2=200, uniqueness_ratio=40, lr_tolerance=0)),
              ("noise_9x20", dict(min_disparity=1, max_disparity=5, uniqueness_ratio=0, lr_check=False, subpixel=False)),
              ("noise_9x20", dict(min_disparity=2, max_disparity=3, p1=0, p2=255)),
              ("rand_12x30", dict(min_disparity=2, max_disparity=9)), ("rand_9x20", dict(min_disparity=1, max_disparity=5, paths=0)),
              ("rand_12x30", dict(min_disparity=1, max_disparity=12, uniqueness_ratio=2, lr_tolerance=0))]


@pytest.mark.parametrize("name,kw", LOOP_CASES, ids=[str(i) for i in range(len(LOOP_CASES))])
def test_restatement_equals_the_plain_loop(name, kw):
    left, right = dc.named(name)
    p = dict(sd.DEFAULTS, **kw)
    got = sd.disparity(left, right, **kw)
    disp, (ev, un, co) = _loop(left, right, p["min_disparity"], p["max_disparity"], p["paths"], p["p1"], p["p2"],
                               p["uniqueness_ratio"], p["lr_check"], p["lr_tolerance"], p["subpixel"])
    assert ev.any()
    assert np.array_equal(got["evaluated"], ev) and np.array_equal(got["unique"], un) and np.array_equal(got["consistent"], co)
    assert got["disparity"].tobytes() == disp.tobytes()


def test_loop_cases_reach_both_outcomes_of_every_test():
    """the small pairs reject and accept pixels at the uniqueness test and at the left-right check, and some disparities are
    fractional: the comparison above says something about each rule"""
    seen = dict(not_unique=0, unique=0, inconsistent=0, consistent=0, fractional=0)
    for name, kw in LOOP_CASES:
        got = sd.disparity(*dc.named(name), **kw)
        seen["not_unique"] += int((got["evaluated"] & ~got["unique"]).sum())
        seen["unique"] += int(got["unique"].sum())
        seen["inconsistent"] += int((got["unique"] & ~got["consistent"]).sum())
        seen["consistent"] += int(got["consistent"].sum())
        seen["fractional"] += int((got["disparity"] != np.floor(got["disparity"])).sum())
    assert all(v > 0 for v in seen.values()), seen


# ---- properties -----------------------------------------------------------------------------------------------------------
def test_no_penalties_is_no_aggregation():
    """p1 = p2 = 0: every L_e is C (the minimum is M), S = 4 C -- the same winners, ratios and parabola as S = C"""
    left, right = dc.named("96x128")
    a = sd.disparity(left, right, paths=4, p1=0, p2=0, **dc.PAIR_RANGE)
    b = sd.disparity(left, right, paths=0, **dc.PAIR_RANGE)
    assert np.array_equal(a["S"], 4 * b["S"])
    assert a["disparity"].tobytes() == b["disparity"].tobytes() and b["consistent"].sum() > 1000
    for k in ("unique", "consistent"):
        assert np.array_equal(a[k], b[k])


def test_flat_pair_strict_uniqueness():
    left, right = dc.named("flat")
    kw = dict(min_disparity=3, max_disparity=12)
    rejected = sd.disparity(left, right, uniqueness_ratio=10, **kw)
    assert rejected["evaluated"].sum() == 42 * 44 and not rejected["unique"].any() and not rejected["disparity"].any()
    accepted = sd.disparity(left, right, uniqueness_ratio=0, **kw)
    ev = accepted["evaluated"]
    assert np.array_equal(accepted["consistent"], ev) and (accepted["disparity"][ev] == F(3.0)).all()


def test_tiled_pair_two_disparities_tie():
    """the 24-pixel period makes 10 and 34 equal everywhere: rejected at u = 10, the smallest d at u = 0"""
    left, right = dc.named("tiled")
    kw = dict(min_disparity=1, max_disparity=40)
    S = sd.disparity(left, right, **kw)["S"]
    assert np.array_equal(S[:, :, 10 - 1], S[:, :, 34 - 1])
    rejected = sd.disparity(left, right, uniqueness_ratio=10, **kw)
    assert rejected["evaluated"].any() and not rejected["unique"].any()
    accepted = sd.disparity(left, right, uniqueness_ratio=0, **kw)
    ev = accepted["evaluated"]
    assert np.array_equal(accepted["consistent"], ev) and (accepted["best"][ev] == 10).all()
    assert (np.abs(accepted["disparity"][ev] - F(10.0)) < 0.5).all()  # (the parabola moves it by less than half a pixel)


def test_empty_rectangle_and_one_column():
    rng = np.random.default_rng(3)
    for cols, width in ((20 + 8, 0), (20 + 9, 1)):
        left = rng.integers(0, 256, (12, cols)).astype(np.uint8)
        got = sd.disparity(left, left, min_disparity=4, max_disparity=20, uniqueness_ratio=0, lr_check=False)
        assert got["evaluated"].sum() == 6 * width
        assert (got["S"] is None) == (width == 0)
        if width:
            assert got["evaluated"][3:9, 24].all() and got["consistent"].sum() == 6
    assert not sd.disparity(np.zeros((6, 64), np.uint8), np.zeros((6, 64), np.uint8))["evaluated"].any()
    empty = sd.adapt(np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), dc.CAMERA, dc.BASELINE)
    assert empty["status"] == 1 and empty["num_pixels"] == 0 and empty["scene_size"] == 0


@pytest.mark.parametrize("nd", [1, 2])
def test_ranges_without_a_runner_up_pass_uniqueness(nd):
    left, right = dc.named("flat")  # (rejected everywhere as soon as there is an S2)
    got = sd.disparity(left, right, min_disparity=5, max_disparity=5 + nd - 1, uniqueness_ratio=99)
    assert got["evaluated"].any() and np.array_equal(got["unique"], got["evaluated"])
    assert not sd.disparity(left, right, min_disparity=5, max_disparity=7, uniqueness_ratio=99)["unique"].any()


# ---- the two-plane quality condition ----------------------------------------------------------------------------------------
def _share(paths):
    left, right, truth, visible = dc.two_plane(96, 128)
    got = sd.disparity(left, right, paths=paths, **dc.TWO_PLANE_RANGE)
    d = got["disparity"]
    good = got["consistent"] & (np.abs(d - truth) <= 1.0)
    accepted = d[got["consistent"]]
    return float((good & visible).sum()) / float(visible.sum()), float((accepted != np.floor(accepted)).mean())


def test_two_plane_quality():
    """aggregation pays: at least 0.98 of the visible pixels carry a disparity within +-1 of the truth with four paths (0.995
    here), the per-pixel cost alone is at least 0.05 lower (0.905 here); at least half of the disparities are fractional"""
    share4, fractional = _share(4)
    share0, _ = _share(0)
    print("two-plane: paths 4 %.4f, paths 0 %.4f, fractional %.4f" % (share4, share0, fractional))
    assert share4 >= 0.98
    assert share0 <= share4 - 0.05
    assert fractional >= 0.5


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import adaptors

    # srrg2_dense_stereo_params as the header declares it is a float and ten int32: 44 bytes (not the 48 once quoted for it)
    assert C.sizeof(abi.DenseStereoParams) == 44 and C.sizeof(abi.DenseStereoResult) == 32
    p = adaptors.default_dense_stereo_params()
    got = {n: getattr(p, n) for n, _ in p._fields_}
    assert got == dict(baseline=0.0, min_disparity=1, max_disparity=64, paths=4, p1=8, p2=48, uniqueness_ratio=10, lr_check=1,
                       lr_tolerance=1, subpixel=1, reserved=0)
    for k, v in sd.DEFAULTS.items():  # (the restatement's defaults are the library's)
        assert int(v) == got[k], k


def test_refusals_need_no_device():
    """everything is checked before a device is touched: codes and the call's name in the message"""
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi, adaptors

    lib = _capi.lib()
    cam, sp = adaptors.default_depth_params(), adaptors.default_dense_stereo_params()
    cam.rows, cam.cols = 48, 64
    img = np.zeros((48, 64), np.uint8)
    disp = np.full((48, 64), 7.0, F)

    def call(sp_ref=None, dptr=disp.ctypes.data, stride=256, istride=64):
        return lib.srrg2_adapt_stereo_dense(None, img.ctypes.data, istride, img.ctypes.data, istride, abi.MEM_HOST, C.byref(cam),
                                            C.byref(sp) if sp_ref is None else sp_ref, dptr, stride, None)

    assert call() == -1 and b"adapt_stereo_dense" in lib.srrg2_amd_last_error() and b"baseline" in lib.srrg2_amd_last_error()
    sp.baseline = 0.1
    assert call(dptr=None) == -1  # dst and disparity_out both NULL
    assert call(stride=252) == -1 and call(stride=258) == -1
    sp.max_disparity = 257
    assert call() == -4 and b"256" in lib.srrg2_amd_last_error()
    sp.max_disparity = 64
    cam.camera_matrix[1] = 0.5
    assert call() == -4
    cam.camera_matrix[1] = 0.0
    cam.rows, cam.cols = 20000, 100000  # 19994 x 99928 x 64 elements
    assert call(stride=400000, istride=100000) == -4 and b"volume" in lib.srrg2_amd_last_error()
    assert (disp == F(7.0)).all()
