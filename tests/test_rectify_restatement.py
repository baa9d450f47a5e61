"""CPU: the numpy restatement of the rectification contract (tests/rectify_restatement.py) pinned by itself -- against per-pixel
loops over Python floats and ints, by the properties the contract promises (identity, integer shifts, constant images, the
inverse model), the stereo calibration's rotations against their geometry, and what rectification buys the dense stereo
restatement on a distorted, misaligned pair.  tests/test_gpu_rectify.py holds the library to the restatement, bit for bit."""
import math

import numpy as np
import pytest

import rectify_cases as rc
import rectify_restatement as rr
import stereo_dense_restatement as sd

INVALID = rr.INVALID


def _entry(r, c, K, dist, R, new_K, src_shape):
    """one entry of the map in Python floats, the contract line by line; None = invalid"""
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    nfx, nfy, ncx, ncy = (float(new_K[0, 0]), float(new_K[1, 1]), float(new_K[0, 2]), float(new_K[1, 2]))
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in dist)
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    x = (float(c) - ncx) / nfx
    y = (float(r) - ncy) / nfy
    X = (R[0][0] * x + R[1][0] * y) + R[2][0]
    Y = (R[0][1] * x + R[1][1] * y) + R[2][1]
    W = (R[0][2] * x + R[1][2] * y) + R[2][2]
    if not W > 0.0:
        return None
    xn = X / W
    yn = Y / W
    r2 = xn * xn + yn * yn
    num = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
    if not den > 0.0:
        return None
    rad = num / den
    xy = xn * yn
    xd = xn * rad + ((2.0 * p1) * xy + p2 * (r2 + 2.0 * (xn * xn)))
    yd = yn * rad + (p1 * (r2 + 2.0 * (yn * yn)) + (2.0 * p2) * xy)
    u = fx * xd + cx
    v = fy * yd + cy
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    U = math.floor(u * 256.0 + 0.5)
    V = math.floor(v * 256.0 + 0.5)
    if not (0 <= U <= 256 * (src_shape[1] - 1) and 0 <= V <= 256 * (src_shape[0] - 1)):
        return None
    return U, V


def _remap_loop(uv, src, border):
    rows, cols = uv.shape[:2]
    if src.dtype == np.uint8:
        out = np.zeros((rows, cols), np.uint8)
    else:
        out = np.zeros((rows, cols), np.uint16 if src.dtype == np.uint16 else np.uint32)
    bits = src if src.dtype != np.float32 else src.view(np.uint32)
    for r in range(rows):
        for c in range(cols):
            U, V = int(uv[r, c, 0]), int(uv[r, c, 1])
            if U == INVALID:
                out[r, c] = border if src.dtype == np.uint8 else (0 if src.dtype == np.uint16 else 0x7fc00000)
            elif src.dtype == np.uint8:
                x0, y0 = U >> 8, V >> 8
                x1, y1 = min(x0 + 1, src.shape[1] - 1), min(y0 + 1, src.shape[0] - 1)
                fx, fy = U & 255, V & 255
                out[r, c] = (int(src[y0, x0]) * (256 - fx) * (256 - fy) + int(src[y0, x1]) * fx * (256 - fy) +
                             int(src[y1, x0]) * (256 - fx) * fy + int(src[y1, x1]) * fx * fy + 32768) >> 16
            else:
                out[r, c] = bits[(V + 128) >> 8, (U + 128) >> 8]
    return out


@pytest.mark.parametrize("rot", sorted(rc.ROTATIONS))
@pytest.mark.parametrize("name", sorted(rc.MODELS))
def test_map_against_a_loop_over_python_floats(name, rot):
    K, dist, R, shape = rc.model(name, rot)
    for dst in ((67, 101), (3, 5)):
        new_K = rc.target_K(name, dst)
        uv, info = rr.build_map(K, dist, R, new_K, shape, dst)
        want = np.full(dst + (2,), INVALID, np.int64)
        for r in range(dst[0]):
            for c in range(dst[1]):
                e = _entry(r, c, K, dist, R, new_K, shape)
                if e is not None:
                    want[r, c] = e
        assert np.array_equal(uv, want), (name, rot, dst)
        ok = want[..., 0] != INVALID
        assert info["num_valid"] == int(ok.sum()) and info["num_pixels"] == dst[0] * dst[1]
        if ok.any():
            rows, cols = np.nonzero(ok)
            assert (info["first_row"], info["last_row"], info["first_col"], info["last_col"]) == \
                (rows.min(), rows.max(), cols.min(), cols.max())
        # both words are invalid together
        assert np.array_equal(uv[..., 0] == INVALID, uv[..., 1] == INVALID)


def test_valid_share_of_the_named_models():
    """the target = the source: every entry valid but for `pincushion` (its corners look outside the source) and `behind`"""
    for rot in rc.ROTATIONS:
        for name in rc.MODELS:
            K, dist, R, shape = rc.model(name, rot)
            _, info = rr.build_map(K, dist, R, K, shape, shape)
            share = info["num_valid"] / info["num_pixels"]
            if name == "pincushion":
                assert 0.85 < share < 0.93, (name, rot, share)
            elif name == "behind":
                assert share == 0.0, (name, rot, share)  # (W <= 0 left of column 33; the rest looks far past the source)
            elif rot == "identity":
                assert share == 1.0, (name, rot, share)
            else:  # (the tilted target looks past one edge of the source)
                assert share > 0.9, (name, rot, share)


def test_empty_source_or_target_and_a_target_behind_the_camera():
    K, dist, R, shape = rc.model("small")
    uv, info = rr.build_map(K, dist, R, K, shape, (0, 0))
    assert uv.shape == (0, 0, 2) and info == dict(num_pixels=0, num_valid=0, first_row=-1, last_row=-1, first_col=-1, last_col=-1)
    uv, info = rr.build_map(K, dist, R, K, (0, 0), (3, 5))
    assert (uv == INVALID).all() and info["num_valid"] == 0 and info["first_col"] == -1
    uv, info = rr.build_map(K, dist, rc.rotation("y", math.pi), K, shape, shape)  # W < 0 everywhere
    assert (uv == INVALID).all()
    uv, _ = rr.build_map(K, dist, rc.model("behind")[2], K, shape, rc.BEHIND_WIDE)  # (wide enough to see the source again)
    assert (uv[..., 0] == INVALID).any() and (uv[..., 0] != INVALID).any()
    assert rr.remap(uv, rc.image(shape), 9)[uv[..., 0] == INVALID].tolist() == [9] * int((uv[..., 0] == INVALID).sum())


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_remap_against_a_loop(kind):
    for name, dst in (("small", (37, 53)), ("behind", (19, 31)), ("small", (3, 5)), ("vga_barrel", (20, 27))):
        K, dist, R, shape = rc.model(name)
        if kind != "u8":
            R = np.eye(3)
        uv, _ = rr.build_map(K, dist, R, rc.target_K(name, dst), shape, dst)
        src = rc.image(shape, kind)
        got = rr.remap(uv, src, 200)
        want = _remap_loop(uv, src, 200)
        assert got.dtype == src.dtype and got.tobytes() == want.tobytes(), (name, dst)
    if kind == "f32":  # NaN payloads survive
        K, dist, R, shape = rc.model("small")
        uv, _ = rr.build_map(K, dist, np.eye(3), K, shape, shape)
        src = rc.nan_payload_image(shape)
        assert np.isnan(src).all() and len(np.unique(src.view(np.uint32))) > 1000
        assert rr.remap(uv, src).tobytes() == _remap_loop(uv, src, 0).tobytes()


def test_identity_returns_the_image():
    K, dist, R, shape = rc.model("identity")
    uv, info = rr.build_map(K, dist, R, K, shape, shape)
    r, c = np.mgrid[0:shape[0], 0:shape[1]]
    assert np.array_equal(uv[..., 0], 256 * c) and np.array_equal(uv[..., 1], 256 * r) and info["num_valid"] == r.size
    for src in (rc.image(shape), rc.image(shape, "u16"), rc.image(shape, "f32"), rc.nan_payload_image(shape)):
        assert rr.remap(uv, src, 5).tobytes() == src.tobytes()


def test_integer_shift_of_the_principal_point_shifts_the_image():
    K, dist, R, shape = rc.model("identity")
    new_K = K.copy()
    new_K[0, 2] += 4.0   # the target's centre moves right by 4: target pixel c shows source pixel c - 4
    new_K[1, 2] -= 3.0
    uv, _ = rr.build_map(K, dist, R, new_K, shape, shape)
    for kind, none in (("u8", 7), ("u16", 0)):
        src = rc.image(shape, kind)
        out = rr.remap(uv, src, 7)
        assert np.array_equal(out[:-3, 4:], src[3:, :-4])
        assert (out[:, :4] == none).all() and (out[-3:, :] == none).all()


@pytest.mark.parametrize("name", rc.DISTORTING)
def test_constant_image_stays_constant(name):
    K, dist, R, shape = rc.model(name, "tilted")
    for dst in ((37, 53), (67, 101)):
        uv, _ = rr.build_map(K, dist, R, rc.target_K(name, dst), shape, dst)
        ok = uv[..., 0] != INVALID
        for level in (0, 1, 137, 255):
            out = rr.remap(uv, np.full(shape, level, np.uint8), 200)
            assert (out[ok] == level).all() and (out[~ok] == 200).all(), (name, dst, level)


@pytest.mark.parametrize("rot", sorted(rc.ROTATIONS))
@pytest.mark.parametrize("name", rc.DISTORTING)
def test_inverse_model_recovers_the_target_pixel(name, rot):
    """every valid entry, taken back through the inverse model (fixed-point iteration, 30 steps), lands on its own target pixel
    within 1/128 px: the entry's quantisation is at most sqrt(2)/512 px in the source, times these models' magnification of
    less than 2.8"""
    K, dist, R, shape = rc.model(name, rot)
    uv, info = rr.build_map(K, dist, R, K, shape, shape)
    ok = uv[..., 0] != INVALID
    if name == "behind":  # (nothing of a target of the source's shape is valid: W <= 0, or far outside the source)
        assert info["num_valid"] == 0
        return
    assert info["num_valid"] > 100
    r, c = np.nonzero(ok)
    cc, rr_ = rc.source_to_target(uv[ok][:, 0] / 256.0, uv[ok][:, 1] / 256.0, K, dist, R, K)
    err = np.hypot(cc - c, rr_ - r)
    print("%s %s: max %.5f px over %d entries" % (name, rot, err.max(), err.size))
    assert err.max() <= 1.0 / 128.0, (name, rot, err.max())


# ---- stereo calibration -> rotations --------------------------------------------------------------------------------

def _calibrations():
    rng = np.random.default_rng(5)
    out = [(rc.RIG_K, rc.RIG_K, rc.RIG_R, rc.RIG_T)]
    for _ in range(6):
        R = rc.rotation("x", rng.uniform(-0.05, 0.05)) @ rc.rotation("y", rng.uniform(-0.08, 0.08))
        t = -R @ np.array([rng.uniform(0.05, 0.5), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
        KL = rc.K3(*rng.uniform(400, 600, 2), *rng.uniform(200, 330, 2))
        KR = rc.K3(*rng.uniform(400, 600, 2), *rng.uniform(200, 330, 2))
        out.append((KL, KR, R, t))
    return out


def _stereo_rectify_elementwise(KL, KR, R, t):
    """the contract again, scalar by scalar in Python floats"""
    R = [[float(v) for v in row] for row in np.asarray(R)]
    t = [float(v) for v in t]
    c = [-((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]) for i in range(3)]
    b = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    e1 = [v / b for v in c]
    zm = [(0.0 + R[2][0]) / 2.0, (0.0 + R[2][1]) / 2.0, (1.0 + R[2][2]) / 2.0]
    z = [zm[1] * e1[2] - zm[2] * e1[1], zm[2] * e1[0] - zm[0] * e1[2], zm[0] * e1[1] - zm[1] * e1[0]]
    zn = math.sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2])
    e2 = [v / zn for v in z]
    e3 = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    R1 = [e1, e2, e3]
    R2 = [[(R1[i][0] * R[j][0] + R1[i][1] * R[j][1]) + R1[i][2] * R[j][2] for j in range(3)] for i in range(3)]
    f = (float(KL[1, 1]) + float(KR[1, 1])) / 2.0
    Kn = [[f, 0.0, (float(KL[0, 2]) + float(KR[0, 2])) / 2.0], [0.0, f, (float(KL[1, 2]) + float(KR[1, 2])) / 2.0], [0.0, 0.0, 1.0]]
    return np.array(R1), np.array(R2), np.array(Kn), b


def test_stereo_rectify_against_elementwise_and_its_geometry():
    rng = np.random.default_rng(6)
    for KL, KR, R, t in _calibrations():
        R1, R2, Kn, b = rr.stereo_rectify(KL, KR, R, t)
        w1, w2, wk, wb = _stereo_rectify_elementwise(KL, KR, R, t)
        assert R1.tobytes() == w1.tobytes() and R2.tobytes() == w2.tobytes() and Kn.tobytes() == wk.tobytes() and b == wb
        for M in (R1, R2):
            assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(M) - 1.0) <= 1e-12
        assert np.abs(R2 @ R @ R1.T - np.eye(3)).max() <= 1e-12
        assert Kn[0, 0] == Kn[1, 1] == (KL[1, 1] + KR[1, 1]) / 2 and Kn[0, 1] == 0.0
        # 3-D points in the left frame: one row in both rectified cameras, x_L - x_R = f' baseline / z
        P = np.stack([rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50), rng.uniform(2, 9, 50)])
        PL = R1 @ P
        PR = R2 @ (R @ P + np.asarray(t)[:, None])
        xl, yl = Kn[0, 0] * PL[0] / PL[2] + Kn[0, 2], Kn[1, 1] * PL[1] / PL[2] + Kn[1, 2]
        xr, yr = Kn[0, 0] * PR[0] / PR[2] + Kn[0, 2], Kn[1, 1] * PR[1] / PR[2] + Kn[1, 2]
        assert np.abs(yl - yr).max() <= 1e-9
        assert np.abs(PL[2] - PR[2]).max() <= 1e-12
        assert np.abs((xl - xr) - Kn[0, 0] * b / PL[2]).max() <= 1e-9
        assert b > 0 and abs(b - np.linalg.norm(R.T @ t)) <= 1e-15


def test_stereo_rectify_refuses_both_degenerate_inputs():
    K = rc.RIG_K
    assert rr.stereo_rectify(K, K, np.eye(3), np.zeros(3)) is None            # one centre
    assert rr.stereo_rectify(K, K, np.eye(3), np.array([0.0, 0.0, -0.3])) is None  # the baseline along the optical axis
    assert rr.stereo_rectify(K, K, np.eye(3), np.array([-0.3, 0.0, 0.0])) is not None


# ---- what it buys the front end -----------------------------------------------------------------------------------------

def test_rectification_restores_dense_stereo_on_a_distorted_misaligned_pair():
    """two_plane_67x101 seen through the rig (distortion, the right camera turned by 0.02 rad): the dense stereo restatement on
    the raw pair against the same on the re-rectified pair, both against the ideal pair's disparity.  No absolute threshold:
    the rectified run must have more consistent pixels and the smaller mean absolute disparity error."""
    g = rc.rig()
    ideal = sd.disparity(*g["ideal"], **rc.RIG_RANGE)
    raw = sd.disparity(*g["raw"], **rc.RIG_RANGE)
    rect = sd.disparity(*rc.rig_rectified(), **rc.RIG_RANGE)

    def score(run):
        both = run["consistent"] & ideal["consistent"]
        err = np.abs(run["disparity"][both] - ideal["disparity"][both]).mean() if both.any() else float("inf")
        return int(run["consistent"].sum()), float(err)

    n_ideal = int(ideal["consistent"].sum())
    (n_raw, e_raw), (n_rect, e_rect) = score(raw), score(rect)
    print("consistent pixels / mean |d - d_ideal|: ideal %d, raw %d / %.3f, rectified %d / %.3f" % (n_ideal, n_raw, e_raw, n_rect, e_rect))
    assert n_rect > n_raw and e_rect < e_raw
