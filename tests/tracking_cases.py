"""Seeded cases of the feature-tracker tests (tests/test_gpu_tracking.py, tests/test_tracking_restatement.py).  numpy only:
nothing here knows the library.

A case is a dict: rows, cols, K (9 floats), pose (moving_in_sensor, 3 x 4), points (nm, 3) and moving_desc (nm, 32) of the
landmarks, fixed_pixels (nf, ascending) and fixed_desc (nf, 32) of the keypoints, and params (search_radius, max_distance,
min_margin, cross_check, depth_min, depth_max).  A landmark is made by un-projecting a chosen pixel at a chosen depth in the
sensor frame and moving it by the inverse of a known pose; a descriptor at a chosen Hamming distance from another by flipping
its first bits.  What each case is for stands in its builder; tests/test_tracking_restatement.py pins that the restatement
really sees it (candidate counts, lanes, ties).

SCAN_TILE: the exclusive scan (csrc/kernels_prep.hip) takes SCAN_THREADS * SCAN_ITEMS = 256 * 8 keep flags per workgroup; more
landmarks than that go through its second level.  The tracker's own kernels (csrc/tracking.hip, csrc/desc_band.hip) have one thread or wave per
element and no capped launch, so there is no other loop to reach; `large` also spans several workgroups of each of them.
"""
import numpy as np

import features_cases as fc
import features_restatement as fr

F = np.float32
SCAN_TILE = 256 * 8
WAVE = 64
K_SMALL = (50.0, 0.0, 23.5, 0.0, 50.0, 19.5, 0.0, 0.0, 1.0)
IDENTITY = np.eye(3, 4, dtype=F)
DEFAULTS = dict(search_radius=16, max_distance=48, min_margin=0, cross_check=True, depth_min=0.4, depth_max=8.0)
_CASES, _IMAGE = {}, {}


def pose(seed):
    """a small rigid motion (3 x 4 float32): a few degrees about a seeded axis, a few centimetres"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= 0.05 / np.linalg.norm(w)
    a = np.linalg.norm(w)
    k = w / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    return np.concatenate([R, rng.uniform(-0.05, 0.05, (3, 1))], axis=1).astype(F)


def unproject(pixels, cols, K, z):
    """sensor-frame points (float64) whose projection under K falls on the pixels' centres at depth z"""
    pixels = np.asarray(pixels, np.int64)
    K = np.asarray(K, np.float64).reshape(3, 3)
    z = np.broadcast_to(np.asarray(z, np.float64), pixels.shape)
    r, c = pixels // cols, pixels % cols
    return np.stack([(c - K[0, 2]) / K[0, 0] * z, (r - K[1, 2]) / K[1, 1] * z, z], -1)


def landmarks_at(pixels, cols, K, z, T):
    """map-frame points (float32) that T = moving_in_sensor brings onto the pixels (up to rounding)"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    S = unproject(pixels, cols, K, z)
    return ((S - T[:, 3]) @ T[:, :3]).astype(F)  # R^T (s - t)


def random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flipped(desc, bits):
    """the descriptor with its first `bits` bits flipped: Hamming distance `bits` from it"""
    d = np.array(desc, np.uint8).copy()
    full, rest = divmod(int(bits), 8)
    d[:full] ^= 0xFF
    if rest:
        d[full] ^= (1 << rest) - 1
    return d


def _case(name, rows, cols, K, T, points, moving_desc, fixed_pixels, fixed_desc, **params):
    pix = np.asarray(fixed_pixels, np.int64)
    assert (np.diff(pix) > 0).all() and (len(pix) == 0 or (pix[0] >= 0 and pix[-1] < rows * cols)), name
    p = dict(DEFAULTS)
    p.update(params)
    return dict(name=name, rows=rows, cols=cols, K=tuple(float(v) for v in K), pose=np.asarray(T, F).reshape(3, 4),
                points=np.ascontiguousarray(points, F).reshape(-1, 3), moving_desc=np.ascontiguousarray(moving_desc, np.uint8).reshape(-1, 32),
                fixed_pixels=pix.astype(np.int32), fixed_desc=np.ascontiguousarray(fixed_desc, np.uint8).reshape(-1, 32), params=p)


def with_params(case, **params):
    out = dict(case)
    out["params"] = dict(case["params"], **params)
    out["name"] = case["name"] + "|" + ",".join("%s=%s" % kv for kv in sorted(params.items()))
    return out


# ---- builders -----------------------------------------------------------------------------------------------------------------
def lane_stride(n_band):
    """64 x 256, radius 8: the row band of the landmarks (row 32) holds exactly n_band keypoints -- 1, 63, 64, 65, 200: the
    lanes' stride ends before, at and past one round -- and 30 more keypoints lie in rows outside it.  Eight landmarks along
    the row, keypoint descriptors within 40 bits of some landmark's, so bests, seconds and refusals all occur"""
    rows, cols, R = 64, 256, 8
    rng = np.random.default_rng(1000 + n_band)
    band = np.sort(rng.choice(np.arange((32 - R) * cols, (32 + R + 1) * cols), n_band, replace=False))
    band[0 if n_band == 1 else n_band // 2] = 32 * cols + 100  # (one keypoint right under a landmark)
    band = np.unique(band)
    while len(band) < n_band:  # (the forced pixel was drawn already)
        band = np.unique(np.r_[band, rng.integers((32 - R) * cols, (32 + R + 1) * cols)])
    outside = np.r_[rng.choice(np.arange(0, (32 - R) * cols), 15, replace=False), rng.choice(np.arange((32 + R + 1) * cols, rows * cols), 15, replace=False)]
    pix = np.sort(np.r_[band, outside])
    lm_pix = 32 * cols + np.array([100, 3, 60, 104, 140, 200, 252, 97])
    K = (120.0, 0.0, 127.5, 0.0, 120.0, 31.5, 0.0, 0.0, 1.0)
    T = pose(n_band)
    md = random_desc(rng, len(lm_pix))
    fd = np.stack([flipped(md[rng.integers(len(md))], rng.integers(0, 41)) for _ in pix])
    return _case("lane_stride_%d" % n_band, rows, cols, K, T, landmarks_at(lm_pix, cols, K, 2.0, T), md, pix, fd, search_radius=R,
                 max_distance=30)


def second_best():
    """8 x 200, radius 255: every keypoint is every landmark's candidate, the band starts at keypoint 0, so candidate j sits in
    lane j % 64.  130 keypoints far from everything, except per landmark a best (3 bits off) and a second (7 bits off) at
    chosen indices (best, second): the same lane (5, 69), a neighbouring lane (7, 8), the other half of the wave (9, 44), the
    same lane with the best in the second round (75, 11), both in the last partial round (128, 129), lanes 31 | 32 (31, 32).
    min_margin 4 accepts all, 5 none"""
    rows, cols = 8, 200
    rng = np.random.default_rng(77)
    slots = ((5, 69), (7, 8), (9, 44), (75, 11), (128, 129), (31, 32))
    pix = np.sort(rng.choice(rows * cols, 130, replace=False))
    fd = random_desc(rng, 130)
    md = random_desc(rng, len(slots))
    for k, (b, s) in enumerate(slots):
        fd[b], fd[s] = flipped(md[k], 3), flipped(md[k], 7)
    lm_pix = rng.choice(rows * cols, len(slots), replace=False)
    T = pose(78)
    K = (90.0, 0.0, 99.5, 0.0, 90.0, 3.5, 0.0, 0.0, 1.0)
    return _case("second_best", rows, cols, K, T, landmarks_at(lm_pix, cols, K, 1.5, T), md, pix, fd, search_radius=255, min_margin=4)


def ties():
    """40 x 48, radius 4.  Landmark 0: two candidates with the SAME descriptor (the lower j wins; h2 == h fails any margin).
    Landmarks 1 and 2: the same descriptor, different pixels, one shared keypoint at the same distance from both (the reverse
    direction keeps the lower i).  Landmark 3: a lone candidate (passes any margin).  Landmark 4: best 10, second 14"""
    rows, cols = 40, 48
    rng = np.random.default_rng(5)
    md = random_desc(rng, 5)
    md[2] = md[1]
    at = lambda r, c: r * cols + c
    pix = [at(5, 5), at(5, 7), at(20, 20), at(30, 40), at(31, 41), at(33, 8)]
    fd = [flipped(md[0], 6), flipped(md[0], 6), flipped(md[1], 9), flipped(md[4], 14), flipped(md[4], 10), flipped(md[3], 12)]
    lm_pix = [at(5, 6), at(19, 19), at(21, 21), at(33, 8), at(30, 41)]
    T = pose(6)
    return _case("ties", rows, cols, K_SMALL, T, landmarks_at(lm_pix, cols, K_SMALL, [1.0, 2.0, 3.0, 2.5, 1.2], T), md, pix, fd,
                 search_radius=4)


def borders():
    """40 x 48, radius 3: landmarks on the four corners and the four edges -- their windows are cut by the first and last row
    and column -- keypoints on and next to the borders, and one pair of keypoints at the end of one row and the start of the
    next (adjacent pixel indices, 47 columns apart: the column gate must tell them apart)"""
    rows, cols = 40, 48
    rng = np.random.default_rng(11)
    at = lambda r, c: r * cols + c
    lm_pix = [at(0, 0), at(0, 47), at(39, 0), at(39, 47), at(0, 20), at(39, 30), at(15, 0), at(25, 47)]
    pix = sorted({at(0, 0), at(1, 2), at(0, 46), at(2, 47), at(38, 1), at(39, 0), at(39, 47), at(37, 45), at(0, 19), at(3, 22),
                  at(38, 30), at(36, 33), at(15, 1), at(14, 47), at(16, 0), at(25, 46), at(26, 0), at(24, 47), at(4, 0), at(39, 43)})
    md = random_desc(rng, len(lm_pix))
    fd = np.stack([flipped(md[rng.integers(len(md))], rng.integers(0, 30)) for _ in pix])
    T = pose(12)
    return _case("borders", rows, cols, K_SMALL, T, landmarks_at(lm_pix, cols, K_SMALL, 2.0, T), md, pix, fd, search_radius=3,
                 max_distance=256)


def view_edges():
    """8 x 48, identity pose, K = (64, 0; 64, 0): u = 64 x / z exactly.  In turn: u + 0.5 exactly 0 (in view, column 0) and one
    ulp below (out); exactly cols (out) and one ulp below (in, column 47); v + 0.5 exactly 0 and exactly rows; c.z exactly
    depth_min and depth_max (in), one ulp outside each (out); c.z = 0, c.z < 0; NaN and inf coordinates"""
    rows, cols = 8, 48
    K = (64.0, 0.0, 0.0, 0.0, 64.0, 0.0, 0.0, 0.0, 1.0)
    z = F(2.0)
    x_of = lambda uf: F((F(uf) - F(0.5)) * z / F(64.0))  # (exact: powers of two)
    dn, up = lambda v: np.nextafter(F(v), F(-np.inf)), lambda v: np.nextafter(F(v), F(np.inf))
    y3 = x_of(3.5)  # row 3
    P = [(x_of(0.0), y3, z), (dn(x_of(0.0)), y3, z), (x_of(48.0), y3, z), (dn(x_of(48.0)), y3, z),
         (x_of(10.5), x_of(0.0), z), (x_of(10.5), x_of(8.0), z), (x_of(10.5), dn(x_of(8.0)), z),
         (0.0, 0.0, 0.5), (0.0, 0.0, dn(0.5)), (0.0, 0.0, 4.0), (0.0, 0.0, up(4.0)), (0.1, 0.1, 0.0), (0.1, 0.1, -1.0),
         (np.nan, 0.0, 2.0), (0.0, np.inf, 2.0), (0.0, 0.0, np.inf), (0.0, 0.0, np.nan), (-np.inf, 0.0, 2.0)]
    rng = np.random.default_rng(21)
    md = random_desc(rng, len(P))
    pix = np.arange(0, rows * cols, 5)
    fd = np.stack([flipped(md[rng.integers(len(md))], rng.integers(0, 60)) for _ in pix])
    return _case("view_edges", rows, cols, K, IDENTITY, np.array(P, F), md, pix, fd, search_radius=2, max_distance=256, depth_min=0.5,
                 depth_max=4.0)


def cross():
    """40 x 48, radius 5.  Landmarks 0 and 1 project onto ONE pixel with different descriptors; landmarks 2 and 3 share their
    best keypoint (3 is closer: with the cross check 2 goes, without it both stay); landmark 4's best keypoint prefers
    landmark 5, which itself prefers another keypoint (4 goes, 5 stays)"""
    rows, cols = 40, 48
    rng = np.random.default_rng(31)
    at = lambda r, c: r * cols + c
    md = random_desc(rng, 6)
    lm_pix = [at(8, 8), at(8, 8), at(20, 30), at(21, 31), at(32, 10), at(32, 13)]
    pix = [at(8, 9), at(9, 8), at(20, 31), at(31, 11), at(33, 14)]
    fd = [flipped(md[0], 4), flipped(md[1], 5), flipped(md[3], 2), flipped(md[5], 8), flipped(md[5], 3)]
    md[2], md[4] = flipped(md[3], 9), flipped(md[5], 20)
    T = pose(32)
    return _case("cross", rows, cols, K_SMALL, T, landmarks_at(lm_pix, cols, K_SMALL, [2.0, 2.5, 1.0, 1.5, 3.0, 3.5], T), md, pix, fd,
                 search_radius=5, max_distance=64)


def gates():
    """40 x 48: keypoints of distance 0, 1, 48, 49 and ~128 from their landmark, exactly under it and one pixel off: radius 0
    takes the exact pixel only, max_distance 0 the identical descriptor only"""
    rows, cols = 40, 48
    rng = np.random.default_rng(41)
    at = lambda r, c: r * cols + c
    md = random_desc(rng, 6)
    lm_pix = [at(5, 5), at(10, 20), at(15, 40), at(25, 8), at(30, 30), at(35, 44)]
    pix = [at(5, 5), at(10, 21), at(15, 40), at(16, 40), at(25, 8), at(30, 30), at(31, 31), at(35, 43)]
    fd = [md[0], md[1], flipped(md[2], 1), md[2], flipped(md[3], 48), flipped(md[4], 49), md[4], random_desc(rng, 1)[0]]
    T = pose(42)
    return _case("gates", rows, cols, K_SMALL, T, landmarks_at(lm_pix, cols, K_SMALL, 2.0, T), md, pix, fd)


def large():
    """96 x 128, radius 5: SCAN_TILE + 300 landmarks (the scan's second tile; ten workgroups of the per-landmark kernels, nearly
    600 of the wave-per-landmark one) against 300 keypoints, about a third of the landmarks out of view or out of depth"""
    rows, cols, nm, nf = 96, 128, SCAN_TILE + 300, 300
    rng = np.random.default_rng(51)
    K = (110.0, 0.0, 63.5, 0.0, 110.0, 47.5, 0.0, 0.0, 1.0)
    pix = np.sort(rng.choice(rows * cols, nf, replace=False))
    fd = random_desc(rng, nf)
    T = pose(52)
    src = rng.integers(0, nf, nm)  # every landmark is a keypoint seen again: a few pixels off, a few bits off
    r, c = pix[src] // cols + rng.integers(-4, 5, nm), pix[src] % cols + rng.integers(-4, 5, nm)
    lm_pix = np.clip(r, 0, rows - 1) * cols + np.clip(c, 0, cols - 1)
    stray = rng.random(nm) < 0.2  # (a fifth anywhere in the image: some windows are empty)
    lm_pix[stray] = rng.integers(0, rows * cols, int(stray.sum()))
    z = rng.uniform(0.2, 10.0, nm)  # (depth gate 0.4 .. 8)
    P = landmarks_at(lm_pix, cols, K, z, T)
    P[rng.random(nm) < 0.1] *= F(3.0)  # (some leave the image)
    md = np.stack([flipped(fd[s], rng.integers(0, 70)) for s in src])
    return _case("large", rows, cols, K, T, P, md, pix, fd, search_radius=5, max_distance=48, min_margin=2)


def _image_case(rows, cols):
    """a real extraction (tests/features_restatement.py) of the rows x cols image of features_cases as the measurement; the
    landmarks are its own keypoints at seeded depths, their descriptors with up to 30 bits flipped, seen from a pose a little
    off the true one; every third landmark is dropped and the rest shuffled (the map's order is not the image's)"""
    if (rows, cols) not in _IMAGE:
        K = (60.0, 0.0, (cols - 1) / 2.0, 0.0, 60.0, (rows - 1) / 2.0, 0.0, 0.0, 1.0)
        ex = fr.extract(fc.image(rows, cols), K=K, fast_threshold=20, max_features=0)
        rng = np.random.default_rng(rows * cols)
        pix, fd = ex["global_indices"].astype(np.int64), ex["descriptors"]
        T = pose(rows + cols)
        order = rng.permutation(len(pix))
        order = order[order % 3 != 0]
        P = landmarks_at(pix[order], cols, K, rng.uniform(1.0, 4.0, len(order)), T)
        md = np.stack([flipped(fd[s], rng.integers(0, 31)) for s in order]) if len(order) else np.zeros((0, 32), np.uint8)
        T2 = T.copy()
        T2[:, 3] += np.array([0.03, -0.02, 0.01], F)  # (a couple of pixels at these depths)
        _IMAGE[(rows, cols)] = _case("image_%dx%d" % (rows, cols), rows, cols, K, T2, P, md, pix, fd, search_radius=6, max_distance=40,
                                     min_margin=3)
    return _IMAGE[(rows, cols)]


BUILDERS = dict(lane_stride_1=lambda: lane_stride(1), lane_stride_63=lambda: lane_stride(63), lane_stride_64=lambda: lane_stride(64),
                lane_stride_65=lambda: lane_stride(65), lane_stride_200=lambda: lane_stride(200), second_best=second_best, ties=ties,
                borders=borders, view_edges=view_edges, cross=cross, gates=gates, large=large,
                image_48x64=lambda: _image_case(48, 64), image_67x101=lambda: _image_case(67, 101))
NAMES = tuple(BUILDERS)


def case(name):
    """the case of a name, built once and shared (treat it as read-only)"""
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


# beyond the case as built and the same with the cross check off (every builder leaves it on): the parameter sets per case
EXTRA = {
    "second_best": [dict(min_margin=5), dict(min_margin=5, cross_check=False), dict(min_margin=0)],
    "ties": [dict(min_margin=1), dict(min_margin=4), dict(min_margin=5), dict(min_margin=256), dict(min_margin=4, cross_check=False)],
    "gates": [dict(search_radius=0), dict(max_distance=0), dict(max_distance=256), dict(search_radius=255),
              dict(search_radius=0, max_distance=0, cross_check=False), dict(search_radius=1, max_distance=48)],
    # (keypoints in rows 0 and rows - 1: 39 is the radius at which a band from one extreme row ends exactly on the other --
    # max(r - R, 0) and min(r + R, rows - 1) hit their limits unclamped -- and 40 the first that is cut there)
    "borders": [dict(search_radius=255), dict(search_radius=0), dict(search_radius=39), dict(search_radius=40, cross_check=False)],
    "image_48x64": [dict(min_margin=0), dict(search_radius=20, max_distance=256)],
}
# (name, k) of every variant, without building a case
VARIANTS = tuple((n, k) for n in NAMES for k in range(2 + len(EXTRA.get(n, []))))


def variants(name):
    """the case with the parameter sets the tests hold the device to"""
    c = case(name)
    return [c, with_params(c, cross_check=False)] + [with_params(c, **kw) for kw in EXTRA.get(name, [])]


def want(c):
    """tracking_restatement.track of a case"""
    import tracking_restatement as tr

    return tr.track(c["points"], c["moving_desc"], c["fixed_pixels"], c["fixed_desc"], c["pose"], c["K"], c["rows"], c["cols"], **c["params"])
