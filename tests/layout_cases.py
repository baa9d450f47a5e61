"""Caller layouts for the cloud entry points (numpy only): packed clouds turned into what an integration hands over -- one array of
point structs with the normal inside the record and a status word behind it, K clouds pooled in one array behind other clouds'
records with an offsets table that does not start at 0 -- and the decoder back to the packed, zero-based arrays a layout denotes.

Every word of a record that is neither a coordinate nor a normal is junk: alternately a NaN and a denormal (a small enum), so a
kernel that reads a neighbouring word gets a value it cannot mistake for a coordinate silently.  The records around a pool's
clouds are DECOYS: true points moved by a third of the gate, with unit normals -- a kernel that reads them matches them, and the
result changes (tests/test_layout_cases.py shows that for every pooled case below, on the float64 oracle)."""
import numpy as np

from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

JUNK = (0x7FC00001, 0x00000003)  # a NaN and a denormal (a status enum)
STRIDES = {3: (12, 16, 28, 32, 44), 2: (8, 12, 20, 24)}
CORR = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])
TAIL = 3  # decoy records behind the last cloud of a pool


def normal_at(dim):
    return dim * 4


def holds_normals(dim, stride):
    """whether a record of `stride` bytes has room for the normal behind the coordinates"""
    return stride >= 2 * dim * 4


def _f32(a, dim):
    return np.ascontiguousarray(a, np.float32).reshape(-1, dim)


def records(points, normals, stride, normal_at=None):
    """one buffer of `stride`-byte records as (n, stride / 4) uint32 words: coordinates at byte 0, normals (if given) at byte
    `normal_at`, junk everywhere else"""
    dim = np.asarray(points).shape[1]
    points = _f32(points, dim)
    assert stride % 4 == 0 and stride >= dim * 4
    n, w = points.shape[0], stride // 4
    buf = np.empty((n, w), np.uint32)
    # (alternating along a record and from record to record, so that records with a single spare word carry both patterns)
    idx = np.arange(n)[:, None] + np.arange(w)[None, :]
    buf[:] = np.where(idx % 2 == 0, np.uint32(JUNK[0]), np.uint32(JUNK[1]))
    buf[:, :dim] = points.view(np.uint32)
    if normals is not None:
        assert normal_at is not None and normal_at % 4 == 0 and normal_at >= dim * 4 and normal_at + dim * 4 <= stride
        buf[:, normal_at // 4:normal_at // 4 + dim] = _f32(normals, dim).view(np.uint32)
    return buf


def unpack_records(buf, dim, normal_at=None):
    """(points, normals or None) of a buffer made by records()"""
    pts = np.ascontiguousarray(buf[:, :dim]).view(np.float32)
    nrm = None if normal_at is None else np.ascontiguousarray(buf[:, normal_at // 4:normal_at // 4 + dim]).view(np.float32)
    return pts, nrm


def decoys(cloud, normals, count, gate, start=0):
    """`count` decoy points: true points of `cloud` moved by a third of the gate along an axis, with unit normals (the point's own,
    or an axis)"""
    dim = cloud.shape[1]
    assert cloud.shape[0] > 0
    sel = (start + np.arange(count)) % cloud.shape[0]
    pts = np.array(cloud[sel], np.float32)
    step = np.zeros((count, dim), np.float32)
    step[np.arange(count), np.arange(count) % dim] = np.float32(gate / 3.0)
    pts += step
    if normals is not None:
        nrm = np.array(normals[sel], np.float32)
    else:
        nrm = np.zeros((count, dim), np.float32)
        nrm[:, dim - 1] = 1.0
    return pts, nrm


def moved(buf, dim, gate):
    """a buffer of records with every point moved by a third of the gate (normals and junk as they were): what a caller's
    buffer is overwritten with once a call has returned"""
    out = buf.copy()
    pts = np.ascontiguousarray(buf[:, :dim]).view(np.float32).copy()
    pts[np.arange(len(pts)), np.arange(len(pts)) % dim] += np.float32(gate / 3.0)
    out[:, :dim] = pts.view(np.uint32)
    return out


def single(points, normals, stride):
    """one cloud as records, in the form of a pool without an offsets table: normals inside the record where it has room, else
    (if given) in a packed array of their own"""
    dim = np.asarray(points).shape[1]
    inside = normals is not None and holds_normals(dim, stride)
    at = normal_at(dim) if inside else None
    out = dict(kind="clouds", dim=dim, stride=stride, normal_at=at, offsets=None, buf=records(points, normals if inside else None, stride, at),
               nbuf=None, nstride=0)
    if normals is not None and not inside:
        out["nbuf"], out["nstride"] = records(normals, None, dim * 4), dim * 4
    return out


def pooled(clouds, normals, lead, stride, gate, tail=TAIL):
    """K clouds in one array of `stride`-byte records behind `lead` decoy records (and `tail` behind the last cloud), with the
    offsets table (offsets[0] = lead).  Normals, if given, sit inside the record where it has room for them, else in an array of
    their own (packed, the same offsets).  The decoys are points of the first non-empty cloud."""
    K = len(clouds)
    dim = np.asarray(clouds[0]).shape[1]
    clouds = [_f32(c, dim) for c in clouds]
    has_n = normals is not None
    if has_n:
        normals = [_f32(n, dim) for n in normals]
    src = next(k for k in range(K) if clouds[k].shape[0] > 0)
    dl, dln = decoys(clouds[src], normals[src] if has_n else None, lead, gate, 0)
    dt, dtn = decoys(clouds[src], normals[src] if has_n else None, tail, gate, lead)
    pts = np.concatenate([dl] + clouds + [dt])
    nrm = np.concatenate([dln] + normals + [dtn]) if has_n else None
    inside = has_n and holds_normals(dim, stride)
    at = normal_at(dim) if inside else None
    offsets = np.zeros(K + 1, np.int32)
    offsets[0] = lead
    offsets[1:] = lead + np.cumsum([c.shape[0] for c in clouds])
    out = dict(kind="clouds", dim=dim, stride=stride, normal_at=at, offsets=offsets, buf=records(pts, nrm if inside else None, stride, at),
               nbuf=None, nstride=0)
    if has_n and not inside:
        out["nbuf"], out["nstride"] = records(nrm, None, dim * 4), dim * 4
    return out


def _decode(pool, offsets):
    pts, nrm = unpack_records(pool["buf"], pool["dim"], pool["normal_at"])
    if pool["nbuf"] is not None:
        nrm = unpack_records(pool["nbuf"], pool["dim"])[0]
    K = len(offsets) - 1
    clouds = [np.ascontiguousarray(pts[offsets[k]:offsets[k + 1]]) for k in range(K)]
    normals = None if nrm is None else [np.ascontiguousarray(nrm[offsets[k]:offsets[k + 1]]) for k in range(K)]
    return clouds, normals


def pooled_corrs(corrs, lead, num_fixed, num_moving, tail=TAIL):
    """K lists of correspondence records in one array behind `lead` decoy records: valid-looking pairs of wrong points"""
    corrs = [np.ascontiguousarray(c, CORR) for c in corrs]

    def wrong(count, start):
        d = np.zeros(count, CORR)
        i = start + np.arange(count)
        d["fixed_idx"] = (7 * i + 1) % max(num_fixed, 1)
        d["moving_idx"] = (13 * i + 5) % max(num_moving, 1)
        d["response"] = 1.0
        return d

    offsets = np.zeros(len(corrs) + 1, np.int32)
    offsets[0] = lead
    offsets[1:] = lead + np.cumsum([len(c) for c in corrs])
    return dict(kind="corrs", offsets=offsets, recs=np.ascontiguousarray(np.concatenate([wrong(lead, 0)] + corrs + [wrong(tail, lead)])))


def unpack(layout):
    """the packed, zero-based arrays a pooled layout denotes: (clouds, normals or None), or the K record arrays"""
    off = layout["offsets"]
    if layout["kind"] == "corrs":
        return [layout["recs"][off[k]:off[k + 1]].copy() for k in range(len(off) - 1)]
    return _decode(layout, off)


def ignoring_base(layout):
    """what a kernel that ignored offsets[0] would see: the same counts, taken from record 0 on"""
    off = layout["offsets"] - layout["offsets"][0]
    if layout["kind"] == "corrs":
        return [layout["recs"][off[k]:off[k + 1]].copy() for k in range(len(off) - 1)]
    return _decode(layout, off)


# ---- the pooled cases of tests/test_gpu_caller_layouts.py (test_layout_cases.py checks on the oracle that their decoys bite) ----
SE3, SE2 = abi.SE3_QUAT_RIGHT, abi.SE2_RIGHT
GATE3, GATE2 = 0.25, 0.3
ITERATIONS = 6
PAIR_LEADS = (5, 3)  # srrg2_align_pairs: the fixed pool's and the moving pool's lead
# srrg2_align_batch_slices: slice -> (lead, stride) of its pooled entry
SLICE_LAYOUT = {"nn2": {0: (2, 28), 1: (259, 16)}, "c3": {0: (259, 32)}}


def cue3():
    """SE(3) point-to-plane, Cauchy kernel, normal gate"""
    c = abi.default_slice_config(SE3)
    c.kind, c.finder, c.finder_max_distance = abi.SLICE_P2PLANE, abi.FINDER_NN_GATED, GATE3
    c.robustifier, c.robustifier_chi_threshold, c.finder_normal_cos = abi.ROBUST_CAUCHY, 0.05, 0.8
    return c


def cue2(slice_kind=abi.SLICE_P2P):
    """SE(2) point-to-point; the normal gate makes the normals count wherever both clouds bring them"""
    c = abi.default_slice_config(SE2)
    c.kind, c.finder, c.finder_max_distance, c.finder_normal_cos = slice_kind, abi.FINDER_NN_GATED, GATE2, 0.8
    return c


def single_case(dim):
    """one pair of clouds for set_fixed / set_moving / compute(): SE(3) point-to-plane at 3 000 points, SE(2) point-to-point at
    380 beams (up to 384 points a first compute() stays on the one-workgroup kernel)"""
    if dim == 3:
        return dict(kind=SE3, cfg=cue3(), gate=GATE3, data=syn.cloud_pair_3d(n=3000, seed=6000))
    return dict(kind=SE2, cfg=cue2(), gate=GATE2, data=syn.scan_pair_2d(beams=380, seed=6001))


def sizes(K, n):
    """K different cloud sizes up to n, an EMPTY cloud at k = 1"""
    return [0 if k == 1 else n - (k % 5) * (n // 9) - 3 * k for k in range(K)]


def _shuffled(seed, *arrays):
    """the arrays in one random order: a prefix of a cloud, and its last few points, are then spread over the whole scene"""
    perm = np.random.default_rng(seed).permutation(arrays[0].shape[0])
    return [np.ascontiguousarray(a[perm]) for a in arrays]


def batch_clouds(K, n=3000, seed=6100):
    """one fixed cloud and K moving clouds of different sizes (k = 1 empty) around it, SE(3), with normals"""
    d = syn.batch_3d(K=K, n=n, seed=seed, shared_fixed_group=max(K, 2), t_max=0.05, rpy_max_deg=1.5)
    ns = sizes(K, n) if K > 1 else [n - 7]
    mv = [_shuffled(seed + k, p["moving"], p["moving_normals"]) for k, p in enumerate(d)]
    return dict(kind=SE3, fixed=d[0]["fixed"], fixed_normals=d[0]["fixed_normals"], moving=[p[0][:m] for p, m in zip(mv, ns)],
                moving_normals=[p[1][:m] for p, m in zip(mv, ns)], guesses=[syn.identity(3)] * K)


def scans(K, beams=400, seed=6200):
    """K pairs of SE(2) scans of different sizes (k = 1 has an empty moving scan)"""
    out = []
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    for k, m in enumerate(sizes(K, beams) if K > 1 else [beams]):
        # (every pair is seen from a place of its own: a neighbour's records are not this pair's points)
        x, y, th = 0.4 * k, -0.3 * k, 0.15 * k
        Pf, Nf = syn.scan_2d(syn.se2(x, y, th), beams - 5 * k)
        Pm, Nm = syn.scan_2d(syn.se2(x + 0.04 + 0.01 * k, y - 0.02, th + np.deg2rad(1.0 + 0.5 * k)), beams)
        Pf, Nf = _shuffled(seed + k, f32(Pf), f32(Nf))
        Pm, Nm = _shuffled(seed + 50 + k, f32(Pm), f32(Nm))
        out.append(dict(fixed=Pf, fixed_normals=Nf, moving=Pm[:m], moving_normals=Nm[:m]))
    return out


def pair_clouds(K=4, n=3000, seed=6600):
    """K pairs of SE(3) clouds, every pair with a fixed cloud of its own (different sizes; k = 1 has an empty moving cloud)"""
    d = syn.batch_3d(K=K, n=n, seed=seed, shared_fixed_group=1, t_max=0.05, rpy_max_deg=1.5)
    out = []
    for k, (p, m) in enumerate(zip(d, sizes(K, n))):
        Pf, Nf = _shuffled(seed + k, p["fixed"], p["fixed_normals"])
        Pm, Nm = _shuffled(seed + 50 + k, p["moving"], p["moving_normals"])
        out.append(dict(fixed=Pf[: n - 11 * k], fixed_normals=Nf[: n - 11 * k], moving=Pm[:m], moving_normals=Nm[:m]))
    return out


def landmarks(K=4, n=600, seed=6300):
    """given-correspondences alignments: one fixed cloud, K moving clouds (k = 1 empty, with no records) and their records"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-5, 5, (n, 3))
    moving, corrs = [], []
    for k, m in enumerate(sizes(K, n)):
        X = syn.se3(rng.uniform(-0.3, 0.3, 3), np.deg2rad(rng.uniform(-10, 10, 3)))
        Xi = syn.se3_inv(X)
        M = (P[:m] @ Xi[:, :3].T + Xi[:, 3] + rng.normal(scale=0.002, size=(m, 3))).astype(np.float32)
        c = np.zeros(m, CORR)
        c["fixed_idx"] = c["moving_idx"] = rng.permutation(m)
        bad = rng.random(m) < 0.2
        c["moving_idx"][bad] = rng.integers(0, max(m, 1), int(bad.sum()))
        c["response"] = rng.uniform(0, 25, m).astype(np.float32)
        moving.append(M)
        corrs.append(c)
    return dict(kind=SE3, fixed=P.astype(np.float32), moving=moving, corrs=corrs, guesses=[syn.identity(3)] * K)


def nn2_case(K=4, seed=6400):
    """two nearest-neighbour SE(3) cue slices with clouds of their own (point-to-plane with normals, point-to-point without) plus
    a prior slice: setup(al) builds the handle, moving / moving_normals are {slice: [K clouds]} (k = 1 empty)"""
    from helpers import cue_config, prior_config

    d0 = syn.cloud_pair_3d(n=3000, seed=seed, t=(0.03, -0.02, 0.01), rpy_deg=(0.5, -1.0, 1.5))
    d1 = syn.cloud_pair_3d(n=2000, seed=seed + 1, t=(0.03, -0.02, 0.01), rpy_deg=(0.5, -1.0, 1.5))
    s0, s1 = sizes(K, 3000), sizes(K, 2000)[::-1]  # (slice 1: the empty cloud at k = K - 2)
    guesses = [syn.se3((0.002 * (k % 5), 0.0, -0.001 * (k % 3)), (0.0, 0.1 * (k % 4), 0.0)) for k in range(K)]

    def setup(al, is_oracle=False):
        al.set_params(max_iterations=ITERATIONS, min_num_inliers=10)
        a = al.add_slice(cue3())
        b = al.add_slice(cue_config(SE3, abi.SLICE_P2P, 0.3))
        p = al.add_slice(prior_config(SE3, info=[1e-2] * 6, sets_guess=0))
        al.set_fixed(a, d0["fixed"], d0["fixed_normals"])
        al.set_fixed(b, d1["fixed"])
        al.set_prior_measurement(p, syn.identity(3))

    return dict(kind=SE3, setup=setup, guesses=guesses, cue=(0, 1), gates={0: GATE3, 1: 0.3},
                moving={0: [d0["moving"][:m] for m in s0], 1: [d1["moving"][:m] for m in s1]},
                moving_normals={0: [d0["moving_normals"][:m] for m in s0], 1: None})


def c3_case(K=3, seed=6500):
    """the projective pack: a projective point-to-plane slice that owns the clouds and a reprojection slice that shares them, on
    the smallest image of tests/test_gpu_batch_slices.py"""
    import projective_restatement as pr
    from helpers import projective_config

    d = pr.rgbd_case(seed, rows=40, cols=56, fx=70.0, density=1.2, nonfinite=0.01, motion=(0.004, 0.008))
    n = d["moving"].shape[0]
    d["moving"], d["moving_normals"] = _shuffled(seed, d["moving"], d["moving_normals"])
    ms = [n - 40 * k for k in range(K)]
    guesses = [d["X_gt"] if k % 2 else syn.identity(3) for k in range(K)]

    def setup(al, is_oracle=False):
        al.set_params(max_iterations=5, min_num_inliers=10)
        a = al.add_slice(projective_config(SE3, abi.SLICE_P2PLANE, d, gate=0.05, robust=abi.ROBUST_CAUCHY, thr=1e-5))
        b = al.add_slice(projective_config(SE3, abi.SLICE_REPROJECTION, d, gate=0.05, robust=abi.ROBUST_CAUCHY, thr=0.5))
        al.set_fixed(a, d["fixed"], d["fixed_normals"])
        if is_oracle:  # (the oracle's slices read clouds of their own: the same data)
            al.set_fixed(b, d["fixed"], d["fixed_normals"])
        else:
            al.share_clouds(b, a)

    return dict(kind=SE3, setup=setup, guesses=guesses, cue=(0, 1), gates={0: 0.05}, shares={1: 0},
                moving={0: [d["moving"][:m] for m in ms]}, moving_normals={0: [d["moving_normals"][:m] for m in ms]})
