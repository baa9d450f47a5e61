"""GPU: srrg2_tsdf_* (csrc/tsdf.hip) against the numpy restatement of its contract (tests/tsdf_restatement.py), BIT FOR BIT: the
planes, the result's counters, the raycast's depth image and scene, the exported scene and its global indices, at the smallest
shapes where the kernels can go wrong (tests/tsdf_cases.py); takes a batch out again, splits it, reverses it, queues it; refusals
leave planes and destinations as they were; and through the stack: a depth frame aligns against the raycast of the volume."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptor_restatement as ar
import tsdf_cases as tc
import tsdf_restatement as tr
from helpers import projective_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import mapping

pytestmark = pytest.mark.gpu
F = np.float32
E_INVALID, E_UNSUPPORTED = -1, -4
ROWS, COLS = 20, 26


def _volume_of(product, v, cam, mu, **adaptor):
    t = product.TsdfVolume(0)
    t.reset(v["nx"], v["ny"], v["nz"], float(v["vs"]), [float(x) for x in v["o"]], v["with_intensity"])
    t.set_camera(cam["K"], cam["rows"], cam["cols"], float(cam["scale"]), float(cam["dmin"]), float(cam["dmax"]), **adaptor)
    t.frame.mu = float(mu)
    return t


def _same_planes(t, planes, what=""):
    got = t.planes()
    for name, g, w in zip(("sum", "weight", "isum"), got, planes):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), "%s %s" % (name, what)
    assert (got[2] is None) == (len(planes) == 2)


def _same_raycast(product, t, planes, v, cam, pose, step, min_weight=1, what="", compact=False):
    """the depth image with and without the block mask, and the scene the depth adaptor makes of it, against the restatement"""
    want, want_inten = tr.raycast(planes, v, cam, pose, step, min_weight)
    scene = mapping.Scene(product.scene_binding(0), 3)
    t.ray.step, t.ray.min_weight, t.camera.compact = float(step), int(min_weight), int(compact)
    for skip in (1, 0):
        t.ray.skip_empty = skip
        got, res = t.raycast(pose, scene)
        assert tr.same_bits(got, want), "depth image, skip_empty %d %s" % (skip, what)
        assert res["num_pixels"] == want.size and res["num_surface"] == int((want != 0).sum()), what
        r = ar.adapt_depth_image(want, cam["K"], float(cam["scale"]), float(cam["dmin"]), float(cam["dmax"]), compact=compact,
                                 intensity=want_inten)
        assert res["adapt"]["num_in_range"] == r["num_in_range"] and res["adapt"]["num_valid"] == r["num_valid"], what
        assert scene.size() == r["points"].shape[0], what
        pts, nrm = scene.get()
        assert ar.same_bits(pts, r["points"]) and ar.same_bits(nrm, r["normals"]), "scene " + what
        assert scene.has_features() == (False, want_inten is not None)
        if want_inten is not None:
            assert ar.same_bits(scene.features()[1], r["intensity"]), "scene intensity " + what
        if compact:
            assert np.array_equal(scene.global_indices(), r["global_indices"]), what
    return want


def _same_export(product, t, planes, v, min_weight=1, what=""):
    pts, nrm, idx = tr.to_scene(planes, v, min_weight)
    scene = mapping.Scene(product.scene_binding(0), 3)
    assert t.to_scene(scene, min_weight) == len(idx) == scene.size(), what
    got_p, got_n = scene.get()
    assert tr.same_bits(got_p, pts), "export points " + what
    assert tr.same_bits(got_n, nrm), "export normals " + what
    assert np.array_equal(scene.global_indices(), idx), "export indices " + what
    assert scene.device_arrays()[1] is not None
    return len(idx)


def _around_the_wall(dims, vs=0.11, with_intensity=False):
    """a volume of `dims` voxels centred on the room's far wall"""
    nx, ny, nz = dims
    return tr.volume(nx, ny, nz, vs, (-0.5 * nx * vs, -0.5 * ny * vs, float(tc.ROOM_HI[2]) - 0.5 * nz * vs), with_intensity)


@functools.lru_cache(maxsize=None)
def _frames(n=5, seed=21, focal=60.0):
    K, poses, depth = tc.room_frames(n, ROWS, COLS, seed, focal=focal)
    depth = tc.spoiled(depth, seed + 1)
    inten = tc.intensity_like(depth, seed + 2)
    for a in (K, poses, depth, inten):
        a.setflags(write=False)
    return K, poses, depth, inten


@functools.lru_cache(maxsize=None)
def _reference(dims):
    K, poses, depth, _ = _frames()
    v = _around_the_wall(dims)
    cam = tr.camera(K, ROWS, COLS, 0.001, 0.4, 3.0)
    planes = tr.new_planes(v)
    out = tr.integrate(planes, v, cam, depth, poses, 0.15)
    for p in planes:
        p.setflags(write=False)
    return v, cam, poses, depth, planes, out


@pytest.mark.parametrize("dims", tc.VOLUMES, ids=str)
def test_shapes_bit_for_bit(product, dims):
    """sides that are no multiple of the 64-voxel run or the mask block, one voxel, an empty volume; the frustum of every frame
    cuts the volume on every side (focal 60 over 26 columns against volumes up to 7 m wide)"""
    v, cam, poses, depth, planes, want = _reference(dims)
    t = _volume_of(product, v, cam, 0.15)
    assert t.integrate(depth, poses) == want, dims
    _same_planes(t, planes, str(dims))
    if min(dims) > 0 and dims != (1, 1, 1):
        assert 0 < want["num_voxel_updates"] < 5 * dims[0] * dims[1] * dims[2]
    assert 0 < want["num_valid_depth"] < want["num_pixels"]
    _same_raycast(product, t, planes, v, cam, poses[0], 0.11, what=str(dims))
    _same_raycast(product, t, planes, v, cam, tc.pose(0.05, -0.3, 0.02, (0.4, 0.1, 0.3)), 0.05, 2, what=str(dims), compact=True)
    for need in (1, 4):
        _same_export(product, t, planes, v, need, str(dims))


def test_views_that_update_nothing(product):
    """a camera inside the volume updates only what lies in front of it; behind the volume looking away, and beside it looking
    past it: nothing at all"""
    K, _, depth, _ = _frames()
    v = _around_the_wall((17, 9, 5))
    cam = tr.camera(K, ROWS, COLS, 0.001, 0.4, 3.0)
    flat = np.full((1, ROWS, COLS), 1.0, F)
    for pose, nothing in ((tc.pose(t=(0.0, 0.0, 2.2)), False), (tc.pose(t=(0.0, 0.0, 3.5)), True), (tc.pose(ry=np.pi, t=(0, 0, 1.0)), True),
                          (tc.pose(ry=np.pi / 2, t=(1.5, 0, 2.2)), True), (tc.pose(ry=-np.pi / 2, t=(1.5, 0, 2.2)), False)):
        planes = tr.new_planes(v)
        want = tr.integrate(planes, v, cam, flat, pose[None], 0.15)
        assert (want["num_voxel_updates"] == 0) == nothing
        t = _volume_of(product, v, cam, 0.15)
        assert t.integrate(flat, pose[None]) == want
        _same_planes(t, planes)
        if not nothing:
            assert not planes[1].all()  # (inside: the voxels behind the camera stay empty)


def test_half_pixels_truncation_ends_and_depth_gate(product):
    # three voxels whose centres project to u + 0.5 = 0 (in: pixel 0), 1 and 2 = cols (out); v + 0.5 = 0
    v = tr.volume(3, 1, 1, 1.0, (0.0, 0.0, 0.5))
    cam = tr.camera(np.array([[1, 0, -1], [0, 1, -1], [0, 0, 1]], F), 1, 2, 0.001, 0.1, 5.0)
    planes = tr.new_planes(v)
    depth = np.full((1, 1, 2), 1.0, F)
    want = tr.integrate(planes, v, cam, depth, tc.pose()[None], 0.5)
    assert planes[1].reshape(-1).tolist() == [1, 1, 0] and want["num_voxel_updates"] == 2
    t = _volume_of(product, v, cam, 0.5)
    assert t.integrate(depth, tc.pose()[None]) == want
    _same_planes(t, planes)
    # one voxel at camera depth 1: s = -mu, just below, = mu, beyond; q = -+32767; depths exactly at depth_min / depth_max and beside
    v = tr.volume(1, 1, 1, 0.5, (-0.25, -0.25, 0.75))
    K = np.array([[10, 0, 1], [0, 10, 1], [0, 0, 1]], F)
    for d, dmin, dmax, q in ((0.75, 0.1, 2.0, -32767), (np.nextafter(F(0.75), F(0)), 0.1, 2.0, None), (1.25, 0.1, 2.0, 32767),
                             (1.9, 0.1, 2.0, 32767), (1.0, 0.1, 2.0, 0), (1.25, 1.25, 2.0, 32767), (1.25, 0.1, 1.25, 32767),
                             (1.25, 1.2500001, 2.0, None), (1.25, 0.1, 1.2499999, None)):
        cam = tr.camera(K, 3, 3, 0.001, dmin, dmax)
        planes = tr.new_planes(v)
        depth = np.full((1, 3, 3), d, F)
        want = tr.integrate(planes, v, cam, depth, tc.pose()[None], 0.25)
        assert (int(planes[0][0, 0, 0]), int(planes[1][0, 0, 0])) == ((q, 1) if q is not None else (0, 0)), (d, dmin, dmax)
        t = _volume_of(product, v, cam, 0.25)
        assert t.integrate(depth, tc.pose()[None]) == want, (d, dmin, dmax)
        _same_planes(t, planes, str((d, dmin, dmax)))


def _device_stack(images, pad):
    """(tensor kept alive, (pointer, image type, row stride)): K images one behind the other, rows padded by `pad` bytes"""
    import torch

    k, rows, cols = images.shape
    row_bytes = cols * images.itemsize
    buf = np.zeros((k * rows, row_bytes + pad), np.uint8)
    buf[:, :row_bytes] = np.ascontiguousarray(images).view(np.uint8).reshape(k * rows, row_bytes)
    ten = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    kind = {1: abi.IMAGE_U8, 2: abi.IMAGE_U16, 4: abi.IMAGE_F32}[images.itemsize]
    return ten, (ten.data_ptr(), kind, row_bytes + pad)


def _host_padded(images, pad_elems):
    """a view with padded rows whose frames still lie one behind the other"""
    k, rows, cols = images.shape
    buf = np.zeros((k, rows, cols + pad_elems), images.dtype)
    buf[:, :, :cols] = images
    return buf[:, :, :cols]


@pytest.mark.parametrize("u16", (False, True), ids=("f32", "u16"))
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
def test_image_types_memory_spaces_and_strides(product, u16, device):
    """U16 (zeros = no reading) and F32 (NaN, +-inf, zero, negative), host and device memory, packed and padded rows, with the
    intensity plane (U8 and F32 images)"""
    K, poses, depth, inten = _frames()
    v = _around_the_wall((17, 9, 5), with_intensity=True)
    cam = tr.camera(K, ROWS, COLS, 0.001, 0.4, 3.0)
    d = tc.to_u16(depth) if u16 else depth
    assert (d == 0).any()
    planes = tr.new_planes(v)
    want = tr.integrate(planes, v, cam, d, poses, 0.15, inten)
    assert planes[2].any()
    for pad, inten_f32 in ((0, False), (12, True)):
        i = inten.astype(F) + F(0.25) if inten_f32 else inten
        t = _volume_of(product, v, cam, 0.15)
        if device:
            keep_d, dd = _device_stack(d, pad)
            keep_i, ii = _device_stack(i, pad)
        else:
            dd, ii = _host_padded(d, pad // 4), _host_padded(i, pad // 4)
        assert t.integrate(dd, poses, ii) == want, (pad, inten_f32)
        _same_planes(t, planes, str((pad, inten_f32)))
    _same_raycast(product, t, planes, v, cam, poses[1], 0.07, what="intensity")
    # an intensity image for a volume without the plane, and the other way round
    with pytest.raises(RuntimeError, match="intensity"):
        t.integrate(d, poses)
    _same_planes(t, planes, "after the refusal")
    bare = _volume_of(product, _around_the_wall((17, 9, 5)), cam, 0.15)
    with pytest.raises(RuntimeError, match="intensity"):
        bare.integrate(d, poses, inten)
    assert not bare.planes()[1].any()


def test_one_call_five_calls_reversed_and_queued(product):
    v, cam, poses, depth, planes, want = _reference((17, 9, 5))
    # K = 1
    one = tr.new_planes(v)
    want1 = tr.integrate(one, v, cam, depth[:1], poses[:1], 0.15)
    t = _volume_of(product, v, cam, 0.15)
    assert t.integrate(depth[:1], poses[:1]) == want1
    _same_planes(t, one, "K = 1")
    # ... the other four one by one: the five calls make what one call of five makes
    parts = [want1] + [t.integrate(depth[k:k + 1], poses[k:k + 1]) for k in range(1, 5)]
    _same_planes(t, planes, "five calls")
    for key in want:
        assert want[key] == sum(p[key] for p in parts), key
    # reversed
    t = _volume_of(product, v, cam, 0.15)
    assert t.integrate(depth[::-1].copy(), poses[::-1].copy()) == want
    _same_planes(t, planes, "reversed")
    # queued (out == NULL), then a call that waits
    t = _volume_of(product, v, cam, 0.15)
    assert t.integrate(depth[:3], poses[:3], want_result=False) is None
    assert t.integrate(depth[3:], poses[3:], want_result=False) is None
    _same_planes(t, planes, "queued")
    # zero frames do nothing
    assert t.integrate(depth[:0], poses[:0]) == {"num_frames": 0, "num_pixels": 0, "num_valid_depth": 0, "num_voxel_updates": 0}
    _same_planes(t, planes, "zero frames")


def test_take_out_and_put_back_at_another_pose(product):
    v, cam, poses, depth, planes, want = _reference((17, 9, 5))
    t = _volume_of(product, v, cam, 0.15)
    t.integrate(depth, poses)
    assert t.remove(depth[1:3], poses[1:3])["num_voxel_updates"] > 0
    moved = poses.copy()
    moved[1:3] = np.stack([tc.pose(0.02, -0.04, 0.01, (0.05, 0.02, -0.03)), tc.pose(-0.03, 0.05, 0.0, (-0.04, 0.0, 0.06))])
    t.integrate(depth[1:3], moved[1:3])
    other = tr.new_planes(v)
    tr.integrate(other, v, cam, depth, moved, 0.15)
    assert not np.array_equal(other[0], planes[0])
    _same_planes(t, other, "re-integrated")
    # everything out: zeros, bit for bit
    assert t.remove(depth, moved) == tr.integrate(other, v, cam, depth, moved, 0.15, weight=-1)
    assert not any(p.any() for p in t.planes()[:2])


def test_raycast_gap_behind_min_weight_and_long_steps(product):
    """walls seen from the front at z = 2.0 and at 1.2 and from the back at 2.05: with min_weight = 2 a ray from the front passes
    valid positive samples, a gap of invalid ones, then valid negative ones -- no surface; with min_weight = 1 it has one"""
    rows, cols = 12, 16
    K = tc.intrinsics(rows, cols, 20.0)
    v = tr.volume(20, 16, 30, 0.05, (-0.5, -0.4, 1.0))
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 4.0)
    front, back = tc.pose(), tc.pose(ry=np.pi, t=(0, 0, 4.0))
    poses = np.stack([front, front, back])
    depth = np.stack([np.full((rows, cols), d, F) for d in (2.0, 1.2, 1.95)])
    planes = tr.new_planes(v)
    tr.integrate(planes, v, cam, depth, poses, 0.1)
    t = _volume_of(product, v, cam, 0.1)
    t.integrate(depth, poses)
    _same_planes(t, planes)
    valid2 = planes[1] >= 2
    assert (planes[0][valid2] > 0).any() and (planes[0][valid2] < 0).any()
    assert not _same_raycast(product, t, planes, v, cam, front, 0.05, 2, "gap").any()
    assert _same_raycast(product, t, planes, v, cam, front, 0.05, 1, "no gap").any()
    assert not _same_raycast(product, t, planes, v, cam, front, 0.05, 4, "min_weight above the weights").any()
    # the front walls entered from behind: F rises along the ray
    only_front = tr.new_planes(v)
    tr.integrate(only_front, v, cam, depth[:1], poses[:1], 0.1)
    t2 = _volume_of(product, v, cam, 0.1)
    t2.integrate(depth[:1], poses[:1])
    assert not _same_raycast(product, t2, only_front, v, cam, back, 0.05, 1, "from behind").any()
    # steps of 2.6 voxels, from a tilted pose
    _same_raycast(product, t2, only_front, v, cam, tc.pose(0.1, 0.2, -0.05, (0.1, 0.0, 0.2)), 0.13, 1, "long steps")
    # no samples at all: depth_max below depth_min
    t2.camera.depth_max = 0.3
    image, res = t2.raycast(front)
    assert not image.any() and res["num_surface"] == 0


def test_raycast_through_a_single_valid_block(product):
    """two pixels of depth, a volume one mask block deep: the valid voxels lie in ONE 8 x 8 x 8 block of 27"""
    rows, cols = 12, 16
    K = tc.intrinsics(rows, cols, 40.0)
    v = tr.volume(24, 24, 8, 0.05, (-0.6, -0.6, 1.8))
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 4.0)
    depth = np.full((1, rows, cols), np.nan, F)
    depth[0, 5:7, 7:9] = 2.0
    planes = tr.new_planes(v)
    tr.integrate(planes, v, cam, depth, tc.pose()[None], 0.1)
    assert tr.block_mask(planes[1], 1).sum() == 1 and planes[1].sum() > 8
    t = _volume_of(product, v, cam, 0.1)
    t.integrate(depth, tc.pose()[None])
    _same_planes(t, planes)
    _same_raycast(product, t, planes, v, cam, tc.pose(), 0.025, 1, "one block")
    _same_export(product, t, planes, v, 1, "one block")


def test_past_the_launch_caps(product):
    """the grid-stride kernels (depth count, block mask, export flags and scatter) run 2048 workgroups at most: two 640 x 480
    frames (614 400 pixels) into 128 x 64 x 65 voxels (532 480 voxels, 1 597 440 export entries) cross every cap"""
    rows, cols = 480, 640
    K, poses, depth = tc.room_frames(2, rows, cols, 31)
    v = _around_the_wall((128, 64, 65), vs=0.03)
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 4.0)
    planes = tr.new_planes(v)
    want = tr.integrate(planes, v, cam, depth, poses, 0.09)
    assert want["num_valid_depth"] == 2 * rows * cols
    t = _volume_of(product, v, cam, 0.09)
    assert t.integrate(depth, poses) == want
    _same_planes(t, planes)
    assert _same_export(product, t, planes, v, 1) > 5000
    small = tr.camera(tc.intrinsics(30, 40), 30, 40, 0.001, 0.4, 4.0)
    t.set_camera(small["K"], 30, 40, 0.001, 0.4, 4.0)
    assert _same_raycast(product, t, planes, v, small, poses[0], 0.03, 1, "large volume").any()


def test_refusals_leave_planes_and_destinations_unchanged(product):
    v, cam, poses, depth, planes, want = _reference((17, 9, 5))
    t = _volume_of(product, v, cam, 0.15)
    t.integrate(depth, poses)
    scene = mapping.Scene(product.scene_binding(0), 3)
    t.raycast(poses[0], scene)
    before = (scene.size(), scene.get()[0].tobytes())
    lib = t._lib
    dptr, pptr = C.c_void_p(depth.ctypes.data), C.c_void_p(poses.ctypes.data)

    def integrate(depth_type=abi.IMAGE_F32, stride=4 * COLS, k=5, weight=1, cam_=None, fp=None, pose_ptr=pptr, h=t._h, d=dptr):
        out = abi.TsdfResult()
        out.num_frames = -7
        rc = lib.srrg2_tsdf_integrate_frames(h, d, depth_type, stride, None, abi.IMAGE_NONE, 0, k, pose_ptr, abi.MEM_HOST,
                                             C.byref(cam_ if cam_ is not None else t.camera), C.byref(fp if fp is not None else t.frame),
                                             weight, C.byref(out))
        assert rc == 0 or out.num_frames == -7
        return rc

    def cam_with(**kw):
        c = abi.DepthAdaptorParams.from_buffer_copy(t.camera)
        for k_, val in kw.items():
            if k_ == "K":
                c.camera_matrix[val[0]] = val[1]
            else:
                setattr(c, k_, val)
        return c

    def fp_with(mu):
        f = abi.TsdfFrameParams()
        f.mu = mu
        return f

    bad_pose = poses.copy()
    bad_pose[2, 1, 3] = np.inf
    for rc, code in ((integrate(weight=2), E_INVALID), (integrate(weight=0), E_INVALID), (integrate(k=-1), E_INVALID),
                     (integrate(depth_type=abi.IMAGE_U8), E_INVALID), (integrate(stride=4 * COLS - 4), E_INVALID),
                     (integrate(stride=4 * COLS + 2), E_INVALID), (integrate(d=None), E_INVALID), (integrate(pose_ptr=None), E_INVALID),
                     (integrate(pose_ptr=C.c_void_p(bad_pose.ctypes.data)), E_INVALID), (integrate(h=None), E_INVALID),
                     (integrate(fp=fp_with(0.0)), E_INVALID), (integrate(fp=fp_with(float("nan"))), E_INVALID),
                     (integrate(cam_=cam_with(K=(0, 0.0))), E_INVALID), (integrate(cam_=cam_with(rows=-1)), E_INVALID),
                     (integrate(cam_=cam_with(K=(1, 0.5))), E_UNSUPPORTED)):
        assert rc == code
    _same_planes(t, planes, "after the refused integrations")
    fresh = product.TsdfVolume(0)  # (a handle before its reset)
    assert integrate(h=fresh._h) == E_INVALID
    # raycast and export
    for field, value in (("step", 0.0), ("step", float("inf")), ("min_weight", 0), ("skip_empty", 2)):
        old = getattr(t.ray, field)
        setattr(t.ray, field, value)
        with pytest.raises(RuntimeError, match="code -1"):
            t.raycast(poses[0], scene)
        setattr(t.ray, field, old)
    flat = mapping.Scene(product.scene_binding(0), 2)
    with pytest.raises(RuntimeError, match="code -1"):
        t.raycast(poses[0], flat)
    with pytest.raises(RuntimeError, match="code -1"):
        t.to_scene(flat)
    with pytest.raises(RuntimeError, match="code -1"):
        t.to_scene(scene, 0)
    with pytest.raises(RuntimeError, match="code -1"):
        t.raycast(bad_pose[2], scene)
    assert (scene.size(), scene.get()[0].tobytes()) == before
    for bad in (dict(nx=-1), dict(nz=2049), dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(origin=(0.0, float("inf"), 0.0))):
        args = dict(nx=4, ny=4, nz=4, voxel_size=0.1, origin=(0.0, 0.0, 0.0))
        args.update(bad)
        with pytest.raises(RuntimeError, match="code -1"):
            t.reset(**args)
    _same_planes(t, planes, "after the refused resets")
    assert t.integrate(depth, poses) == want  # the same call without a mistake goes through


def test_frame_to_model_tracking_against_the_raycast(product):
    """six frames of the box room fused; the volume ray-cast from a pose 3 cm and 2 degrees off a seventh frame's; that frame
    aligned against the raycast scene with the projective point-to-plane slice ends nearer to the truth than it started"""
    rows, cols = 120, 160
    K, poses, depth = tc.room_frames(7, rows, cols, 41)
    origin, vs = (-1.1, -0.9, -0.3), 0.04
    v = tr.volume(55, 45, 65, vs, origin)
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 4.0)
    t = _volume_of(product, v, cam, 0.12)
    out = t.integrate(depth[:6], poses[:6])
    assert out["num_valid_depth"] == 6 * rows * cols and out["num_voxel_updates"] > 100000
    truth = poses[6].astype(np.float64)
    off = tc.pose(0.02, -0.025, 0.015, (0.02, -0.015, 0.02)).astype(np.float64)
    guess = np.zeros((3, 4))
    guess[:, :3], guess[:, 3] = truth[:, :3] @ off[:, :3], truth[:, 3] + off[:, 3]
    t.ray.step = vs
    model = mapping.Scene(product.scene_binding(0), 3)
    image, res = t.raycast(guess.astype(F), model)
    assert res["num_surface"] > 0.8 * rows * cols and res["adapt"]["num_valid"] > 0.5 * rows * cols
    fixed, fixed_n = model.get()
    r = ar.adapt_depth_image(depth[6], K, 0.001, 0.4, 4.0, compact=True)
    # truth: the seventh camera in the raycast camera's frame
    Rg, tg = guess[:, :3].astype(F).astype(np.float64), guess[:, 3].astype(F).astype(np.float64)
    X_gt = np.zeros((3, 4))
    X_gt[:, :3], X_gt[:, 3] = Rg.T @ truth[:, :3], Rg.T @ (truth[:, 3] - tg)
    data = {"K": K, "rows": rows, "cols": cols, "depth_min": 0.4, "depth_max": 4.0}
    al = product.MultiAligner(abi.SE3_QUAT_RIGHT, device=0)
    si = al.add_slice(projective_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, data, gate=0.15))
    al.set_fixed(si, fixed, fixed_n)
    al.set_moving(si, r["points"], r["normals"])
    start = np.eye(3, 4, dtype=F)
    al.set_moving_in_fixed(start)
    al.compute()
    assert al.status() == abi.SUCCESS

    def errors(X):
        X = np.asarray(X, np.float64).reshape(3, 4)
        dR = X[:, :3].T @ X_gt[:, :3]
        return float(np.linalg.norm(X[:, 3] - X_gt[:, 3])), float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))

    t0, r0 = errors(start)
    t1, r1 = errors(al.moving_in_fixed())
    print("frame-to-model: translation %.4f -> %.4f m, rotation %.3f -> %.3f deg" % (t0, t1, r0, r1))
    assert t1 < t0 and r1 < r0
