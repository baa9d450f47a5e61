"""CPU: the vectorised restatement of the TSDF volume (tests/tsdf_restatement.py) against the contract written out as a plain
per-frame, per-voxel loop, and the contract's own properties: a batch taken out restores zeros, order and split do not matter,
the counters add up, the block mask changes no bit of a raycast, and a wall at a known depth ray-casts to that depth."""
import numpy as np

import tsdf_cases as tc
import tsdf_restatement as tr

F = np.float32


def _small(with_intensity, seed=5, u16=False):
    """9 x 7 x 5 voxels in front of four frames of the room, the frustum cutting the volume on every side"""
    rows, cols = 20, 26
    K, poses, depth = tc.room_frames(4, rows, cols, seed, focal=60.0)
    v = tr.volume(9, 7, 5, 0.11, (-0.5, -0.35, 1.75), with_intensity)
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 3.0)
    depth = tc.spoiled(depth, seed + 1)
    inten = tc.intensity_like(depth, seed + 2) if with_intensity else None
    return v, cam, poses, (tc.to_u16(depth) if u16 else depth), inten


def test_vectorised_restatement_equals_the_plain_loop():
    for with_intensity, u16 in ((False, False), (True, True)):
        v, cam, poses, depth, inten = _small(with_intensity, u16=u16)
        a, b = tr.new_planes(v), tr.new_planes(v)
        out = tr.integrate(a, v, cam, depth, poses, 0.03, inten)
        updates = tr.integrate_loop(b, v, cam, depth, poses, 0.03, inten)
        assert out["num_voxel_updates"] == updates > 50
        assert updates < 4 * 9 * 7 * 5  # (the frustum and the truncation leave voxels out)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert a[1].max() == 4 and a[1].min() == 0
        # F32 intensity restates as the U8 image it rounds to
        if with_intensity:
            c = tr.new_planes(v)
            tr.integrate(c, v, cam, depth, poses, 0.03, inten.astype(F) + F(0.25))
            assert np.array_equal(c[2], a[2])


def test_take_out_restores_zeros_and_order_and_split_do_not_matter():
    v, cam, poses, depth, inten = _small(True)
    planes = tr.new_planes(v)
    whole = tr.integrate(planes, v, cam, depth, poses, 0.03, inten)
    assert whole["num_frames"] == 4 and whole["num_pixels"] == 4 * 20 * 26
    assert 0 < whole["num_valid_depth"] < whole["num_pixels"]
    assert planes[1].sum() == whole["num_voxel_updates"]
    # any permutation, any split
    for order in ((3, 2, 1, 0), (2, 0, 3, 1)):
        other = tr.new_planes(v)
        o = list(order)
        tr.integrate(other, v, cam, depth[o], poses[o], 0.03, inten[o])
        assert all(np.array_equal(x, y) for x, y in zip(planes, other))
    split, parts = tr.new_planes(v), []
    for sl in (slice(0, 1), slice(1, 3), slice(3, 4)):
        parts.append(tr.integrate(split, v, cam, depth[sl], poses[sl], 0.03, inten[sl]))
    assert all(np.array_equal(x, y) for x, y in zip(planes, split))
    for key in whole:
        assert whole[key] == sum(p[key] for p in parts), key
    # +1 then -1
    back = tr.integrate(planes, v, cam, depth, poses, 0.03, inten, weight=-1)
    assert back == whole and not any(p.any() for p in planes)


def test_edges_of_the_truncation_and_of_the_depth_gate():
    """one voxel on the optical axis at camera depth 1: s exactly -mu, just below it, exactly mu, beyond it; depths exactly at the
    gate's ends; q at +-32767"""
    v = tr.volume(1, 1, 1, 0.5, (-0.25, -0.25, 0.75))
    K = np.array([[10, 0, 1], [0, 10, 1], [0, 0, 1]], F)
    T = tc.pose()[None]
    mu = F(0.25)
    for d, dmin, dmax, want in ((0.75, 0.1, 2.0, (-32767, 1)), (np.nextafter(F(0.75), F(0)), 0.1, 2.0, (0, 0)), (1.25, 0.1, 2.0, (32767, 1)),
                                (1.9, 0.1, 2.0, (32767, 1)), (1.0, 0.1, 2.0, (0, 1)), (1.25, 1.25, 2.0, (32767, 1)), (1.25, 0.1, 1.25, (32767, 1)),
                                (1.25, 1.2500001, 2.0, (0, 0)), (1.25, 0.1, 1.2499999, (0, 0))):
        planes = tr.new_planes(v)
        cam = tr.camera(K, 3, 3, 0.001, dmin, dmax)
        tr.integrate(planes, v, cam, np.full((1, 3, 3), d, F), T, mu)
        assert (int(planes[0][0, 0, 0]), int(planes[1][0, 0, 0])) == want, (d, dmin, dmax)
    # the same voxel from a camera behind it looking away, and from inside it: c.z <= 0 adds nothing
    for pose_ in (tc.pose(ry=np.pi), tc.pose(t=(0, 0, 1.0)), tc.pose(t=(0, 0, 1.3))):
        planes = tr.new_planes(v)
        out = tr.integrate(planes, v, tr.camera(K, 3, 3, 0.001, 0.1, 2.0), np.full((1, 3, 3), 1.0, F), pose_[None], mu)
        assert out["num_voxel_updates"] == 0 and not planes[1].any()


def test_a_wall_raycasts_to_its_depth():
    vol, K, rows, cols, poses, depth, wall, mu = tc.wall_case()
    v = tr.volume(**vol)
    cam = tr.camera(K, rows, cols, 0.001, 0.4, 3.0)
    planes = tr.new_planes(v)
    tr.integrate(planes, v, cam, depth, poses, mu)
    step = float(v["vs"])  # step <= voxel_size: the crossing is bracketed by two samples one voxel apart at most
    for min_weight in (1, 3):
        image, _ = tr.raycast(planes, v, cam, poses[0], step, min_weight)
        got = image != 0
        centre = got[rows // 4:-(rows // 4), cols // 4:-(cols // 4)]
        assert centre.mean() > 0.5, (min_weight, centre.mean())
        assert np.abs(image[got] - F(wall)).max() <= float(v["vs"]), np.abs(image[got] - F(wall)).max()
        skipped, _ = tr.raycast(planes, v, cam, poses[0], step, min_weight, skip_empty=True)
        assert tr.same_bits(image, skipped)
    # nothing is seen from behind the wall (F rises along the ray: no crossing from + to -), nor with min_weight above the weights
    behind, _ = tr.raycast(planes, v, cam, tc.pose(ry=np.pi, t=(0, 0, 2.6)), step, 1)
    assert not behind.any()
    none, _ = tr.raycast(planes, v, cam, poses[0], step, 4)
    assert not none.any()
    # the export puts its points on the wall, with normals along -z (F falls with z)
    pts, nrm, idx = tr.to_scene(planes, v, 3)
    assert len(idx) > 50 and np.all(idx % 3 == 2)
    assert np.abs(pts[:, 2] - F(wall)).max() <= float(v["vs"])
    has = ~np.isnan(nrm[:, 0])
    assert has.any() and (~has).any() and np.all(nrm[has, 2] < -0.99)


def test_export_zero_on_a_voxel_and_missing_neighbours():
    v = tr.volume(3, 3, 3, 1.0, (0.0, 0.0, 0.0))
    planes = tr.new_planes(v)
    planes[1][:] = 2
    planes[0][:, :, 0], planes[0][:, :, 1], planes[0][:, :, 2] = 8, 0, -8  # F = 4, 0, -4 along x: the zero lies ON voxel x = 1
    pts, nrm, idx = tr.to_scene(planes, v, 1)
    assert len(idx) == 18 and np.all(idx % 3 == 0)  # every x edge, both the one that ends in the zero and the one that starts there
    assert np.all(pts[:, 0] == F(1.5))
    centre = idx == 3 * 13 + 0  # voxel (1, 1, 1): the only one with all six neighbours
    assert centre.sum() == 1 and np.array_equal(nrm[centre][0], np.array([-1, 0, 0], F))
    assert np.isnan(nrm[~centre]).all()
    planes[1][1, 1, 2] = 0  # a neighbour of (1, 1, 1) goes missing: its edge and the normal go with it
    pts2, nrm2, idx2 = tr.to_scene(planes, v, 1)
    assert len(idx2) == 17 and np.isnan(nrm2).all()
    assert tr.to_scene(tr.new_planes(v), v, 1)[2].size == 0
