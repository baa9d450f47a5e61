"""-m gpu: handles release what they allocate (create / use / destroy in a loop leaves the device memory level where it
was), and several handles live side by side."""
import numpy as np
import pytest

import consensus_cases as cc
import features_cases as fc
import stereo_cases as sc
from helpers import cue_config, setup_pair
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import adaptors, mapping
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def _free_bytes():
    """hipMemGetInfo of the HIP runtime the product library itself is linked against"""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    assert hip.hipDeviceSynchronize() == 0
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_no_device_memory_leak(product):
    d = syn.cloud_pair_3d(n=50_000, seed=31)
    g = syn.pose_graph_3d(V=2000, E=6000, seed=32)

    def cycle():
        al = product.MultiAligner(abi.SE3_QUAT_RIGHT)
        setup_pair(al, d, cue_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05))
        al.compute()
        al.correspondences(0)
        b = product.scene_binding(0)
        s1, s2 = mapping.Scene(b, 3), mapping.Scene(b, 3)
        s1.set(d["fixed"], d["fixed_normals"])
        cl = mapping.SceneClipperBall(b, 5.0)
        cl.set_full_scene(s1); cl.set_clipped_scene_in_robot(s2); cl.set_robot_in_local_map(syn.identity(3))
        cl.compute()
        pg = product.PoseGraph(abi.SE3_QUAT_RIGHT, 0)
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
        pg.solve()
        for h in (al, s1, s2, pg):
            h.close()

    for _ in range(3):
        cycle()  # allocator warm-up
    before = _free_bytes()
    for _ in range(25):
        cycle()
    after = _free_bytes()
    assert before - after < 8 << 20, (before, after)  # nothing accumulates (the clouds alone are ~10 MB per cycle)


def _sweep_points(n, seed):
    """n returns of a spinning lidar: every azimuth, elevations inside the +-0.4 rad of the model below, 2 .. 60 m"""
    rng = np.random.default_rng(seed)
    az, el, r = rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.38, 0.38, n), rng.uniform(2.0, 60.0, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], -1).astype(np.float32)


def _descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def test_no_device_memory_leak_scene_entry_points(product):
    """one of every handle family per cycle.  Three cases are sized so that a scratch buffer nobody frees shows: the sweep's
    range image (64 x 2048 pixels x 8 bytes = 1 MiB), its de-skewed points (131 072 x 16 bytes = 2 MiB) and the occluding
    spherical clip's staged pixels (131 072 x 8 bytes = 1 MiB) -- 4 MiB per cycle, 100 MiB over the 25 cycles, against the
    8 MiB bound.  The others run on the smallest shapes of their own tests."""
    rows, cols, n = 64, 2048, 131_072
    P = _sweep_points(n, 71)
    motion = syn.se3(np.array([0.3, -0.1, 0.02]), np.deg2rad([0.5, -0.3, 2.0]))[:3]
    img, depth = fc.image(120, 160), fc.depth_for(fc.image(120, 160), "u16")
    left, right = sc.named("120x160")[:2]
    rng = np.random.default_rng(72)
    D1, D2 = _descriptors(rng, 300), _descriptors(rng, 2000)  # (the second add passes the 1024-element floor: grow and keep)
    c = cc.basic(3)
    b = product.scene_binding(0)

    def cycle():
        scenes = [mapping.Scene(b, 3) for _ in range(8)]
        sweep, full, clipped, vox, feat, stereo, landmarks, view = scenes
        # a de-skewed lidar sweep (srrg2_adapt_lidar_sweep_ex)
        ad = adaptors.MeasurementAdaptorLidarSweep()
        adaptors.spherical_model_full_turn(rows, cols, -0.4, 0.4, model=ad.params.model)
        ad.set_meas(sweep)
        ad.set_motion(motion)
        ad.set_raw_data(P)
        ad.compute()
        assert sweep.size() > 0
        # the spherical clip with occlusion, then voxels and normals of what it kept
        full.set(P)
        cl = mapping.SceneClipperSpherical(b)
        adaptors.spherical_model_full_turn(rows, cols, -0.4, 0.4, model=cl.params.model)
        cl.params.occlusion_margin = 0.1
        cl.set_full_scene(full); cl.set_clipped_scene_in_robot(clipped); cl.set_robot_in_local_map(syn.identity(3))
        cl.compute()
        assert clipped.size() > n // 4
        clipped.voxelize(vox, 0.5)
        clipped.estimate_normals(1.0)
        # image features, stereo features
        fa = adaptors.MeasurementAdaptorImageFeatures()
        fa.set_camera_matrix(fc.CAMERA)
        fa.params.max_features = 0
        fa.set_meas(feat)
        fa.set_raw_data(img, depth)
        fa.compute()
        sa = adaptors.MeasurementAdaptorStereoFeatures()
        sa.set_camera_matrix(sc.CAMERA)
        sa.stereo.baseline = sc.BASELINE
        sa.params.max_features = 0
        sa.set_meas(stereo)
        sa.set_raw_data(left, right)
        sa.compute()
        # the tracker: the image's own keypoints as landmarks, seen from where they were taken
        assert feat.size() >= 30
        landmarks.set(feat.get()[0])
        landmarks.set_features(*feat.features())
        ball = mapping.SceneClipperBall(b, 100.0)
        ball.set_full_scene(landmarks); ball.set_clipped_scene_in_robot(view); ball.set_robot_in_local_map(syn.identity(3))
        ball.compute()
        tp = mapping.default_track_params()
        for i, v in enumerate(fc.CAMERA):
            tp.camera_matrix[i] = v
        tp.image_rows, tp.image_cols = 120, 160
        ft = mapping.FeatureTracker(b, tp)
        ft.set_fixed(feat); ft.set_moving(view); ft.set_moving_in_sensor(syn.identity(3))
        assert len(ft.compute()) > 0
        # descriptor database, consensus verifier
        db = product.DescriptorDatabase(0)
        db.add(D1); db.add(D2)
        assert 0 in db.match(D1, max_distance=25.0).indices
        cv = product.ConsensusVerifier(3)
        cv.compute(c["fixed"], c["movings"], c["corrs"], **c["params"])
        for h in scenes + [db, cv]:
            h.close()

    for _ in range(3):
        cycle()  # allocator warm-up
    before = _free_bytes()
    for _ in range(25):
        cycle()
    after = _free_bytes()
    print("before - after = %d bytes" % (before - after))
    assert before - after < 8 << 20, (before, after)


def test_grown_buffers_keep_their_head(product):
    """the three buffers that grow under live content keep it, bit for bit: a scene appended into past its capacity, a descriptor
    database across its doubling, a pose graph's arrays under appended leaves.  (tests/test_gpu_posegraph_append.py::
    test_growing_from_the_first_pose reads the poses back against its mirror after every append; this one compares the solve.)"""
    rng = np.random.default_rng(81)
    b = product.scene_binding(0)
    # scene: 1000 points set (room for < 3000), 5000 appended by a merge without correspondences
    n0, n1 = 1000, 5000

    def cloud(n):
        N = rng.normal(size=(n, 3))
        return rng.uniform(-5, 5, (n, 3)).astype(np.float32), (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)

    (P0, N0), (P1, N1) = cloud(n0), cloud(n1)
    d0, i0 = _descriptors(rng, n0), rng.uniform(0, 1, n0).astype(np.float32)
    scene, meas = mapping.Scene(b, 3), mapping.Scene(b, 3)
    scene.set(P0, N0); scene.set_features(d0, i0)
    meas.set(P1, N1); meas.set_features(_descriptors(rng, n1), rng.uniform(0, 1, n1).astype(np.float32))
    head = (scene.get(), scene.features())
    mg = mapping.MergerCorrespondenceHomo(b)
    mg.set_scene(scene); mg.set_measurement(meas); mg.set_measurement_in_scene(syn.identity(3))
    mg.set_correspondences(np.zeros(0, mapping.CORR_DTYPE))
    mg.compute()
    assert scene.size() == n0 + n1
    (pts, nrm), (desc, inten) = scene.get(), scene.features()
    assert pts[:n0].tobytes() == head[0][0].tobytes() == P0.tobytes() and nrm[:n0].tobytes() == head[0][1].tobytes()
    assert desc[:n0].tobytes() == d0.tobytes() and inten[:n0].tobytes() == i0.tobytes()
    scene.close(); meas.close()
    # descriptor database: the first map fits the first 1024-element block, the second add doubles past it
    D1, D2 = _descriptors(rng, 300), _descriptors(rng, 2000)
    Q = D1.copy()
    Q[::3, 0] ^= 0x15  # (a few bits off: distances 0 and 3)
    db = product.DescriptorDatabase(0)
    assert db.add(D1) == 0
    first = db.match(Q, max_distance=25.0)
    assert db.add(D2) == 1
    again = db.match(Q, max_distance=25.0)
    assert list(first.indices) == [0] and first.num_matches[0] >= 300
    k = list(again.indices).index(0)
    assert again.num_matches[k] == first.num_matches[0] and again.map_counts[0] == first.map_counts[0]
    assert again.correspondences[k].tobytes() == first.correspondences[0].tobytes()
    db.close()
    # pose graph: 40 leaves appended to a 20-pose graph whose arrays have room for 23 poses and 49 factors, against a handle
    # whose arrays were first sized by the whole graph
    V0, nl = 20, 40
    g = syn.pose_graph_3d(V=V0, E=45, seed=82)
    leaves = []  # (pose, parent, Z): leaf k hangs off base pose k % V0 through one factor
    for k in range(nl):
        Z = syn.se3(rng.uniform(-0.5, 0.5, 3), rng.uniform(-0.2, 0.2, 3))
        leaves.append((syn.se3_mul(g["poses_init"][k % V0].reshape(3, 4), Z).astype(np.float32), k % V0, Z.astype(np.float32)))

    def solved(presized):
        pg = product.PoseGraph(abi.SE3_QUAT_RIGHT, 0)
        if presized:  # (every array takes its final size first; a later set_graph keeps the room)
            big = syn.pose_graph_3d(V=V0 + nl, E=3 * (V0 + nl), seed=83)
            pg.set_graph(big["poses_init"], big["ij"], big["Z"])
        pg.set_graph(g["poses_init"], g["ij"], g["Z"])
        for k, (pose, parent, Z) in enumerate(leaves):
            assert pg.add_variable(pose) == V0 + k
            pg.add_factor(parent, V0 + k, Z)
        pg.solve()
        out = pg.poses().copy()
        pg.close()
        return out

    grown, full_size = solved(False), solved(True)
    assert grown.shape[0] == V0 + nl and grown.tobytes() == full_size.tobytes()


def test_handles_side_by_side(oracle, product):
    """two aligners with different clouds interleaved: neither disturbs the other's state"""
    d1 = syn.cloud_pair_3d(n=8000, seed=41)
    d2 = syn.cloud_pair_3d(n=12000, seed=42, t=(0.02, 0.04, -0.03))
    cfg = cue_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05)
    a1, a2 = product.MultiAligner(abi.SE3_QUAT_RIGHT), product.MultiAligner(abi.SE3_QUAT_RIGHT)
    setup_pair(a1, d1, cfg)
    setup_pair(a2, d2, cfg)
    a1.compute(); a2.compute()
    X1, X2 = a1.moving_in_fixed().copy(), a2.moving_in_fixed().copy()
    c1 = a1.correspondences(0)
    a2.set_moving_in_fixed(syn.identity(3)); a2.compute()
    assert np.array_equal(a1.correspondences(0), c1) and a1.moving_in_fixed().tobytes() == X1.tobytes()
    a1.set_moving_in_fixed(syn.identity(3)); a1.compute()
    assert a1.moving_in_fixed().tobytes() == X1.tobytes() and a2.moving_in_fixed().tobytes() == X2.tobytes()
    r1 = oracle.OracleAligner(abi.SE3_QUAT_RIGHT)
    setup_pair(r1, d1, cfg)
    r1.compute()
    assert r1.moving_in_fixed().tobytes() == X1.tobytes()


def test_distinct_handles_from_distinct_threads(product):
    """one handle = one non-thread-safe object; distinct handles are usable from distinct threads:
    four threads align concurrently (ctypes releases the GIL), results equal the sequential ones bit for bit."""
    import threading

    cfg = cue_config(abi.SE3_QUAT_RIGHT, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05)
    data = [syn.cloud_pair_3d(n=20000 + 3000 * k, seed=60 + k) for k in range(4)]

    def run(k, out, reps):
        al = product.MultiAligner(abi.SE3_QUAT_RIGHT)
        setup_pair(al, data[k], cfg)
        for _ in range(reps):
            al.set_moving_in_fixed(syn.identity(3))
            al.compute()
        out[k] = (al.moving_in_fixed().copy(), al.correspondences(0).copy(), al.status())
        al.close()

    seq, par = {}, {}
    for k in range(4):
        run(k, seq, 1)
    threads = [threading.Thread(target=run, args=(k, par, 20)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k in range(4):
        assert par[k][2] == seq[k][2] == abi.SUCCESS
        assert par[k][0].tobytes() == seq[k][0].tobytes()
        assert np.array_equal(par[k][1], seq[k][1])
