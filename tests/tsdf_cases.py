"""Seeded cases for the TSDF volume tests: a box room rendered analytically into depth frames, a fronto-parallel wall, poses
around them, and the small volumes at which the kernels can go wrong.  Shared by tests/test_tsdf_restatement.py (CPU) and
tests/test_gpu_tsdf.py; nothing here knows the library."""
import numpy as np

F = np.float32

# nx, ny, nz: sides that are no multiple of the 64-voxel run or the 8-voxel mask block, one voxel, a run and one voxel, empty
VOLUMES = ((17, 9, 5), (65, 3, 2), (1, 1, 1), (0, 4, 4), (9, 7, 5), (70, 11, 9))
ROOM_LO, ROOM_HI = np.array([-1.0, -0.8, -0.2]), np.array([1.0, 0.8, 2.2])


def intrinsics(rows, cols, focal=None):
    f = float(focal if focal is not None else 0.9 * cols)
    return np.array([[f, 0, (cols - 1) / 2.0], [0, f, (rows - 1) / 2.0], [0, 0, 1]], F)


def pose(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    """camera_in_world (3, 4) float32: R = Rz Ry Rx (float64, rounded once), the camera looks along its +z"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = Rz @ Ry @ Rx, t
    return T.astype(F)


def render_room(T, K, rows, cols, lo=ROOM_LO, hi=ROOM_HI):
    """(rows, cols) float32: the camera depth (z along the optical axis) at which every pixel's ray leaves the box [lo, hi] that
    the camera stands in, float64 throughout and rounded once"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    K = np.asarray(K, np.float64).reshape(3, 3)
    c, r = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    d = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], -1) @ T[:, :3].T
    o = T[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    return t.min(-1).astype(F)


def room_trajectory(n, seed):
    """n poses inside the room, near its front, looking roughly along +z with a few degrees and centimetres of motion"""
    rng = np.random.default_rng(seed)
    return np.stack([pose(*(0.12 * rng.uniform(-1, 1, 3)), t=0.15 * rng.uniform(-1, 1, 3)) for _ in range(n)])


def room_frames(n, rows, cols, seed, focal=None):
    """(K, poses (n, 3, 4), depth (n, rows, cols) float32)"""
    K = intrinsics(rows, cols, focal)
    poses = room_trajectory(n, seed)
    return K, poses, np.stack([render_room(T, K, rows, cols) for T in poses])


def to_u16(depth, scale=0.001):
    """millimetre counts of a float depth image (0 where it is not finite)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(depth), np.rint(depth / scale), 0).clip(0, 65535).astype(np.uint16)


def room_volume(n=(32, 28, 24), voxel=0.05):
    """(origin, voxel_size): a volume of n voxels around the room's far wall and the corners beside it"""
    return (float(-0.5 * n[0] * voxel), float(-0.5 * n[1] * voxel), float(ROOM_HI[2] + 0.2 - n[2] * voxel)), voxel


def spoiled(depth, seed):
    """a float32 depth stack with NaN, +inf, -inf, zeros and negative readings sprinkled in"""
    rng = np.random.default_rng(seed)
    d = depth.copy()
    for value in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        d[rng.random(d.shape) < 0.02] = value
    return d


def intensity_like(depth, seed):
    """a uint8 image stack the shape of `depth`: a gradient plus noise"""
    rng = np.random.default_rng(seed)
    k, rows, cols = depth.shape
    base = (np.arange(cols)[None, None, :] * 3 + np.arange(rows)[None, :, None] * 5 + np.arange(k)[:, None, None] * 11) % 200
    return (base + rng.integers(0, 56, depth.shape)).astype(np.uint8)


def wall_case():
    """a fronto-parallel wall at world z = 1.4 seen from three poses that differ in translation only: (volume args, K, rows,
    cols, poses, depth images, wall z, mu).  The depth of every pixel of pose k is 1.4 - t_z exactly."""
    rows, cols, wall = 24, 32, 1.4
    K = np.array([[30, 0, 15.5], [0, 30, 11.5], [0, 0, 1]], F)
    poses = np.stack([pose(t=(0.0, 0.0, 0.0)), pose(t=(0.1, -0.05, 0.1)), pose(t=(-0.08, 0.04, -0.15))])
    depth = np.stack([np.full((rows, cols), wall - float(T[2, 3]), F) for T in poses])
    vol = dict(nx=24, ny=20, nz=16, voxel_size=0.05, origin=(-0.6, -0.5, 1.0))
    return vol, K, rows, cols, poses, depth, wall, 0.15
