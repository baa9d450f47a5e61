"""CPU: the numpy restatement of srrg2_scene_voxelize (tests/voxel_restatement.py) against an independent float64 formulation
(np.unique on the cells, the mean per cell), and the exact cases of the contract (DESIGN.md section 4 "Voxel-grid decimation")."""
import numpy as np
import pytest

import voxel_restatement as vr

F = np.float32


def _ulps(a, b):
    """distance in float32 units in the last place between two finite float32 arrays"""
    def ordered(x):
        u = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(ordered(a) - ordered(b))


@pytest.mark.parametrize("leaf", [0.05, 0.25, 1.0, 3.7])
@pytest.mark.parametrize("shift", [0.0, 100.0, 1e4, -3e4])
def test_against_float64_means(shift, leaf):
    """20 k uniform points in +-5 m: the same cells and counts, every centroid within 1 float32 ulp of float32(float64 mean).
    The bound: a point is quantised to within 2^-(e+1) with e >= 44 here -- far below half an ulp of any coordinate; one ulp is
    for the double rounding (float64 sum of fixed-point terms -> float64 -> float32 against float64 mean -> float32)."""
    rng = np.random.default_rng(3)
    n = 20_000
    pts = (rng.uniform(-5, 5, (n, 3)) + shift).astype(F)
    assert vr.exponents(leaf, n)[0] >= 44
    r = vr.voxelize(pts, leaf)
    cells = np.floor(pts.astype(np.float64) / np.float64(F(leaf)))
    uc, first, inv, cnt = np.unique(cells, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(first)  # cells by their first point
    assert r["result"]["num_occupied"] == len(uc) == r["result"]["num_voxels"] and r["result"]["num_finite"] == n
    assert np.array_equal(r["global_indices"], first[order])
    assert np.array_equal(r["counts"], cnt[order])
    assert r["result"]["max_points_per_voxel"] == cnt.max()
    # membership: every point's cell is the cell of the emitted point its cell maps to
    rank = np.empty(len(uc), np.int64)
    rank[order] = np.arange(len(uc))
    assert np.array_equal(cells[r["global_indices"][rank[inv]]], cells)
    mean = np.zeros((len(uc), 3))
    np.add.at(mean, inv, pts.astype(np.float64))
    mean = (mean / cnt[:, None])[order].astype(F)
    worst = int(_ulps(r["points"], mean).max())
    print("shift %g leaf %g: %d cells, worst %d ulp" % (shift, leaf, len(uc), worst))
    assert worst <= 1


def _lattice(m, spacing, dim):
    g = np.arange(m, dtype=np.float64) * spacing
    return np.stack([a.ravel() for a in np.meshgrid(*([g] * dim), indexing="ij")], 1)


@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_whose_spacing_is_the_leaf(dim):
    """origin on the lattice: every point sits on a corner and owns its cell -> the cloud comes back unchanged.  Origin half a
    leaf off: the same.  Two points per axis step (spacing = leaf / 2): 2^dim points per cell, the mean is exact"""
    leaf = 0.25
    for shift in (0.0, 1e4, -3e4):
        pts = (_lattice(6, leaf, dim) - 0.5 + shift).astype(F)
        assert np.array_equal(np.diff(np.unique(pts[:, 0])), np.full(5, F(leaf)))
        for origin in ((0.0, 0.0, 0.0), (0.125, 0.125, 0.125)):
            for mode in (vr.CENTROID, vr.FIRST):
                r = vr.voxelize(pts, leaf, origin=origin, mode=mode)
                assert vr.same_bits(r["points"], pts) and np.array_equal(r["global_indices"], np.arange(len(pts)))
                assert (r["counts"] == 1).all()
    fine = (_lattice(8, leaf / 2, dim)).astype(F)
    r = vr.voxelize(fine, leaf)
    assert len(r["points"]) == 4 ** dim and (r["counts"] == 2 ** dim).all()
    assert np.array_equal(np.unique(r["points"][:, 0]), (np.arange(4) * 0.25 + 0.0625).astype(F))


def test_faces_negative_coordinates_and_minus_zero():
    leaf = 0.5
    pts = np.array([[0.5, 0.0], [0.75, 0.25],     # cell (1, 0): the point ON the face x = 0.5 belongs to the upper cell
                    [0.25, 0.25],                  # cell (0, 0)
                    [-0.0, 0.0],                   # cell (0, 0): -0.0 floors to cell 0
                    [-0.25, 0.0],                  # cell (-1, 0): negative coordinates floor downwards
                    [-0.5, -0.5],                  # cell (-1, -1): on a face again
                    [-0.5000001, -0.5]], F)        # cell (-2, -1)
    r = vr.voxelize(pts, leaf, dim=2)
    assert np.array_equal(r["global_indices"], [0, 2, 4, 5, 6])
    assert np.array_equal(r["counts"], [2, 2, 1, 1, 1])
    assert vr.same_bits(r["points"][0], np.array([0.625, 0.125], F)) and vr.same_bits(r["points"][1], np.array([0.125, 0.125], F))
    assert vr.same_bits(r["points"][2:], pts[4:])  # one point: verbatim
    assert r["result"] == {"num_points": 7, "num_finite": 7, "num_occupied": 5, "num_voxels": 5, "num_with_normal": 0,
                           "max_points_per_voxel": 2}
    # dim 2 ignores z; a non-finite coordinate takes the point out
    p3 = np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 7.0], [np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, np.nan]], F)
    assert vr.voxelize(p3, 1.0, dim=3)["result"]["num_finite"] == 2 and vr.voxelize(p3, 1.0, dim=3)["result"]["num_voxels"] == 2
    r2 = vr.voxelize(p3, 1.0, dim=2)
    assert r2["result"]["num_finite"] == 3 and np.array_equal(r2["counts"], [3])


def test_a_single_point_comes_back_verbatim_whatever_the_fixed_point_would_do():
    p = np.array([[1.0000001, 1e-30, -123456.79]], F)
    for leaf in (1e-3, 0.3, 1e3):
        assert vr.same_bits(vr.voxelize(p, leaf)["points"], p)


@pytest.mark.parametrize("dim", [2, 3])
def test_normals(dim):
    z = [0.0] * (dim - 2)
    pts = np.tile(np.array([[0.1, 0.1] + [0.1] * (dim - 2)], F), (8, 1))
    pts[4:] += 1.0  # two cells of four points
    nrm = np.array([[1, 0] + z, [-1, 0] + z, [0, 1] + z, [0, -1] + z,  # sums to zero: NaN
                    [0, 1] + z, [np.nan, 1] + z, [2.0, 0] + z, [0, 1] + z], F)  # NaN and a component >= 2 are left out
    r = vr.voxelize(pts, 1.0, normals=nrm)
    assert np.isnan(r["normals"][0]).all()
    assert vr.same_bits(r["normals"][1], np.array([0, 1] + z, F))
    assert r["result"]["num_with_normal"] == 1
    nrm[4:] = np.nan
    r = vr.voxelize(pts, 1.0, normals=nrm)  # no normal contributed
    assert np.isnan(r["normals"]).all() and r["result"]["num_with_normal"] == 0
    # the mean direction, normalised in float64
    nrm = np.tile(np.array([[0.6, 0.8] + z], F), (8, 1))
    nrm[1] = np.array([0.8, 0.6] + z, F)
    r = vr.voxelize(pts, 1.0, normals=nrm)
    v = nrm[:4].astype(np.float64).sum(0)
    assert np.abs(r["normals"][0].astype(np.float64) - v / np.linalg.norm(v)).max() < 1e-7
    # one point per cell: its normal goes through the same arithmetic (normalised), its coordinates do not
    r = vr.voxelize(pts[[0, 4]], 1.0, normals=np.array([[3e-3, 4e-3] + z, [0, 1.5] + z], F))
    assert np.abs(r["normals"].astype(np.float64) - np.array([[0.6, 0.8] + z, [0, 1] + z])).max() < 1e-6


def test_min_points_gate_order_and_counts():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 4, (300, 3)).astype(F)
    full = vr.voxelize(pts, 1.0)
    assert (np.diff(full["global_indices"]) > 0).all() and full["counts"].sum() == 300
    for mp in (2, 3, 6):
        r = vr.voxelize(pts, 1.0, min_points=mp)
        keep = full["counts"] >= mp
        assert 0 < keep.sum() < len(keep)
        assert np.array_equal(r["global_indices"], full["global_indices"][keep]) and np.array_equal(r["counts"], full["counts"][keep])
        assert vr.same_bits(r["points"], full["points"][keep])
        res = r["result"]
        assert res["num_occupied"] == len(keep) and res["num_voxels"] == keep.sum() and res["max_points_per_voxel"] == full["counts"].max()


@pytest.mark.parametrize("dim", [2, 3])
def test_first_is_the_source_at_the_global_indices_and_modes_agree_on_cells(dim):
    rng = np.random.default_rng(8)
    n = 2000
    pts = rng.uniform(-3, 3, (n, dim)).astype(F)
    pts[rng.choice(n, 40, replace=False), 0] = np.nan
    nrm = rng.normal(size=(n, dim)).astype(F)
    desc, inten = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.random(n, dtype=F)
    a = vr.voxelize(pts, 0.4, mode=vr.FIRST, normals=nrm, descriptors=desc, intensity=inten, min_points=2)
    g = a["global_indices"]
    assert vr.same_bits(a["points"], pts[g]) and vr.same_bits(a["normals"], nrm[g])
    assert vr.same_bits(a["descriptors"], desc[g]) and vr.same_bits(a["intensity"], inten[g])
    b = vr.voxelize(pts, 0.4, mode=vr.CENTROID, normals=nrm, descriptors=desc, intensity=inten, min_points=2)
    assert np.array_equal(b["global_indices"], g) and np.array_equal(b["counts"], a["counts"])
    assert vr.same_bits(b["descriptors"], desc[g]) and vr.same_bits(b["intensity"], inten[g])
    assert {k: v for k, v in a["result"].items() if k != "num_with_normal"} == \
           {k: v for k, v in b["result"].items() if k != "num_with_normal"}
    assert a["result"]["num_finite"] == n - 40 and 0 < a["result"]["num_voxels"] < a["result"]["num_occupied"]


def test_key_layout():
    """which extents the device's cell key holds: 2^30 cells per axis, 63 bits over the axes, relative to the lowest cell"""
    assert vr.key_layout(np.array([[5e5, 0, 0], [5e5 + 1000, 3, 0.5]], F), 1.0, (0, 0, 0), 3) == [10, 2, 0]
    assert vr.key_layout(np.array([[0, 0], [2.0 ** 31, 0]], F), 1.0, (0, 0, 0), 2) is None  # two points 2^31 leaves apart
    assert vr.key_layout(np.array([[0, 0], [2.0 ** 30 - 64, 0]], F), 1.0, (0, 0, 0), 2) == [30, 0]  # (a float32)
    far = np.array([[0, 0, 0], [1e7, 1e7, 1e7]], F)  # 3 x 24 bits
    assert vr.key_layout(far, 1.0, (0, 0, 0), 3) is None and vr.key_layout(far[:, :2], 1.0, (0, 0, 0), 2) == [24, 24]
    assert vr.key_layout(np.full((3, 3), np.nan, F), 1.0, (0, 0, 0), 3) == [0, 0, 0]
