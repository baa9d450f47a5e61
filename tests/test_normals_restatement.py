"""CPU: the numpy restatement of srrg2_scene_estimate_normals (tests/normals_restatement.py, DESIGN.md section 4 "Normals of
unorganised scenes") against numpy.linalg.eigh, exact rational moments and known geometry; the ctypes layouts and the C++ mirror's
header.  The GPU suite (tests/test_gpu_normals.py) then holds the library to this restatement bit for bit."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import normals_restatement as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

# radius per surface: about 30 neighbours at 5 000 points
CASES_3D = [("plane", 0.09), ("sphere", 0.16), ("cylinder", 0.12), ("crossing", 0.09)]
CASES_2D = [("line", 0.006), ("circle", 0.02), ("crossing", 0.012)]


@pytest.fixture(scope="module")
def estimated():
    out = {}
    for dim, cases in ((3, CASES_3D), (2, CASES_2D)):
        for seed, (kind, radius) in enumerate(cases):
            P = nr.surface(kind, 5000, 100 + seed, radius, dim)
            out[(dim, kind)] = (P, radius, nr.estimate_normals(P, radius, dim=dim, viewpoint=None, drop=False))
    return out


@pytest.mark.parametrize("dim,kind", [(3, k) for k, _ in CASES_3D] + [(2, k) for k, _ in CASES_2D])
def test_solver_against_eigh(estimated, dim, kind):
    """on the covariance matrices the restatement itself formed: where (lambda1 - lambda0) / trace >= 1e-3 the eigenvector is
    eigh's to |sin| <= 1e-9 and the eigenvalues agree within 1e-12 trace; at most 2 % of the points fall under the gap"""
    P, radius, r = estimated[(dim, kind)]
    f = np.flatnonzero(np.isfinite(r["cov"]).all((1, 2)))
    assert f.size > 4000
    cov = r["cov"][f]
    diag, V = nr.jacobi(cov, dim)
    l0, vec, trace = nr.smallest(diag, V, dim)
    w, U = np.linalg.eigh(cov)
    gap = (w[:, 1] - w[:, 0]) / trace
    sel = gap >= 1e-3
    excluded = 1.0 - sel.mean()
    print("%dD %s: %d matrices, %.2f %% under the gap" % (dim, kind, f.size, 100 * excluded))
    assert excluded <= 0.02
    vec = vec / np.linalg.norm(vec, axis=1, keepdims=True)
    cosang = np.abs(np.einsum("ij,ij->i", vec, U[:, :, 0]))
    sin = np.sqrt(np.maximum(0.0, 1.0 - cosang * cosang))
    # (1 - cos^2 loses half the digits near 1: take the sine from the component orthogonal to eigh's vector)
    ortho = vec - np.einsum("ij,ij->i", vec, U[:, :, 0])[:, None] * U[:, :, 0]
    sin = np.minimum(sin, np.linalg.norm(ortho, axis=1))
    print("   max |sin| %.3g, max eigenvalue error / trace %.3g" %
          (sin[sel].max(), (np.abs(np.sort(diag, 1) - w) / trace[:, None])[sel].max()))
    assert sin[sel].max() <= 1e-9
    assert (np.abs(np.sort(diag, 1) - w)[sel] <= 1e-12 * trace[sel, None]).all()


@pytest.mark.parametrize("dim", [2, 3])
def test_fixed_point_moments_are_the_exact_moments_rounded_per_term(dim):
    """|S / 2^e - exact| <= k * 2^-(e+1), in exact rational arithmetic"""
    rng = np.random.default_rng(5)
    P = rng.uniform(-1, 1, (150, dim)).astype(F32)
    radius = 0.45
    count, S1, S2, (e1, e2) = nr.moments(P, radius, dim)
    pairs = nr.second_moment_pairs(dim)
    members = {i: [] for i in range(len(P))}
    for qi, cj, d in nr.member_pairs(P, radius, dim):
        for i, dd in zip(qi.tolist(), d.tolist()):
            members[i].append([Fraction(float(F32(x))) for x in dd])
    assert count.min() >= 1 and count.max() > 10
    for i, ds in members.items():
        k = len(ds)
        assert k == count[i]
        for a in range(dim):
            exact = sum(d[a] for d in ds)
            assert abs(Fraction(int(S1[i, a]), 1) / Fraction(2) ** e1 - exact) <= k * Fraction(1, 2) ** (e1 + 1)
        for c, (a, b) in enumerate(pairs):
            exact = sum(d[a] * d[b] for d in ds)
            assert abs(Fraction(int(S2[i, c]), 1) / Fraction(2) ** e2 - exact) <= k * Fraction(1, 2) ** (e2 + 1)


@pytest.mark.parametrize("radius", [1e-3, 0.1, 0.75, 1.0, 37.5, 1e4])
def test_fixed_point_range_at_the_largest_scene(radius):
    """n = 2^31 - 1 members, every |d| = radius (and a float32 rounding above it): the sums stay below 2^62, a term below 2^51"""
    n = 2 ** 31 - 1
    e1, e2 = nr.exponents(radius, n)
    d = Fraction(float(F32(radius))) * (1 + Fraction(1, 2 ** 22))
    assert n * d * Fraction(2) ** e1 < 2 ** 62 and n * d * d * Fraction(2) ** e2 < 2 ** 62
    for m in (1, 2, 1000, n):
        f1, f2 = nr.exponents(radius, m)
        assert d * Fraction(2) ** f1 < 2 ** 51 and d * d * Fraction(2) ** f2 < 2 ** 51
        assert m * d * Fraction(2) ** f1 < 2 ** 62 and m * d * d * Fraction(2) ** f2 < 2 ** 62
    # ... and the library's host-side formula is the same (no device needed)
    from srrg2_slam_interfaces_amd import _capi

    a, b = C.c_int(0), C.c_int(0)
    for m in (1, 2, 3, 1000, 100000, n):
        _capi.lib().srrg2_normals_exponents(C.c_float(radius), C.c_int(m), C.byref(a), C.byref(b))
        assert (a.value, b.value) == nr.exponents(radius, m)


def _lattice_plane(m=9, spacing=0.125):
    g = np.arange(m, dtype=np.float64) * spacing
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.zeros(m * m)], 1).astype(F32)


def test_lattice_plane_gives_the_exact_normal():
    P = _lattice_plane()
    for vp, sign in (((0.5, 0.5, 2.0), 1.0), ((0.5, 0.5, -2.0), -1.0), (None, 1.0)):
        r = nr.estimate_normals(P, 0.26, viewpoint=vp, drop=False)
        assert (r["cls"] == nr.CLS_NORMAL).all()
        assert np.array_equal(r["normals"], np.tile(np.array([0, 0, sign], F32), (len(P), 1)))  # (a flipped 0 is -0)
        assert nr.same_bits(r["curvature"], np.zeros(len(P), F32))
    # no viewpoint: the component of largest magnitude is positive, the first on a tie
    Q = np.stack([P[:, 0], P[:, 1], (-P[:, 0]).astype(F32)], 1)  # plane x + z = 0: n = +-(1, 0, 1) / sqrt 2
    n = nr.estimate_normals(Q, 0.25, viewpoint=None, drop=False)["normals"]
    assert (n[:, 0] > 0).all() and (n[:, 2] > 0).all() and np.allclose(n[:, 1], 0, atol=1e-7)
    n = nr.estimate_normals(Q, 0.25, viewpoint=(np.nan, 0, 0), drop=False)["normals"]
    assert (n[:, 0] > 0).all()


def test_classes():
    cluster = _lattice_plane(5, 0.125)
    lonely = np.array([[50.0, 0, 0]], F32)
    dup = np.tile(np.array([[9.0, 9.0, 9.0]], F32), (5, 1))
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0]], F32)
    P = np.concatenate([cluster, lonely, dup, bad])
    r = nr.estimate_normals(P, 0.26, min_neighbours=5, drop=True)
    cls = r["cls"]
    assert (cls[:25] == nr.CLS_NORMAL).all() and cls[25] == nr.CLS_TOO_FEW
    assert (cls[26:31] == nr.CLS_DEGENERATE).all() and (cls[31:] == nr.CLS_NOT_FINITE).all()
    assert r["result"] == {"num_points": 33, "num_finite": 31, "num_with_normal": 25, "num_too_few": 1, "num_degenerate": 5,
                           "num_too_curved": 0, "scene_size": 25}
    assert np.array_equal(r["kept"], np.arange(25))
    assert np.isnan(r["curvature"][25:]).all() and np.isnan(r["normals"][25:]).all()
    # too curved: a noisy blob against a gate
    blob = np.random.default_rng(1).normal(size=(200, 3)).astype(F32)
    r = nr.estimate_normals(blob, 1.0, max_curvature=0.05, drop=False)
    curved = r["cls"] == nr.CLS_TOO_CURVED
    assert curved.sum() > 50 and (r["curvature"][curved] > F32(0.05)).all() and np.isnan(r["normals"][curved]).all()
    assert (r["curvature"][r["cls"] == nr.CLS_NORMAL] <= F32(0.05)).all()


def test_collinear_points_in_3d_are_pinned():
    """points on the x axis: the covariance is diag(c, 0, 0), no rotation happens, lambda0 = lambda1 = 0 tie -> the lowest column
    of the two, (0, 1, 0); curvature 0"""
    P = np.zeros((7, 3), F32)
    P[:, 0] = np.arange(7) * 0.125
    r = nr.estimate_normals(P, 0.55, viewpoint=None, drop=False)
    assert (r["cls"] == nr.CLS_NORMAL).all()
    assert nr.same_bits(r["normals"], np.tile(np.array([0, 1, 0], F32), (7, 1)))
    assert nr.same_bits(r["curvature"], np.zeros(7, F32))


@pytest.mark.parametrize("dim", [2, 3])
def test_membership_is_inclusive_at_exactly_the_radius(dim):
    """a lattice with spacing exactly the radius: the axis neighbours are members, the diagonal ones are not"""
    m, radius = 5, 0.25
    g = np.arange(m, dtype=np.float64) * radius
    P = np.stack([a.ravel() for a in np.meshgrid(*([g] * dim), indexing="ij")], 1).astype(F32)
    count = nr.moments(P, radius, dim)[0]
    idx = np.stack([a.ravel() for a in np.meshgrid(*([np.arange(m)] * dim), indexing="ij")], 1)
    expect = 1 + sum((idx[:, d] > 0).astype(int) + (idx[:, d] < m - 1).astype(int) for d in range(dim))
    assert np.array_equal(count, expect)


def test_ctypes_layouts_and_header():
    from srrg2_slam_interfaces_amd import _abi as abi

    assert C.sizeof(abi.NormalsParams) == 32
    assert C.sizeof(abi.NormalsResult) == 28
    txt = open(os.path.join(ROOT, "include", "srrg2_slam_amd.h")).read()
    assert "void srrg2_normals_default_params(srrg2_normals_params* p, int dim);" in txt
    assert "srrg2_scene_estimate_normals(srrg2_scene_h scene, const srrg2_normals_params* p," in txt
    assert "#define SRRG2_AMD_ABI_VERSION 4" in txt


def test_default_params_through_the_library():
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import _capi

    for dim, mn in ((3, 5), (2, 3)):
        p = abi.NormalsParams()
        _capi.lib().srrg2_normals_default_params(C.byref(p), dim)
        assert p.min_neighbours == mn and p.max_curvature == 1.0 and p.drop_points_without_normal == 1 and p.radius > 0
        assert list(p.viewpoint) == [0.0, 0.0, 0.0]


def test_header_compiles_with_plain_gxx(tmp_path):
    src = tmp_path / "tu.cpp"
    src.write_text('#include <vector>\n#include "srrg2_slam_amd.hpp"\n'
                   'int f(srrg2_slam_amd::Scene<3>& a, srrg2_slam_amd::Scene<2>& b) {\n'
                   '  srrg2_normals_params p;\n  srrg2_normals_default_params(&p, 3);\n  std::vector<float> curv;\n'
                   '  srrg2_normals_result r = a.estimateNormals(p, &curv);\n  srrg2_normals_default_params(&p, 2);\n'
                   '  return r.num_with_normal + b.estimateNormals(p).scene_size;\n}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
