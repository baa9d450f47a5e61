"""CPU: the provenance helper of tests/scene_provenance.py (which measurement point's fields every point of a merged scene
carries, read from the existing scene oracle through tagged normals) against a direct replay of
MergerCorrespondenceHomo_::compute() (S/mapping/merger_correspondence_homo_impl.cpp:51-115) that tracks the source of every
point itself -- duplicates, failed gates, invalid points and appends, in 2-D and 3-D, with tags up to the cap; and the
argument checking of Scene.set_features."""
import numpy as np
import pytest

import scene_provenance as sp_
from srrg2_slam_interfaces_amd import mapping
from srrg2_slam_interfaces_amd import synthetic as syn
from test_oracle_scene import _clouds_nd, _sqnorm, _valid, _xform

f32 = np.float32


def replay(scene_p, meas_p, T, corr, params):
    """:51-115 with `point_scene = point_meas` (:71) followed as "scene point s now carries measurement point m";
    returns (src, num_merged, num_added)"""
    sp = np.array(scene_p, f32)
    src = np.full(len(sp), -1, np.int64)
    valid = np.isfinite(np.asarray(meas_p, f32)).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        if corr is None:  # :30-41
            app = np.flatnonzero(valid)
            return np.concatenate([src, app]), 0, len(app)
        merged = np.zeros(len(meas_p), bool)
        for (s, m, resp) in corr:
            if not (f32(resp) < f32(params.maximum_response)):  # :60
                continue
            q = _xform(T, meas_p[m])
            if not (_sqnorm(q - sp[s]) < f32(params.maximum_distance_geometry_squared)):  # :69
                continue
            sp[s] = ((q + sp[s]) * f32(0.5)).astype(f32)  # :74
            src[s] = m  # :71
            merged[m] = True  # :75
    num_merged = int(merged.sum())
    app = np.flatnonzero(valid & ~merged) if num_merged < params.target_number_of_merges else np.zeros(0, np.int64)  # :92-115
    return np.concatenate([src, app]), num_merged, len(app)


def _transform(dim, k=0):
    return (syn.se3(np.array([0.1, -0.05, 0.02]) * (k + 1), np.deg2rad(np.array([20.0 + 31 * k, -10.0, 33.0 + 7 * k]))) if dim == 3
            else syn.se2(0.1, -0.05, np.deg2rad(33.0 + 47 * k))).astype(f32)


@pytest.mark.parametrize("target", [10 ** 6, 20, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_provenance_matches_the_replay_on_small_clouds(oracle, dim, target):
    sp, sn, mp, mn, T, corr = _clouds_nd(90 + dim, dim, ns=300, nm=400)
    hits = np.bincount([c[0] for c in corr], minlength=len(sp))
    assert hits.max() >= 3  # scene points hit several times
    params = mapping.MergerParams(50.0, 0.25, target)
    want, merged_n, added = replay(sp, mp, T, corr, params)
    src, coords, res = sp_.provenance(oracle, dim, sp, mp, T, corr, params)
    assert np.array_equal(src, want)
    assert (res["num_merged"], res["num_added"]) == (merged_n, added)
    assert merged_n > 20 and (added > 0) == (target > 20)
    # failed gates: some correspondences did not merge; invalid points: never appended, never a source
    assert (src[:len(sp)] >= 0).sum() < len({c[0] for c in corr})
    assert 5 not in src[len(sp):] and src[corr[0][0]] == -1
    # several hits with mixed outcomes: the last one that passed decides, not simply the last one listed
    last_listed = {}
    for (s, m, _) in corr:
        last_listed[s] = m
    assert any(src[s] not in (-1, m) for s, m in last_listed.items())
    # the carried field
    rng = np.random.default_rng(1)
    sf, mf = rng.integers(0, 256, (len(sp), 32), dtype=np.uint8), rng.integers(0, 256, (len(mp), 32), dtype=np.uint8)
    out = sp_.carried(src, sf, mf)
    for i, s in enumerate(src):
        assert np.array_equal(out[i], sf[i] if s < 0 else mf[s])


@pytest.mark.parametrize("dim", [3, 2])
def test_provenance_without_correspondences(oracle, dim):
    sp, _, mp, _, T, _ = _clouds_nd(95, dim)
    for scene_p in (sp, np.zeros((0, dim), f32)):
        want, _, added = replay(scene_p, mp, T, None, mapping.default_merger_params())
        src, coords, res = sp_.provenance(oracle, dim, scene_p, mp, T, None, mapping.default_merger_params())
        assert np.array_equal(src, want) and res["num_added"] == added == len(mp) - 1


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("dim", [3, 2])
def test_provenance_at_tags_up_to_the_cap(oracle, dim, k):
    """clouds of 2^20 - 1 points: the correspondences live at the highest indices, and the append reaches the highest tag"""
    rng = np.random.default_rng(100 + 10 * k + dim)
    n = sp_.TAG_CAP - 1
    T = _transform(dim, k)
    Ti = syn.se3_inv(T.astype(np.float64)) if dim == 3 else np.linalg.inv(T.astype(np.float64))[:2]
    sp = rng.uniform(-50, 50, (n, dim)).astype(f32)
    C = 4000
    m_idx = n - 1 - rng.permutation(6000)[:C]
    s_idx = n - 1 - rng.integers(0, 1500, C)  # ~2.7 hits per scene point
    mp = rng.uniform(-50, 50, (n, dim)).astype(f32)
    near = sp[s_idx].astype(np.float64) + rng.normal(scale=0.2, size=(C, dim))
    mp[m_idx] = (near @ Ti[:, :dim].T + Ti[:, dim]).astype(f32)
    mp[n - 7] = np.nan
    mp[::50021] = np.inf
    sp[n - 3] = np.nan
    corr = list(zip(s_idx.tolist(), m_idx.tolist(), rng.uniform(0, 80, C).tolist()))
    params = mapping.MergerParams(50.0, 0.25, 10 ** 9)
    want, merged_n, added = replay(sp, mp, T, corr, params)
    src, coords, res = sp_.provenance(oracle, dim, sp, mp, T, corr, params)
    assert np.array_equal(src, want)
    assert (res["num_merged"], res["num_added"]) == (merged_n, added)
    assert 500 < merged_n < C and added > n - C - 100
    assert src[n:].max() >= n - 20 and (src[:n] >= n - 6000).sum() > 300  # the highest tags, merged and appended


def test_provenance_refuses_clouds_past_the_cap(oracle):
    big = np.zeros((sp_.TAG_CAP, 2), f32)
    with pytest.raises(AssertionError, match="2\\^20"):
        sp_.provenance(oracle, 2, big, big[:3], syn.identity(2), None, mapping.default_merger_params())


# ---- Scene.set_features: argument checking (no device needed) --------------------------------------------------------------
def test_set_features_argument_checks():
    chk = mapping.as_scene_features
    d = np.zeros((5, 32), np.uint8)
    i = np.arange(5, dtype=np.float64)
    dd, ii = chk(d, i, 5)
    assert dd.dtype == np.uint8 and dd.shape == (5, 32) and ii.dtype == np.float32 and ii.shape == (5,)
    assert chk(None, None, 5) == (None, None)
    dd, _ = chk(np.zeros((5, 4), np.uint64), None, 5)  # any integer rows of 32 bytes
    assert dd.shape == (5, 32)
    assert chk(None, np.zeros((5, 1), f32), 5)[1].shape == (5,)
    for bad in (np.zeros((5, 31), np.uint8), np.zeros((4, 32), np.uint8), np.zeros((5, 8), f32), np.zeros(160, np.uint8)):
        with pytest.raises(ValueError):
            chk(bad, None, 5)
    for bad in (np.zeros(4, f32), np.zeros((5, 2), f32), np.array(["a"] * 5), np.zeros(5, np.complex64)):
        with pytest.raises(ValueError):
            chk(None, bad, 5)


def test_oracle_binding_has_no_features(oracle):
    s = mapping.Scene(oracle.scene_binding(), 3)
    s.set(np.zeros((2, 3), f32))
    with pytest.raises(NotImplementedError, match="product library only"):
        s.set_features(np.zeros((2, 32), np.uint8))
    with pytest.raises(NotImplementedError):
        s.has_features()
