"""CPU: the calls, caps and references of tests/map_large_cases.py are what they claim to be -- before tests/test_gpu_map_large.py
holds the device to them.  Crossing a launch cap exercises nothing unless the result depends on what lies behind it: the scans of
the second trip must have winners away from their guesses, the tiles of the strided trip must differ from those of the first and
hold winners, the long rays must leave misses in the grid late in their walk, and the guarded poses must be the ones the
restatement refuses to convert.  Needs no GPU: the library is imported (by tests/test_gpu_scan_match.py, for its map) and not
called."""
import numpy as np
import pytest

import gridmap_restatement as gr
import map_large_cases as mc


def test_constants():
    assert mc.PREP_CAP == 2_097_152 and mc.SCORE_CAP == 8_192
    assert gr.MAX_STEPS == 32000.0 and gr.CELL_GUARD == 2.0 ** 30
    assert np.float32(mc.RANGE_MAX) / np.float32(0.05) <= np.float32(gr.MAX_STEPS)
    # the tilings the existing tests run: one tile per (scan, rotation)
    assert mc.score_tiling(0, 0, 64, 65) == dict(LX=16, TY=64, tiles_x=1, tiles_y=1, nt=129, tiles=8385)
    t = mc.score_tiling(16, 16, 60, 23)
    assert mc.tile_of(t, 0) == (0, 0, 0, 0) and mc.tile_of(t, 4) == (0, 1, 1, 0) and mc.tile_of(t, 121 * 3) == (0, 0, 0, 1)


def test_prep_cap_second_trip_decides_winners():
    c = mc.match_case("prep_cap")
    nb, K, (wx, wy, ht), step = c["sc"]["num_beams"], len(c["scans"]), c["window"], c["step"]
    nt = 2 * ht + 1
    assert (K, nt, nb) == (33, 61, 1081) and K * nt * nb == 2_176_053 > mc.PREP_CAP
    first_whole = -(-mc.PREP_CAP // (nt * nb))  # the first scan whose triples all lie in trip 2
    assert first_whole == 32 == K - 1
    w = c["want"]
    print("prep_cap jtheta", w["jtheta"], "score", w["score"][-3:], "beams", w["num_scored_beams"][-3:])
    late = slice(first_whole, K)
    assert (w["score"][late] > 0).all() and ((w["jtheta"][late] != 0) | (w["dx"][late] != 0)).all()
    assert len(np.unique(w["jtheta"])) >= 5
    # the straddling scan 31: rotations on both sides of the cap (the 64-bit index is split mid-scan at the trip's start)
    jj_cap = (mc.PREP_CAP - 31 * nt * nb) // nb
    assert 0 < jj_cap < nt - 1
    assert 0 < w["num_scored_beams"].min() and w["num_scored_beams"].max() < nb  # the mixed ranges skip beams in every scan
    assert (w["score"] > w["score_at_guess"]).sum() >= K // 2


@pytest.mark.parametrize("name,tiling,tiles", [("tile_stride_y", (64, 16, 1, 3), 8349), ("tile_stride_xy", (32, 32, 3, 2), 9000)])
def test_tile_stride_hands_a_workgroup_another_tile(name, tiling, tiles):
    c = mc.match_case(name)
    (wx, wy, ht), K = c["window"], len(c["scans"])
    t = mc.score_tiling(wx, wy, ht, K)
    assert (t["LX"], t["TY"], t["tiles_x"], t["tiles_y"]) == tiling and t["tiles"] == tiles > mc.SCORE_CAP
    # every workgroup of the second trip holds another (tx, ty) than on its first
    for b in range(t["tiles"] - mc.SCORE_CAP):
        assert mc.tile_of(t, b)[:2] != mc.tile_of(t, b + mc.SCORE_CAP)[:2], b
    last_high = 2 * wy + 1 - (t["tiles_y"] - 1) * t["TY"]
    last_wide = 2 * wx + 1 - (t["tiles_x"] - 1) * t["LX"]
    assert (last_high, last_wide) == ((1, 33) if name == "tile_stride_y" else (9, 17))  # partial tiles: `high`, `wide`
    w = c["want"]
    tx, ty = mc.winner_tiles(t, w, wx, wy)
    print(name, "winner tiles tx", np.bincount(tx, minlength=3), "ty", np.bincount(ty, minlength=3), "jtheta", np.unique(w["jtheta"]).size)
    assert (ty > 0).any() and (ty == 0).any() and (w["score"] > 0).all()
    if t["tiles_x"] > 1:
        assert (tx > 0).any() and len(np.unique(tx)) >= 2
    # winners among the scans that have tiles in the strided trip, away from the guess
    first_late = mc.SCORE_CAP // (t["tiles"] // K)
    assert first_late < K and ((w["dx"][first_late:] != 0) | (w["dy"][first_late:] != 0)).any()
    assert w["scores"].shape == (K, 2 * ht + 1, 2 * wy + 1, 2 * wx + 1) and (w["scores"][first_late:] > 0).any()
    if name == "tile_stride_y":
        assert w["scores"].size == 3_030_687
        assert w["scores"][:, :, -1, :].any()  # the tile row of one shift holds scores


def _late_misses(c, first_step):
    """in-grid miss cells of rays at steps >= first_step: (number of such (ray, step) pairs, the rays' n)"""
    g, sc = c["g"], c["sc"]
    b = gr.beams(c["ranges"], c["poses"], sc, g)
    t = b["traced"].reshape(-1)
    x0, y0, x1, y1, n = (b[k].reshape(-1)[t] for k in ("x0", "y0", "x1", "y1", "n"))
    count, ns = 0, []
    for r in np.flatnonzero(n > first_step):
        i = np.arange(first_step, n[r])  # (step n is the end cell: a hit or nothing)
        one = np.ones(len(i), np.int64)
        cx, cy = gr.step_cells(x0[r] * one, y0[r] * one, x1[r] * one, y1[r] * one, i)
        inside = (cx >= 0) & (cx < g["cols"]) & (cy >= 0) & (cy < g["rows"])
        if inside.any():
            count += int(inside.sum())
            ns.append(int(n[r]))
    return count, ns


def test_long_rays_leave_misses_late_in_their_walk():
    c = mc.long_rays()
    w = c["want"]
    print("long_rays", w, "planes", int(c["h"].sum()), int(c["w"].sum()))
    assert w["num_miss_updates"] > 0 and w["num_hits_in_grid"] > 0 and w["num_skipped"] > 0
    assert w["num_cleared_only"] == 4 * 64 + 2
    b = gr.beams(c["ranges"], c["poses"], c["sc"], c["g"])
    n, dx, dy = b["n"], np.abs(b["x1"] - b["x0"]), np.abs(b["y1"] - b["y0"])
    assert b["traced"][b["clr"]].all() and n.max() == 31980
    assert ((n >= 31000) & (dx > 4 * dy)).any() and ((n >= 31000) & (dy > 4 * dx)).any()  # x-major and y-major
    assert ((n >= 22000) & (np.abs(dx - dy) < 200) & (dx != dy)).any()  # near the diagonal, not on it
    count, ns = _late_misses(c, 16001)
    print("long_rays: in-grid misses at steps > 16 000:", count, "from rays of n =", ns)
    assert count >= 10 and len(ns) >= 3 and max(ns) == 31980
    count30, _ = _late_misses(c, 29000)
    assert count30 >= 3  # the y-major ray reaches the grid after 30 000 steps
    # the lone long beams: one cleared beam in a scan whose other beams are short returns or skipped
    for k in (4, 5):
        assert b["clr"][k].sum() == 1 and n[k][b["clr"][k]] >= 31900 and n[k][b["ret"][k]].max() <= 8 and (~b["ret"][k] & ~b["clr"][k]).sum() >= 5
    alone = gr.integrate(*gr.new_planes(c["g"]), c["ranges"][5:], c["poses"][5:], c["sc"], c["g"])
    assert alone["num_miss_updates"] > 0  # the lone beam from 800 m away crosses the grid


@pytest.mark.parametrize("nb", [64, 32])
def test_guard_poses_are_the_ones_the_restatement_refuses(nb):
    for origin in ((0.0, 0.0), (0.0, -1.0e9)):
        c = mc.guard(nb, origin)
        b = gr.beams(c["ranges"], c["poses"], c["sc"], c["g"])
        ret, traced = b["ret"], b["traced"]
        w = c["want"]
        print("guard", nb, origin, w)
        assert w["num_returns"] == ret.sum() > 0 and w["num_skipped"] > 0
        for k in mc.GUARD_GROUPS["beyond"]:
            assert ret[k].any() and not traced[k].any()  # counted as returns, not convertible
        if origin[1] == 0.0:
            for k in mc.GUARD_GROUPS["within"] + mc.GUARD_GROUPS["inside"]:
                assert traced[k][ret[k]].all()  # convertible, however far away
            k = mc.GUARD_GROUPS["edge"][0]
            assert (ret[k] & traced[k]).any() and (ret[k] & ~traced[k]).any()  # the sensor's cell is, some end cells are not
            assert w["num_hits_in_grid"] > 0 and w["num_miss_updates"] > 0 and c["h"].any()
            solo = gr.integrate(*gr.new_planes(c["g"]), c["ranges"][[0, 7]], c["poses"][[0, 7]], c["sc"], c["g"])
            assert (solo["num_hits_in_grid"], solo["num_miss_updates"]) == (w["num_hits_in_grid"], w["num_miss_updates"])
        else:
            assert not traced.any() and not c["h"].any() and not c["w"].any() and w["num_hits_in_grid"] == w["num_miss_updates"] == 0
