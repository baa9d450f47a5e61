"""GPU: the scan matcher (csrc/scan_match.hip) past both of its launch caps and the grid map (csrc/gridmap.hip) on rays of tens of
thousands of steps and on cells its guard refuses (tests/map_large_cases.py says where the thresholds come from), BIT FOR BIT
against the numpy restatements with the helpers of tests/test_gpu_scan_match.py and tests/test_gpu_gridmap.py.
tests/test_map_large_cases.py proves on the CPU that each case reaches the path it is here for:

  second trip of k_match_prep, the triple's index split past 2 097 152              test_prep_cap
  k_match_score strided over tiles with another ty / tx and ty on the second trip,
  partial last tile rows and columns (high = 1; wide = 17, high = 9)                test_tile_stride[tile_stride_y], [tile_stride_xy]
  the merged walk over 31 980 steps against the closed form: x-major, y-major and
  near the diagonal; one long ray beside 63 dead or short lanes; in and out again   test_long_rays
  sensor or end cell not convertible: counted, nothing drawn                        test_cell_guard[64], [32]

Not reached, on purpose: grids near 32 768 x 32 768 (8 GB of planes); a score volume or a triple count near 2^31 (no restatement
follows them in test time); the builds with -DSRRG2_SCAN_MATCH_PLAIN and -DSRRG2_GRIDMAP_WAVE_MERGE=0, which the library does
not ship.

The device's share of every test is milliseconds; the time is the CPU restatements', computed once per case in map_large_cases and
shared by the tests of a session.  Seconds on one core of the development machine: prep_cap 5.4, tile_stride_y 0.8,
tile_stride_xy 0.6, long_rays 1.2, guard 1.0 per scanner and origin (its `edge` scan and the cleared beams of
gridmap_cases.mixed are rays of up to 31 980 steps as well).
"""
import numpy as np
import pytest

import gridmap_restatement as gr
import map_large_cases as mc
import test_gpu_gridmap as tg
import test_gpu_scan_match as tm

pytestmark = pytest.mark.gpu
F = np.float32


def _match(product, name):
    c = mc.match_case(name)
    m = tm._drawn(product, c["drawn"])
    assert np.array_equal(m.likelihood(), c["drawn"][7])
    (wx, wy, ht), want = c["window"], c["want"]
    got = m.match_scans(c["scans"], c["guesses"], (wx, wy), ht, c["step"], want_scores=True)
    tm._same(got, want, name)
    return m, c


def test_prep_cap(product):
    """33 scans x 61 rotations x 1 081 beams = 2 176 053 triples: k_match_prep's grid-stride loop takes its second trip, which
    holds the end of scan 31 and all of scan 32; every result member and the volume"""
    m, c = _match(product, "prep_cap")
    assert len(c["scans"]) * 61 * 1081 > mc.PREP_CAP
    # ... and from device memory, the volume left on the device
    import torch

    (wx, wy, ht), want = c["window"], c["want"]
    dr, dg = torch.from_numpy(np.array(c["scans"])).cuda(), torch.from_numpy(np.array(c["guesses"])).cuda()
    vol = torch.full((want["scores"].size + 4,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    got = m.match_scans(dr, dg, (wx, wy), ht, c["step"], want_scores=vol[:want["scores"].size])
    back = vol.cpu().numpy()
    assert np.array_equal(back[:-4].reshape(want["scores"].shape), want["scores"]) and (back[-4:] == -7).all()
    got["scores"] = want["scores"]
    tm._same(got, want, "prep_cap from the device")


@pytest.mark.parametrize("name", ["tile_stride_y", "tile_stride_xy"])
def test_tile_stride(product, name):
    """more tiles than k_match_score has workgroups, several tiles per (scan, rotation): on its second trip a workgroup scores
    another (tx, ty) -- another `wide`, `high` and `holds` over the same shared beam list, live count and reduction words; every
    result member and the whole volume (3 030 687 and 4 982 100 scores)"""
    m, c = _match(product, name)
    (wx, wy, ht), K = c["window"], len(c["scans"])
    assert mc.score_tiling(wx, wy, ht, K)["tiles"] > mc.SCORE_CAP
    # without the volume the winners are the same
    tm._same(m.match_scans(c["scans"], c["guesses"], (wx, wy), ht, c["step"]), {k: v for k, v in c["want"].items() if k != "scores"},
             name + " without the volume")


def test_long_rays(product):
    """rays of up to 31 980 steps that cross the 7 x 9 grid after 16 000 and 30 000 of them: the carried quotient / remainder of
    the walk against the contract's closed form -- planes and all counters; a wave with one live long ray; then the same batch
    with weight -1 leaves the zero planes"""
    c = mc.long_rays()
    m = tm._grid_of(product, c["g"], c["sc"])
    assert m.integrate(c["ranges"], c["poses"]) == c["want"]
    tg._same_planes(m, c["h"], c["w"], "long rays in")
    assert c["w"].any() and c["h"].any()
    assert m.remove(c["ranges"], c["poses"]) == c["want"]
    zero = gr.new_planes(c["g"])
    tg._same_planes(m, zero[0], zero[1], "long rays out again")
    # scan by scan, from device memory, queued: the same planes
    import torch

    dr, dp = torch.from_numpy(np.array(c["ranges"])).cuda(), torch.from_numpy(np.array(c["poses"])).cuda()
    torch.cuda.synchronize()
    for k in range(len(c["poses"])):
        assert m.integrate(dr[k:k + 1], dp[k:k + 1], want_result=False) is None
    tg._same_planes(m, c["h"], c["w"], "long rays, one scan per call")


@pytest.mark.parametrize("nb", [64, 32])
def test_cell_guard(product, nb):
    """poses at +-6e7 m (x / 0.05 passes 2^30), at 5.3e7 m (just inside), on the last convertible float32, and a grid whose origin
    is (0, -1e9): a beam whose sensor or end cell is not convertible counts as a return and draws nothing; nb = 32: two scans per
    wave, a drawing one beside a guarded one"""
    for origin in ((0.0, 0.0), (0.0, -1.0e9)):
        c = mc.guard(nb, origin)
        m = tm._grid_of(product, c["g"], c["sc"])
        assert m.integrate(c["ranges"], c["poses"]) == c["want"], (nb, origin)
        tg._same_planes(m, c["h"], c["w"], "guard %d %s" % (nb, origin))
        assert m.remove(c["ranges"], c["poses"]) == c["want"], (nb, origin)
        zero = gr.new_planes(c["g"])
        tg._same_planes(m, zero[0], zero[1], "guard out again")
