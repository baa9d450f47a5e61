"""Pair batches (srrg2_align_pairs): K alignments, each of its own fixed cloud against its own moving cloud, in one call.

"Equal" means bit-identical: estimate bits, status, iteration count, the last IterationStats record, correspondence count
and H.  Every pair is compared with a fresh handle's single set_fixed / set_moving / set_moving_in_fixed / compute()."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import cue_config, prior_config
from srrg2_slam_interfaces_amd import _abi as abi
from srrg2_slam_interfaces_amd import synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -4, -5  # srrg2_status codes of the C ABI


def _record(r, dim):
    """the comparable content of one result record (a BatchResults item), as bytes and ints"""
    return (r["moving_in_fixed"].tobytes(), r["status"], r["num_iterations"], tuple(sorted(r["last"].items())),
            r["num_correspondences"], r["information"].tobytes())


def _make(product, kind, cfgs, params=None, term=None, priors=None):
    al = product.MultiAligner(kind)
    for c in cfgs:
        al.add_slice(c)
    if params:
        al.set_params(**params)
    if term is not None:
        al.set_termination_criteria(term)
    for si, T in (priors or {}).items():
        al.set_prior_measurement(si, T)
    return al


def _single(product, kind, cfgs, pair, guess, **setup):
    """a fresh handle's single compute() of one pair, as a result record (the defining loop, run for one pair)"""
    al = _make(product, kind, cfgs, **setup)
    return al._pairs_loop([pair["fixed"]], [pair["moving"]], [guess],
                          None if pair.get("fixed_normals") is None else [pair["fixed_normals"]],
                          None if pair.get("moving_normals") is None else [pair["moving_normals"]])[0]


def _pairs(al, pairs, guesses, normals=True):
    fn = [p["fixed_normals"] for p in pairs] if normals else None
    mn = [p["moving_normals"] for p in pairs] if normals else None
    return al.compute_batch_pairs([p["fixed"] for p in pairs], [p["moving"] for p in pairs], guesses, fn, mn)


def _assert_each_equals_single(product, kind, cfgs, pairs, guesses, res, **setup):
    dim = abi.point_dim(kind)
    assert len(res) == len(pairs)
    for k, (p, g) in enumerate(zip(pairs, guesses)):
        ref = _single(product, kind, cfgs, p, g, **setup)
        assert _record(res[k], dim) == _record(ref, dim), k


def _distinct_3d(K, n, seed):
    return syn.batch_3d(K=K, n=n, seed=seed, shared_fixed_group=1)


def test_distinct_se3_pairs_equal_single_compute_and_oracle(oracle, product):
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05, 0.8)
    pairs = _distinct_3d(8, 20_000, 4700)
    ident = syn.identity(3)
    al = _make(product, kind, [cfg])
    res = _pairs(al, pairs, [ident] * 8)
    assert all(r["status"] == abi.SUCCESS for r in res)
    _assert_each_equals_single(product, kind, [cfg], pairs, [ident] * 8, res)
    # the project's parity target: the oracle's own loop on two sampled pairs
    ref = oracle.OracleAligner(kind)
    ref.add_slice(cfg)
    picks = [1, 6]
    ro = ref.compute_batch_pairs([pairs[k]["fixed"] for k in picks], [pairs[k]["moving"] for k in picks], [ident] * 2,
                                 [pairs[k]["fixed_normals"] for k in picks], [pairs[k]["moving_normals"] for k in picks])
    for j, k in enumerate(picks):
        assert _record(ro[j], 3) == _record(res[k], 3), k


@pytest.mark.parametrize("slice_kind", [abi.SLICE_P2P, abi.SLICE_P2PLANE])
def test_se2_scans_on_the_one_workgroup_path(product, slice_kind):
    kind = abi.SE2_RIGHT
    cfg = cue_config(kind, slice_kind, 0.3)
    pairs = [syn.scan_pair_2d(beams=1000, t=(0.05 * k, -0.03 * k), theta_deg=1.0 + k, seed=1300 + 10 * k) for k in range(6)]
    guesses = [syn.identity(2)] * len(pairs)
    al = _make(product, kind, [cfg])
    res = _pairs(al, pairs, guesses)
    assert al.last_compute_path() & abi.PATH_ONE_WORKGROUP
    assert all(r["status"] == abi.SUCCESS for r in res)
    _assert_each_equals_single(product, kind, [cfg], pairs, guesses, res)


def test_se3_euler_point_to_point(product):
    kind = abi.SE3_EULER_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2P, 0.25)
    pairs = _distinct_3d(5, 6_000, 4800)
    guesses = [syn.identity(3)] * 5
    al = _make(product, kind, [cfg])
    res = _pairs(al, pairs, guesses, normals=False)
    _assert_each_equals_single(product, kind, [cfg], [dict(p, fixed_normals=None, moving_normals=None) for p in pairs],
                               guesses, res)


def _scaled(p, s):
    return dict(p, fixed=np.ascontiguousarray(p["fixed"] * s), moving=np.ascontiguousarray(p["moving"] * s))


def test_mixed_pairs_sizes_empty_nonfinite_and_extents(product):
    """0 / 1 / 10 / 1 000 / 100 000 fixed points, an empty moving cloud, NaN / inf points, a 10 km pair beside a 1 m pair:
    every pair equals its single compute(), a bad pair does not disturb its neighbours"""
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2P, 0.25)
    big = syn.cloud_pair_3d(n=100_000, seed=4900)
    base = syn.cloud_pair_3d(n=3_000, seed=4901)

    def cut(nf, nm=2_000):
        return {"fixed": big["fixed"][:nf], "moving": big["moving"][:nm]}

    bad = {"fixed": base["fixed"].copy(), "moving": base["moving"].copy()}
    bad["fixed"][::7, 0] = np.nan
    bad["fixed"][3::11, 2] = np.inf
    bad["moving"][::5, 1] = -np.inf
    bad["moving"][2::13, 0] = np.nan
    pairs = [cut(0), cut(1), cut(10), cut(1_000), {"fixed": big["fixed"], "moving": big["moving"]},
             {"fixed": base["fixed"], "moving": base["moving"][:0]}, bad,
             _scaled(base, 1000.0), _scaled(base, 0.1), cut(1_000)]
    for p in pairs:
        p["fixed"], p["moving"] = (np.ascontiguousarray(p[k], dtype=np.float32) for k in ("fixed", "moving"))
    guesses = [syn.identity(3)] * len(pairs)
    al = _make(product, kind, [cfg])
    res = _pairs(al, pairs, guesses, normals=False)
    _assert_each_equals_single(product, kind, [cfg], pairs, guesses, res)
    # the neighbours of the bad pair alone give what they give inside the batch
    alone = _pairs(al, pairs[3:4], guesses[:1], normals=False)
    assert _record(alone[0], 3) == _record(res[3], 3)
    assert _record(alone[0], 3) == _record(res[9], 3)


def test_exponent_isolation(product):
    """pair B = pair A with its fixed normals scaled x 8: A's bits do not depend on whether B is in the batch (every pair's
    fixed-point exponent is sized by its own normals, as its single compute()'s)"""
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25)  # (normal gate off: scaled normals are legal input)
    a = _distinct_3d(1, 8_000, 5000)[0]
    b = dict(a, fixed_normals=np.ascontiguousarray(a["fixed_normals"] * 8.0))
    ident = syn.identity(3)
    al = _make(product, kind, [cfg])
    alone = _pairs(al, [a], [ident])
    both = _pairs(al, [a, b], [ident, ident])
    assert _record(alone[0], 3) == _record(both[0], 3)
    _assert_each_equals_single(product, kind, [cfg], [a, b], [ident, ident], both)


def test_solver_settings(product):
    kind = abi.SE3_QUAT_RIGHT
    pairs = _distinct_3d(4, 5_000, 5100)
    guesses = [syn.identity(3)] * 4
    term = abi.TerminationParams(3, 12, 12, 12, 0.3)
    Z = syn.identity(3)
    Z[0, 3] = 0.01
    setups = [
        ([cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CLAMP, 0.002)],
         dict(params=dict(max_iterations=8, enable_inlier_only_runs=True))),
        ([cue_config(kind, abi.SLICE_P2P, 0.25, abi.ROBUST_CAUCHY, 0.01)],
         dict(params=dict(keep_only_inlier_correspondences=True))),
        ([cue_config(kind, abi.SLICE_P2PLANE, 0.25, min_corr=50)], dict(params=dict(max_iterations=20), term=term)),
        ([cue_config(kind, abi.SLICE_P2PLANE, 0.25), prior_config(kind, [10, 10, 10, 100, 100, 100], sets_guess=0)],
         dict(priors={1: Z})),
    ]
    for cfgs, setup in setups:
        al = _make(product, kind, cfgs, **setup)
        res = _pairs(al, pairs, guesses)
        _assert_each_equals_single(product, kind, cfgs, pairs, guesses, res, **setup)


@pytest.mark.parametrize("stride", [12, 16])
def test_device_inputs_equal_host_inputs(product, stride):
    import torch

    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05, 0.8)
    pairs = _distinct_3d(6, 10_000, 5200)
    ident = syn.identity(3)
    al = _make(product, kind, [cfg])
    host = _pairs(al, pairs, [ident] * 6)

    def dev(key):
        a = np.concatenate([p[key] for p in pairs], axis=0)
        out = np.zeros((a.shape[0], stride // 4), np.float32)
        out[:, :3] = a
        return torch.from_numpy(out).cuda()

    f, fn, m, mn = (dev(k) for k in ("fixed", "fixed_normals", "moving", "moving_normals"))
    foff = np.concatenate([[0], np.cumsum([p["fixed"].shape[0] for p in pairs])]).astype(np.int32)
    moff = np.concatenate([[0], np.cumsum([p["moving"].shape[0] for p in pairs])]).astype(np.int32)
    torch.cuda.synchronize()
    d = al.compute_batch_pairs_device(f.data_ptr(), stride, fn.data_ptr(), stride, foff, m.data_ptr(), stride, mn.data_ptr(),
                                      stride, moff, np.stack([ident] * 6))
    assert [_record(r, 3) for r in d] == [_record(r, 3) for r in host]


def test_handle_state_around_a_pair_call(product):
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05, 0.8)
    shared = syn.batch_3d(K=4, n=10_000, seed=5300, shared_fixed_group=4)
    pairs = _distinct_3d(3, 8_000, 5310)
    ident = syn.identity(3)
    al = _make(product, kind, [cfg])
    al.set_fixed(0, shared[0]["fixed"], shared[0]["fixed_normals"])
    mov = [p["moving"] for p in shared]
    mnr = [p["moving_normals"] for p in shared]
    before = bytes(al.compute_batch(mov, [ident] * 4, mnr)._raw)
    # the same handle twice: its map's grid has its neighbour lists by now (the second batch takes the list path)
    before2 = bytes(al.compute_batch(mov, [ident] * 4, mnr)._raw)
    res = _pairs(al, pairs, [ident] * 3)
    # status, estimate, statistics and H of pair K-1 are the handle's
    assert al.status() == res[2]["status"]
    assert al.moving_in_fixed().tobytes() == res[2]["moving_in_fixed"].tobytes()
    n, last = al.last_iteration_stats()
    assert n == res[2]["num_iterations"] and last == res[2]["last"]
    assert al.information().tobytes() == res[2]["information"].tobytes()
    assert al.num_correspondences() == res[2]["num_correspondences"]
    # no pair records
    for fn in (al.correspondences, al.factor_status):
        with pytest.raises(RuntimeError, match=r"code %d" % E_STATE):
            fn(0)
    # the moving cloud is unbound
    with pytest.raises(RuntimeError, match=r"code %d" % E_STATE):
        al.compute()
    # the bound map is untouched
    after = bytes(al.compute_batch(mov, [ident] * 4, mnr)._raw)
    assert after == before2 == before
    al.set_moving(0, shared[1]["moving"], shared[1]["moving_normals"])
    al.set_moving_in_fixed(ident)
    assert al.compute() == abi.SUCCESS
    assert len(al.correspondences(0)) > 0


def _raw_call(al, K, fc, foff, mc, moff, mem=abi.MEM_HOST, fptr=True, mptr=True):
    f = al._b.lib.srrg2_align_pairs
    g = np.stack([syn.identity(al.dim)] * max(K, 1)).astype(np.float32)
    res = (abi.BatchResult * max(K, 1, 70000 if K > 65535 else 1))()
    i32 = C.POINTER(C.c_int32)
    fp = C.POINTER(C.c_float)
    return f(al._h, C.c_int(K), fc.ctypes.data_as(fp) if fptr else None, C.c_int(12), None, C.c_int(0),
             foff.ctypes.data_as(i32) if foff is not None else None, mc.ctypes.data_as(fp) if mptr else None, C.c_int(12), None,
             C.c_int(0), moff.ctypes.data_as(i32) if moff is not None else None, C.c_int(mem), g.ctypes.data_as(fp), res)


def test_errors_leave_the_handle_usable(product):
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2P, 0.25)
    pairs = _distinct_3d(2, 3_000, 5400)
    guesses = [syn.identity(3)] * 2
    good = [_single(product, kind, [cfg], p, g) for p, g in zip(pairs, guesses)]

    def check_good(al):
        res = _pairs(al, pairs, guesses, normals=False)
        assert [_record(r, 3) for r in res] == [_record(r, 3) for r in good]

    al = _make(product, kind, [cfg])
    fc = np.ascontiguousarray(np.concatenate([p["fixed"] for p in pairs]), np.float32)
    mc = np.ascontiguousarray(np.concatenate([p["moving"] for p in pairs]), np.float32)
    off = np.array([0, 3_000, 6_000], np.int32)
    big = np.zeros(70_000, np.int32)
    assert _raw_call(al, 0, fc, off, mc, off) == 0
    assert _raw_call(al, -1, fc, off, mc, off) == E_INVALID
    assert _raw_call(al, 65536, fc, big, mc, big) == E_INVALID
    assert _raw_call(al, 2, fc, np.array([0, 3_000, 2_000], np.int32), mc, off) == E_INVALID
    assert _raw_call(al, 2, fc, off, mc, np.array([10, 5, 6_000], np.int32)) == E_INVALID
    assert _raw_call(al, 2, fc, off, mc, off, fptr=False) == E_INVALID
    assert _raw_call(al, 2, fc, off, mc, off, mptr=False) == E_INVALID
    assert _raw_call(al, 2, fc, None, mc, off) == E_INVALID
    assert _raw_call(al, 2, fc, off, mc, off, mem=abi.MEM_DEVICE_KEPT) == E_INVALID
    check_good(al)
    # refused configurations
    proj = abi.default_slice_config(kind)
    proj.kind, proj.finder = abi.SLICE_P2PLANE, abi.FINDER_PROJECTIVE
    proj.image_rows, proj.image_cols, proj.depth_min, proj.depth_max = 4, 4, 0.1, 10.0
    proj.camera_matrix[0], proj.camera_matrix[4], proj.camera_matrix[8] = 100.0, 100.0, 1.0
    given = cue_config(kind, abi.SLICE_P2P, 0.25)
    given.finder = abi.FINDER_CORRESPONDENCES
    for cfgs in ([proj], [given], [cfg, cue_config(kind, abi.SLICE_P2P, 0.25)]):
        bad = _make(product, kind, cfgs)
        assert _raw_call(bad, 2, fc, off, mc, off) == E_UNSUPPORTED
    al.set_point_shard(lambda op, ptr, count, stream: None, 6_000)
    assert _raw_call(al, 2, fc, off, mc, off) == E_UNSUPPORTED
    al.set_point_shard(None, 0)
    check_good(al)


def test_repeated_calls_and_full_size(product):
    kind = abi.SE3_QUAT_RIGHT
    cfg = cue_config(kind, abi.SLICE_P2PLANE, 0.25, abi.ROBUST_CAUCHY, 0.05, 0.8)
    al = _make(product, kind, [cfg])
    ident = syn.identity(3)
    for K, n, seed in ((3, 4_000, 5500), (9, 1_500, 5510), (1, 30_000, 5520), (17, 700, 5530)):
        pairs = _distinct_3d(K, n, seed)
        res = _pairs(al, pairs, [ident] * K)
        for k in sorted({0, K // 2, K - 1}):
            ref = _single(product, kind, [cfg], pairs[k], ident)
            assert _record(res[k], 3) == _record(ref, 3), (K, k)
    K = 256
    pairs = _distinct_3d(K, 50_000, 5600)
    res = _pairs(al, pairs, [ident] * K)
    assert all(r["status"] == abi.SUCCESS for r in res)
    for k in (0, 77, 180, K - 1):
        assert _record(res[k], 3) == _record(_single(product, kind, [cfg], pairs[k], ident), 3), k


CPP = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;
int main(int argc, char** argv) {
  const int K = 4, n = 2000;
  std::vector<std::vector<float>> F(K), M(K);
  for (int k = 0; k < K; ++k) {
    for (int i = 0; i < n; ++i) {
      const float u = (float) (i % 50) * 0.04f, v = (float) (i / 50) * 0.05f;
      const float x = u, y = v, z = 0.3f * std::sin(2.f * u + (float) k) + 0.2f * std::cos(3.f * v);
      F[k].insert(F[k].end(), {x, y, z});
      M[k].insert(M[k].end(), {x - 0.02f * (k + 1), y + 0.01f, z - 0.01f});
    }
  }
  auto make = []() {
    auto* al = new MultiAligner_<SRRG2_SE3_QUAT_RIGHT>(0);
    srrg2_slice_config c;
    srrg2_slice_default_config(&c, SRRG2_SE3_QUAT_RIGHT);
    c.kind = SRRG2_SLICE_P2P;
    c.finder = SRRG2_FINDER_NN_GATED;
    c.finder_max_distance = 0.2f;
    al->addSlice(c);
    return al;
  };
  std::vector<const float*> fp, mp;
  std::vector<int> fs, ms;
  std::vector<Isometry3f> g(K, Isometry3f::Identity());
  for (int k = 0; k < K; ++k) {
    fp.push_back(F[k].data()); mp.push_back(M[k].data()); fs.push_back(n); ms.push_back(n);
  }
  auto* al = make();
  auto res = al->computeBatchPairs(fp, fs, {}, mp, ms, {}, g);
  int bad = 0;
  for (int k = 0; k < K; ++k) {
    auto* one = make();
    one->setFixed(0, F[k].data(), 12, nullptr, 0, n, SRRG2_MEM_HOST);
    one->setMoving(0, M[k].data(), 12, nullptr, 0, n, SRRG2_MEM_HOST);
    one->setMovingInFixed(g[k]);
    one->compute();
    const auto X = one->movingInFixed();
    if (std::memcmp(X.data(), res[k].moving_in_fixed, sizeof(float) * 12) != 0 || (int) one->status() != res[k].status) ++bad;
    delete one;
  }
  delete al;
  std::printf("pairs %d bad %d\n", K, bad);
  return bad ? 1 : 0;
}
"""


def test_cpp_mirror_compute_batch_pairs(tmp_path):
    src = tmp_path / "pairs.cpp"
    src.write_text(CPP)
    exe = tmp_path / "pairs"
    libdir = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lsrrg2_slam_amd", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pairs 4 bad 0" in out.stdout
