"""The C++ mirror of srrg2_scene_voxelize (Scene::voxelize in include/srrg2_slam_amd.hpp): one small translation unit compiled
with plain g++ against include/ and linked with the built library.  Compiling and linking need no GPU; the GPU leg runs
set -> voxelize -> estimateNormals -> setFixed / setMoving -> compute() through the mirror and prints bit patterns, which must be
those of the restatements (tests/voxel_restatement.py, tests/normals_restatement.py) and of the oracle's alignment of the
restatement-made clouds."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

SOURCE = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "srrg2_slam_amd.hpp"
using namespace srrg2_slam_amd;

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static void dump(const char* tag, const float* v, size_t n) {
  std::printf("%s", tag);
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &v[i], 4);
    std::printf(" %08x", u);
  }
  std::printf("\n");
}

static void dump_ints(const char* tag, const std::vector<int32_t>& v) {
  std::printf("%s", tag);
  for (int32_t i : v) std::printf(" %d", i);
  std::printf("\n");
}

static bool read_cloud(std::FILE* f, std::vector<float>& pts) {
  int32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n <= 0) return false;
  pts.resize((size_t) n * 3);
  return std::fread(pts.data(), 4, pts.size(), f) == pts.size();
}

int main(int argc, char** argv) {
  if (argc < 2 || !std::strcmp(argv[1], "link-only")) return 0;  // (link check only)
  std::FILE* f = std::fopen(argv[1], "rb");
  REQUIRE(f);
  float leaf = 0.f, radius = 0.f, gate = 0.f, view[3];
  REQUIRE(std::fread(&leaf, 4, 1, f) == 1 && std::fread(&radius, 4, 1, f) == 1 && std::fread(&gate, 4, 1, f) == 1);
  REQUIRE(std::fread(view, 4, 3, f) == 3);
  std::vector<float> cloud[2];
  REQUIRE(read_cloud(f, cloud[0]) && read_cloud(f, cloud[1]));
  std::fclose(f);

  srrg2_voxel_params vp;
  srrg2_voxel_default_params(&vp);
  REQUIRE(vp.leaf_size == 0.05f && vp.mode == SRRG2_VOXEL_CENTROID && vp.min_points_per_voxel == 1);
  REQUIRE(vp.origin[0] == 0.f && vp.origin[1] == 0.f && vp.origin[2] == 0.f && vp.reserved[0] == 0 && vp.reserved[1] == 0);
  vp.leaf_size = leaf;
  srrg2_normals_params np;
  srrg2_normals_default_params(&np, 3);
  np.radius = radius;
  for (int d = 0; d < 3; ++d) np.viewpoint[d] = view[d];

  Scene<3> full[2], dec[2];
  const char* names[2] = {"map", "meas"};
  char tag[64];
  for (int k = 0; k < 2; ++k) {
    const int n = (int) cloud[k].size() / 3;
    full[k].set(cloud[k].data(), 12, nullptr, 0, n);
    std::vector<int32_t> counts;
    const srrg2_voxel_result r = full[k].voxelize(vp, dec[k], &counts);
    REQUIRE(r.num_points == n && r.num_voxels == dec[k].size() && (int) counts.size() == r.num_voxels && full[k].size() == n);
    std::vector<float> c, m;
    dec[k].get(c, m);
    std::snprintf(tag, sizeof(tag), "%s_points", names[k]);
    dump(tag, c.data(), c.size());
    std::snprintf(tag, sizeof(tag), "%s_counts", names[k]);
    dump_ints(tag, counts);
    std::snprintf(tag, sizeof(tag), "%s_gidx", names[k]);
    dump_ints(tag, dec[k].globalIndices());
    std::printf("%s_result %d %d %d %d %d %d\n", names[k], r.num_points, r.num_finite, r.num_occupied, r.num_voxels,
                r.num_with_normal, r.max_points_per_voxel);
    const srrg2_normals_result nr = dec[k].estimateNormals(np);
    dec[k].get(c, m);
    std::snprintf(tag, sizeof(tag), "%s_normals", names[k]);
    dump(tag, m.data(), m.size());
    std::printf("%s_size %d\n", names[k], nr.scene_size);
  }
  // refused: dst keeps its content
  const int before = dec[0].size();
  bool thrown = false;
  vp.leaf_size = 0.f;
  try { full[0].voxelize(vp, dec[0]); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown && dec[0].size() == before);
  thrown = false;
  vp.leaf_size = leaf;
  try { full[0].voxelize(vp, full[0]); } catch (const std::exception&) { thrown = true; }
  REQUIRE(thrown);

  using Aligner = MultiAligner_<SRRG2_SE3_QUAT_RIGHT>;
  Aligner al(0);
  srrg2_slice_config cfg = Aligner::defaultSliceConfig();
  cfg.kind = SRRG2_SLICE_P2PLANE;
  cfg.finder = SRRG2_FINDER_NN_GATED;
  cfg.finder_max_distance = gate;
  cfg.robustifier = SRRG2_ROBUST_CAUCHY;
  cfg.robustifier_chi_threshold = 0.05f;
  cfg.finder_normal_cos = -2.f;
  cfg.min_num_correspondences = 0;
  const int si = al.addSlice(cfg);
  const float *mp, *mn, *fp, *fn;
  int nm = 0, nf = 0;
  dec[0].deviceArrays(mp, mn, nm);
  dec[1].deviceArrays(fp, fn, nf);
  REQUIRE(mn && fn);
  al.setFixed(si, fp, 16, fn, 16, nf, SRRG2_MEM_DEVICE);
  al.setMoving(si, mp, 16, mn, 16, nm, SRRG2_MEM_DEVICE);
  al.setMovingInFixed(Isometry<3>::Identity());
  al.compute();
  const Isometry<3>& X = al.movingInFixed();
  dump("estimate", X.data(), 12);
  std::printf("run %d %d %d\n", (int) al.status(), (int) al.iterationStats().size(),
              al.iterationStats().empty() ? -1 : al.iterationStats().back().num_correspondences);
  std::printf("ok\n");
  return 0;
}
"""


def _build(tmp_path):
    src = tmp_path / "voxel.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "voxel"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", LIBDIR, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBDIR, "-o", str(exe)])
    return str(exe)


def test_cpp_voxelize_compiles_and_links(tmp_path):
    exe = _build(tmp_path)
    assert subprocess.run([exe, "link-only"], timeout=120).returncode == 0


def test_the_case_is_not_vacuous():
    import voxel_cases as vc

    P, M = vc.clouds(3)
    v, nrm = vc.restated(P, 3)
    n, m = len(P), v["result"]["num_voxels"]
    assert n // 4 < m < 3 * n // 4 and v["result"]["max_points_per_voxel"] > 3
    assert nrm["result"]["scene_size"] > 0.9 * m


def _floats(line):
    return np.array([int(w, 16) for w in line.split()[1:]], np.uint32).view(np.float32)


def _ints(line):
    return np.array([int(w) for w in line.split()[1:]], np.int64)


@pytest.mark.gpu
def test_cpp_voxelize_through_the_stack(product, oracle, tmp_path):
    import normals_restatement as nr
    import voxel_cases as vc

    P, M = vc.clouds(3)
    path = tmp_path / "clouds.bin"
    with open(path, "wb") as f:
        f.write(np.array([vc.LEAF, vc.RADIUS, vc.GATE, *vc.VIEW], np.float32).tobytes())
        for c in (P, M):
            f.write(np.int32(len(c)).tobytes())
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
    out = subprocess.run([_build(tmp_path), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]
    lines = {l.split()[0]: l for l in out.stdout.splitlines() if l.strip()}
    want = {}
    for name, cloud in (("map", P), ("meas", M)):
        v, n = vc.restated(cloud, 3)
        want[name] = n
        assert nr.same_bits(_floats(lines[name + "_points"]).reshape(-1, 3), v["points"]), name
        assert np.array_equal(_ints(lines[name + "_counts"]), v["counts"]) and np.array_equal(_ints(lines[name + "_gidx"]), v["global_indices"])
        res = v["result"]
        assert list(_ints(lines[name + "_result"])) == [res[k] for k in (
            "num_points", "num_finite", "num_occupied", "num_voxels", "num_with_normal", "max_points_per_voxel")]
        assert nr.same_bits(_floats(lines[name + "_normals"]).reshape(-1, 3), n["normals_out"]), name
        assert int(lines[name + "_size"].split()[1]) == n["result"]["scene_size"]
    ref = vc.oracle_run(oracle, 3, want["meas"], want["map"])
    status, iterations, ncorr = (int(w) for w in lines["run"].split()[1:])
    assert status == ref.status() and iterations == len(ref.iteration_stats())
    assert ncorr == ref.iteration_stats()[-1]["num_correspondences"] > len(want["map"]["points_out"]) // 2
    assert _floats(lines["estimate"]).tobytes() == np.ascontiguousarray(ref.moving_in_fixed(), np.float32).tobytes()
