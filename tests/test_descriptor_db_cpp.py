"""The C++ mirror of the descriptor database (srrg2_slam_amd::DescriptorDatabase in include/srrg2_slam_amd.hpp):
a small program compiled with g++ against the C ABI library, run on the GPU, compared with the numpy restatement."""
import os
import subprocess

import numpy as np
import pytest

import hbst_restatement as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBD = os.path.join(ROOT, "srrg2_slam_interfaces_amd", "lib")

PROGRAM = r'''
#include <cstdio>
#include <fstream>
#include <vector>
#include "srrg2_slam_amd.hpp"

static std::vector<uint8_t> rows(std::ifstream& f, int& n) {
  f.read(reinterpret_cast<char*>(&n), sizeof(n));
  std::vector<uint8_t> d((size_t) n * SRRG2_DESCRIPTOR_BYTES);
  f.read(reinterpret_cast<char*>(d.data()), (std::streamsize) d.size());
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int maps = 0;
  f.read(reinterpret_cast<char*>(&maps), sizeof(maps));
  srrg2_slam_amd::DescriptorDatabase db(0);
  for (int r = 0; r < maps; ++r) {
    int n = 0;
    std::vector<uint8_t> d = rows(f, n);
    std::printf("add %d\n", db.add(d.data(), nullptr, n));
  }
  int nq = 0;
  std::vector<uint8_t> q = rows(f, nq);
  std::printf("size %d %lld\n", db.size(), (long long) db.numDescriptors());
  for (const auto& c : db.match(q.data(), nullptr, nq, db.size(), 25.0f, 1, 2)) {
    std::printf("cand %d %lld\n", c.index, (long long) c.num_matches);
    for (const auto& k : c.correspondences) std::printf("corr %d %d %g\n", k.fixed_idx, k.moving_idx, k.response);
  }
  for (long long c : db.mapCounts()) std::printf("count %lld\n", c);
  try {
    db.match(q.data(), nullptr, -1, 0);
  } catch (const std::runtime_error&) {
    std::printf("invalid refused\n");
  }
  return 0;
}
'''


@pytest.mark.gpu
def test_cpp_descriptor_database_matches_the_restatement(tmp_path, product):
    rng = np.random.default_rng(41)
    maps = [hr.random_descriptors(rng, s) for s in (5, 300, 0, 64, 1000)]
    q = hr.random_descriptors(rng, 1500)
    flat = np.concatenate([m for m in maps if len(m)])
    for i in rng.choice(1500, 700, replace=False):
        q[i] = hr.flip_bits(rng, flat[rng.integers(0, len(flat))], int(rng.integers(0, 30)))
    blob = [np.int32(len(maps)).tobytes()]
    for m in maps + [q]:
        blob += [np.int32(len(m)).tobytes(), m.tobytes()]
    data = tmp_path / "in.bin"
    data.write_bytes(b"".join(blob))
    src, exe = tmp_path / "db.cpp", tmp_path / "db"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", LIBD, "-lsrrg2_slam_amd", "-Wl,-rpath," + LIBD])
    out = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr

    ref = hr.RestatedDatabase()
    expect = ["add %d" % ref.add(m) for m in maps]
    expect.append("size %d %d" % (len(ref.maps), sum(len(m[0]) for m in ref.maps)))
    r = ref.match(q, None, len(ref.maps), 25.0, 1, 2)
    for k, cnt, c in zip(r["indices"], r["num_matches"], r["correspondences"]):
        expect.append("cand %d %d" % (k, cnt))
        expect += ["corr %d %d %g" % (a, b, d) for a, b, d in c.tolist()]
    expect += ["count %d" % r["map_counts"][k] for k in sorted(r["map_counts"])]
    expect.append("invalid refused")
    assert out.stdout.splitlines() == expect
    assert len(r["indices"]) >= 2
