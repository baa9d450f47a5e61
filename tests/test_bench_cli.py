"""bench.py's command line around --gpus N: the multi-GPU points of the scaling curve are the driver's to
run; what this repo owns is that the command cannot quietly fall back to one rank and still print a line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**over):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SRRG2_BENCH_SHARE_GPU")}
    env.update(over)
    return env


def test_gpus_n_without_a_launcher_starts_n_ranks_itself():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "3", "--warmup", "1", "--print-launch"],
                         capture_output=True, text=True, timeout=120, env=_env(), cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    cmd = json.loads(out.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(BENCH) + 1:]
    assert tail == ["--gpus", "4", "--steps", "3", "--warmup", "1"]  # the ranks get the same command line


def test_a_launcher_with_another_world_size_is_refused():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "8"], capture_output=True, text=True, timeout=120,
                         env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), cwd=ROOT)
    assert out.returncode != 0 and "WORLD_SIZE=2" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1"], capture_output=True, text=True, timeout=120,
                         env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), cwd=ROOT)
    assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_bare_gpus_2_runs_two_ranks_or_fails_loudly():
    """`python bench.py --gpus 2` with NO launcher: (i) on a one-GPU box it must fail -- never print an n_gpus = 1 line;
    (ii) under the dry-run hook (both ranks on device 0, gloo) it prints ONE line with n_gpus == 2 that says it was a dry run"""
    import torch

    args = [sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--total-alignments", "8",
            "--batch-points", "8000", "--no-one-gpu-reference"]
    if torch.cuda.device_count() < 2:
        out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
        assert out.returncode != 0
        assert "HIP device" in (out.stderr + out.stdout)
        assert not [l for l in out.stdout.splitlines() if l.startswith("{")]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=_env(SRRG2_BENCH_SHARE_GPU="1"), cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["shared_gpu_dry_run"] is True and rec["config"]["alignments_per_step_by_rank"] == [4, 4]


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the result records of the last timed step as .npy files (float32 / float64, well under 64 MB),
    equal to what one compute_batch of the same seeded job returns; --steps sets the number of timed steps and the line
    carries ms_per_step"""
    import numpy as np

    out_dir = tmp_path / "outputs"
    args = [sys.executable, BENCH, "--gpus", "1", "--workload", "c4", "--batch", "8", "--batch-points", "8000",
            "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=_env(), cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and len(rec["step_ms_min_median_max"]) == 3 and rec["ms_per_step"] > 0
    got = {f[:-len(".npy")]: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert all(f.endswith(".npy") for f in os.listdir(out_dir))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the same job in this process, through the host-memory entry point
    import srrg2_slam_interfaces_amd as pkg
    from srrg2_slam_interfaces_amd import _abi as abi
    from srrg2_slam_interfaces_amd import synthetic as syn

    sys.path.insert(0, ROOT)
    import bench

    probs = syn.batch_3d(K=8, n=8000, seed=4000, shared_fixed_group=1 << 30)
    al = bench.make_aligner(lambda: pkg.MultiAligner(abi.SE3_QUAT_RIGHT, device=0), abi, 10)
    al.set_fixed(0, probs[0]["fixed"], probs[0]["fixed_normals"])
    res = al.compute_batch([p["moving"] for p in probs], [syn.identity(3)] * 8, [p["moving_normals"] for p in probs])
    assert got["moving_in_fixed"].dtype == np.float32
    assert got["moving_in_fixed"].tobytes() == np.ascontiguousarray(res.moving_in_fixed, np.float32).tobytes()
    assert np.array_equal(got["status"], res.status.astype(np.float64)) and not got["status"].any()
    assert np.array_equal(got["num_iterations"], res.num_iterations.astype(np.float64))
    assert np.array_equal(got["num_inliers"], res.last["num_inliers"].astype(np.float64))
    assert got["chi_inliers"].tobytes() == res.last["chi_inliers"].astype(np.float32).tobytes()
    H = np.asarray(res.information, np.float32)
    assert np.array_equal(got["information"], np.triu(H) + np.transpose(np.triu(H, 1), (0, 2, 1)))


def _one_line(args, env=None):
    out = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env or _env(), cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_full_reaches_every_rank():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "3", "--warmup", "1", "--full", "--print-launch"],
                         capture_output=True, text=True, timeout=120, env=_env(), cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    cmd = json.loads(out.stdout.strip().splitlines()[-1])["launch"]
    assert cmd[cmd.index(BENCH) + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1", "--full"]


@pytest.mark.gpu
def test_plain_run_measures_the_headline_alone_and_full_the_rest():
    """`bench.py --gpus 1 --steps K --warmup W` (no --workload: C2) prints the headline and nothing that takes runs of its
    own; --full adds the long run, the profiled roofline, the fresh-fixed-cloud figure and the CPU baseline (small clouds)"""
    plain = _one_line([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--points", "8000"])
    assert set(plain) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "step_ms_min_median_max",
                          "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
    assert plain["metric"] == "icp_iterations_per_sec" and plain["unit"] == "iterations/s" and plain["dtype"] == "f32"
    assert plain["higher_is_better"] is True and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["all_success"] is True
    full = _one_line([sys.executable, BENCH, "--gpus", "1", "--workload", "c2", "--steps", "3", "--warmup", "1", "--points", "8000",
                      "--full", "--cpu-seconds", "1", "--no-cpu-all-cores"])
    assert set(plain) <= set(full)
    assert full["long_run"]["steps"] >= 200 and full["value_long"] > 0
    assert full["roofline"]["launches_timed"] > 0 and full["roofline"]["achieved"] > 0
    assert full["c2_fresh_fixed"]["ms_per_step"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["parity_indices_bit_exact_and_X_within_1e-5"] is True


@pytest.mark.gpu
def test_full_multi_rank_run_carries_the_one_gpu_reference():
    """--full at N > 1 (two ranks on device 0 over gloo, the dry-run hook): rank 0 runs the whole job alone after the timed
    region, and the line carries that reference and the strong-scaling ratio"""
    rec = _one_line([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--total-alignments", "8",
                     "--batch-points", "8000", "--full"], env=_env(SRRG2_BENCH_SHARE_GPU="1"))
    assert rec["n_gpus"] == 2 and rec["config"]["all_success"] is True and rec["roofline"]["launches_timed"] > 0
    assert rec["one_gpu_same_job"]["value"] > 0 and rec["strong_scaling_speedup"] > 0
