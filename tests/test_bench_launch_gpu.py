"""GPU: bench.py started exactly as the driver starts it.

`python3 bench.py --gpus N` with no launcher around it must spawn its own ranks (child processes of a parent that never touched the
GPU), print ONE JSON line and exit 0. On the one-GPU box the ranks share the card and the collectives go over gloo
(APDS_BENCH_BACKEND=gloo: same choreography, threads, streams and buffers as over RCCL); on an 8-GPU node the same command line with the
default backend is BASELINE config 5. The N = 1 line is checked for the fields the contract names."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout,
                       cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    return p.returncode, lines, p.stderr


def test_bare_two_rank_launch_prints_one_json_line(gpu_pkg):
    rc, lines, err = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--tile", "1024", "--db-rows", "100000", "--no-cpu-baseline"],
                          {"APDS_BENCH_BACKEND": "gloo"})
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["scaling"] == "weak"
    assert out["config"]["homography_found"] is True
    assert out["config"]["db_rows_per_gpu"] == 50000 and out["config"]["frames_per_step"] == 2
    assert out["collectives"]["world"] == 2 and out["collectives"]["ranks_in_group"] == 2 and out["collectives"]["backend"] == "gloo"
    assert out["value"] > 0 and out["roofline"]["frac"] > 0


def test_a_failing_first_transport_is_retried_on_the_second(gpu_pkg):
    """The bare parent starts a fresh set of ranks with --transport torch when the first set (the library's own RCCL communicator) exits
    non-zero; the JSON line says which transport ran and what it fell back from. (Over gloo both map onto host callbacks: what is under
    test is the parent's retry, which never touches the GPU.)"""
    rc, lines, err = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--tile", "1024", "--db-rows", "100000", "--no-cpu-baseline", "--no-host-frames"],
                          {"APDS_BENCH_BACKEND": "gloo", "APDS_BENCH_FAIL_TRANSPORT": "rccl"})
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["collectives"]["transport_requested"] == "torch" and "rccl" in out["collectives"]["fell_back_from"]
    assert out["n_gpus"] == 2 and out["config"]["homography_found"] is True
    assert "starting a fresh set with --transport torch" in err


def test_single_gpu_line_carries_the_contract_fields(gpu_pkg):
    rc, lines, err = _run(["--steps", "3", "--warmup", "1", "--tile", "1024", "--db-rows", "100000", "--no-cpu-baseline", "--host-frames", "--full"])
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["collectives"]["world"] == 1
    assert out["value_host_frames"] and out["value_host_frames"] > 0          # frames uploaded from pinned host memory every step
    assert out["config"]["homography_found"] is True
    assert out["detect_roofline"]["ms_standalone"] > 0                         # --full: the stand-alone extraction probe ran


def test_plain_line_times_the_steps_and_dumps_the_last_step(gpu_pkg, tmp_path):
    """A plain run (no --full) times exactly --steps steps and leaves out what takes runs of its own; --dump-outputs writes the last
    step's result, and a second run with the same arguments writes the same arrays."""
    args = ["--steps", "4", "--warmup", "1", "--tile", "1024", "--db-rows", "100000"]
    runs = []
    for d in ("a", "b"):
        rc, lines, err = _run(args + ["--dump-outputs", str(tmp_path / d)])
        assert rc == 0, err[-3000:]
        assert len(lines) == 1, lines
        runs.append(json.loads(lines[0]))
    out = runs[0]
    assert out["steps"] == 4 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["value"] - 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]            # one frame per step on one GPU
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert out[key] == runs[1][key], key
    assert "cpu_baseline" not in out and "detect_roofline" not in out and out["value_host_frames"] is None
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frame_counts.npy", "homography.npy"] and sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    counts = np.load(tmp_path / "a" / "frame_counts.npy")
    assert counts[0] > 0 and counts[3] == 1.0 and out["config"]["homography_found"] is True
    H = np.load(tmp_path / "a" / "homography.npy")
    assert H.shape == (3, 3) and abs(H[2, 2] - 1.0) < 1e-9
