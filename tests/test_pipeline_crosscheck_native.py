"""The pipeline's cross-check mode (apds_pipeline_set_matcher, csrc/pipeline.cpp; the swapped scan in csrc/pipeline_match.cpp) driven by a host that is not Python:
tests/cpp/pipeline_crosscheck_test.cpp, built by g++ against libapds_hip.so (no torch, no HIP headers). It builds a train set on the
device, sets the matcher, streams 10 frames and compares every result with the one-call functions (apds_dev_crosscheck_match, itself
compared with apds_get_bruteforce_matches, then the point gather and apds_dev_find_homography)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cubesat-apds_amd")


@pytest.mark.gpu
def test_a_cpp_host_streams_frames_through_the_crosscheck_matcher(gpu_pkg, tmp_path):
    exe = str(tmp_path / "pipeline_crosscheck_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_crosscheck_test.cpp"), "-o", exe, "-L", LIBDIR, "-lapds_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-4000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("... ok") == 2 and "0 failed" in out.stdout
