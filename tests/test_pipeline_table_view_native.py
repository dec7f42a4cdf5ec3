"""The per-frame-view pipeline (apds_pipeline_create_table / apds_pipeline_submit_select, csrc/pipeline.cpp; the select per frame in csrc/pipeline_match.cpp) driven by a host that is not
Python: tests/cpp/pipeline_table_view_test.cpp, built by g++ against libapds_hip.so (no torch, no HIP headers). It fills a table on the
device, streams 12 frames with six different selections (two of them empty) and compares every result with the serial composition of the
one-call entry points on apds_db_select's view."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cubesat-apds_amd")


@pytest.mark.gpu
def test_a_cpp_host_streams_frames_with_per_frame_selections(gpu_pkg, tmp_path):
    exe = str(tmp_path / "pipeline_table_view_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_table_view_test.cpp"), "-o", exe, "-L", LIBDIR, "-lapds_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-4000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("... ok") == 2 and "0 failed" in out.stdout
