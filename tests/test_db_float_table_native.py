"""The float keypoint table driven by a host that is not Python: tests/cpp/db_float_table_test.cpp, built by g++ against libapds_hip.so (no
torch, no HIP headers). CPU: it compiles and links. GPU: it runs - it builds a float table from the device and from the host, reads
selections and a view's L2 train handle back, streams 12 frames through apds_pipeline_create_table with six selections (two of them empty)
against the serial composition of the public calls, and deletes by image and by id."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "cubesat-apds_amd")


def _build(tmp_path):
    exe = str(tmp_path / "db_float_table_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "db_float_table_test.cpp"), "-o", exe, "-L", LIBDIR, "-lapds_hip",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])
    return exe


def test_float_table_host_compiles_and_links(pkg, tmp_path):
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_a_cpp_host_builds_selects_streams_and_deletes_on_a_float_table(gpu_pkg, tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr[-4000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("... ok") == 5 and "0 failed" in out.stdout
