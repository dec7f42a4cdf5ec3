"""No GPU: the register budget of the top-2 matrix-core Hamming kernel (hamming_mfma_kernel in csrc/hamming_mfma.hip), read from the
metadata of the gfx950 assembly.

A SIMD holds 512 vector registers per lane and hands them out in granules of 8. The kernel runs four waves per SIMD; what they leave decides
whether a wave of another stage's kernel (the AKAZE extraction's, 96 registers or fewer) can live beside them for the whole launch or has
to wait until a match workgroup retires. For every instantiation the launchers can pick (PRIO 0..3 x THR false/true):

  - at most 104 VGPRs (APDS_HM_TOP2_VGPRS, stated to the compiler with amdgpu_num_vgpr),
  - no scratch and no spills (a cap the allocator meets by spilling would be worse than no cap),
  - the arithmetic itself: 4 x round_up(vgprs, 8) + 96 <= 512.

tests/test_hamming_mfma_isa.py pins the loop's structure (the looser 128-register bound included); this file pins the budget only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cubesat-apds_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is absent")

CAP = 104            # registers a match wave may hold
GRANULE = 8          # allocation granule, registers per lane
SIMD_FILE = 512      # registers per lane and SIMD
WAVES = 4            # match waves per SIMD (amdgpu_waves_per_eu(4, 4))
GUEST = 96           # what one wave of a co-resident kernel may hold


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile, its variables resolved (ARCH = gfx950, no EXTRA_CXXFLAGS)."""
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = line.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(EXTRA_CXXFLAGS)", "").split()
            assert "-O3" in flags and "--offload-arch=gfx950" in flags
            return flags
    raise AssertionError("no CXXFLAGS in csrc/Makefile")


@pytest.fixture(scope="module")
def top2_metadata(tmp_path_factory):
    """{kernel name: metadata text} of every hamming_mfma_kernel instantiation in the assembly."""
    out = tmp_path_factory.mktemp("budget") / "hamming_mfma.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.check_call([hipcc] + _makefile_flags() + ["-S", "--cuda-device-only", os.path.join(CSRC, "hamming_mfma.hip"), "-o", str(out)],
                          cwd=CSRC, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+).*?\.wavefront_size:\s+\d+", text, re.S)}
    top2 = {n: m for n, m in meta.items() if re.match(r"_ZN4apds\d+hamming_mfma_kernelILi", n)}
    assert len(top2) == 8, sorted(meta)   # PRIO 0..3 x THR
    return top2


def _field(meta, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, meta).group(1))


def test_every_top2_instantiation_holds_at_most_104_registers_without_scratch(top2_metadata):
    for name, meta in sorted(top2_metadata.items()):
        vgprs, agprs = _field(meta, "vgpr_count"), _field(meta, "agpr_count")
        scratch, spills = _field(meta, "private_segment_fixed_size"), _field(meta, "vgpr_spill_count")
        print(f"{name[:48]}: {vgprs} VGPRs ({agprs} of them AGPRs), {scratch} bytes of scratch, {spills} spilled")
        assert vgprs <= CAP, name            # (.vgpr_count is the unified count: it includes the AGPRs)
        assert scratch == 0 and spills == 0, name


def test_four_match_waves_leave_a_96_register_wave_its_room(top2_metadata):
    for name, meta in sorted(top2_metadata.items()):
        allocated = -(-_field(meta, "vgpr_count") // GRANULE) * GRANULE
        assert WAVES * allocated + GUEST <= SIMD_FILE, (name, allocated)


def test_the_cap_in_the_source_is_the_one_checked_here():
    src = open(os.path.join(CSRC, "hamming_mfma.hip")).read()
    m = re.search(r"#define APDS_HM_TOP2_VGPRS \(APDS_HM_WPE == 4 \? (\d+) :", src)
    assert m and int(m.group(1)) == CAP
    assert "amdgpu_num_vgpr(APDS_HM_TOP2_VGPRS / 2)" in src
