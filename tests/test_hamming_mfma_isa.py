"""No GPU: what hipcc generates for the tile loop of the matrix-core Hamming kernels (csrc/hamming_mfma.hip), read from the gfx950 assembly.

The loop's speed rests on three facts of the generated code that the source cannot show and a compiler update can silently undo:
  - four waves per SIMD: at most 128 VGPRs and no scratch, for every instantiation the launchers can pick;
  - the LDS-DMA of the next tile stays in flight while this tile is computed: no `s_waitcnt vmcnt(0)` between the loop's
    global_load_lds and the first MFMA behind them (a builtin-issued DMA got one two instructions later: the compiler cannot tell the
    two LDS buffers apart);
  - and it IS waited for, by the wave that issued it, in front of the barrier that closes the tile (a barrier alone does not wait for
    an LDS-DMA; a ds_read ahead of one returns the old bytes).
Nothing else is pinned: no instruction counts, no register numbers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cubesat-apds_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc is absent")


def _makefile_flags():
    """CXXFLAGS of csrc/Makefile, its variables resolved (ARCH = gfx950, no EXTRA_CXXFLAGS)."""
    for line in open(os.path.join(CSRC, "Makefile")):
        if line.startswith("CXXFLAGS"):
            flags = line.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(EXTRA_CXXFLAGS)", "").split()
            assert "-O3" in flags and "--offload-arch=gfx950" in flags
            return flags
    raise AssertionError("no CXXFLAGS in csrc/Makefile")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel name: (metadata text, [instruction lines])} for every hamming_mfma*_kernel in the assembly."""
    out = tmp_path_factory.mktemp("isa") / "hamming_mfma.s"
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.check_call([hipcc] + _makefile_flags() + ["-S", "--cuda-device-only", os.path.join(CSRC, "hamming_mfma.hip"), "-o", str(out)],
                          cwd=CSRC, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = {m.group(1): m.group(0) for m in re.finditer(r"- \.agpr_count:.*?\.name:\s+(\S+).*?\.wavefront_size:\s+\d+", text, re.S)}
    found = {}
    for m in re.finditer(r"^(_ZN4apds\d+hamming_mfma(?:_topk)?_kernel\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        name = m.group(1)
        found[name] = (meta[name], [ln.strip() for ln in m.group(0).splitlines()[1:] if ln.strip()])
    return found


def _launchable(kernels):
    """hm_scan_device / hm_scan_k_launch pick: top-2 <PRIO 0..3, THR>, top-k <K 4|8, NC 2, PRIO 0|2, THR>."""
    top2 = [n for n in kernels if "hamming_mfma_kernelILi" in n]
    topk = [n for n in kernels if "hamming_mfma_topk_kernelILi" in n]
    assert len(top2) == 8 and len(topk) == 8, sorted(kernels)
    return top2 + topk


def _tile_loop(lines):
    """The instructions of the loop that holds the MFMAs, in the order of the text. The assembly printer marks every basic block of a loop
    in the comment of its label (".LBB17_152: ; =>This Inner Loop Header: Depth=1", "; %bb.153: ; in Loop: Header=BB17_152 Depth=1")."""
    loops, header = {}, None
    for ln in lines:
        block = re.match(r"(?:\.LBB\d+_\d+:|; %bb\.\d+:)(.*)", ln)
        if block:
            own = re.match(r"\.L(BB\d+_\d+):.*This (?:Inner )?Loop Header", ln)
            inside = re.search(r"in Loop: Header=(BB\d+_\d+)", block.group(1))
            header = own.group(1) if own else (inside.group(1) if inside else None)
        elif header and not ln.startswith(";"):
            loops.setdefault(header, []).append(ln.split(";")[0].strip())
    with_mfma = [body for body in loops.values() if any(x.startswith("v_mfma") for x in body)]
    assert len(with_mfma) == 1, f"{len(with_mfma)} loops with MFMAs"
    return [x for x in with_mfma[0] if x]


def test_four_waves_per_simd_and_no_scratch(kernels):
    for name in _launchable(kernels):
        meta, lines = kernels[name]
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", meta).group(1))
        print(f"{name[:60]}: {vgprs} VGPRs, {scratch} bytes of scratch")
        assert vgprs <= 128 and scratch == 0 and spills == 0, name
        assert not any(ln.startswith("scratch_") for ln in lines), name


def test_the_prefetch_is_in_flight_under_the_mfmas_and_waited_for_at_the_barrier(kernels):
    drain = re.compile(r"s_waitcnt\b.*vmcnt\(0\)")
    for name in _launchable(kernels):
        lines = kernels[name][1]
        loop = _tile_loop(lines)
        dma = [i for i, ln in enumerate(loop) if ln.startswith("global_load_lds")]
        assert dma, f"{name}: no LDS-DMA in the tile loop"
        mfma_after = next(i for i, ln in enumerate(loop) if i > dma[-1] and ln.startswith("v_mfma"))
        early = [ln for ln in loop[dma[0]:mfma_after] if drain.match(ln)]
        assert not early, f"{name}: the prefetch is drained in front of the tile's first MFMA: {early}"
        barriers = [i for i, ln in enumerate(loop) if ln.startswith("s_barrier")]
        assert barriers and barriers[-1] > dma[-1], f"{name}: no barrier closes the tile"
        close = barriers[-1]
        assert any(drain.match(ln) for ln in loop[dma[-1]:close]), f"{name}: nothing waits for the LDS-DMA in front of the closing barrier"
        # ... and that wait is the last vector-memory event in front of the barrier: no DMA issued between the two
        wait_at = max(i for i, ln in enumerate(loop[:close]) if drain.match(ln))
        assert not any(ln.startswith("global_load_lds") for ln in loop[wait_at:close]), name
