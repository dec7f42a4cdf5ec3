"""CPU: the extraction plan of the product (csrc/akaze_plan.h: the host arithmetic decided before the first launch), compiled by g++ into
a host-only test library (tests/cpp/akaze_plan_host.cpp).

Levels: for each size the plan's level list equals the oracle's (oracle_akaze_level_info / oracle_akaze_level_tau of a whole oracle
extraction of an image of that size) exactly - w, h, octave, sigma_size, border, nsteps as integers, esigma, etime, ratio and every tau as
float bit patterns. The sizes: one octave (the `lw < 80` stop), two octaves with the stop hit from the other side, odd halves, the smallest
image with four octaves, and an odd one with four.

Area tap tables (no oracle accessor): what the construction implies - at most 4 taps per destination, every offset inside the source, the
weights of a destination sum to 1 within 4 ulp of float (<= 4 weights, each the float rounding of a / cell where the a's sum to cell;
every weight is below 1, so its rounding moves the sum by at most a quarter ulp of 1), and on the exact 2 : 1 case two taps of 0.5.

Launch plan: for every level of those sizes and every value of APDS_LEVEL_FUSE / APDS_LEVEL_STRIP, single and batched, the passes' step
counts sum to nsteps, none exceeds its fuse depth, and the last pass lands in Lt.

Kernel families (plan_extraction / plan_base: the table the extraction driver executes): its invariants under every switch setting
(check_plan in the host program: strip-Hessian levels are a prefix, exactly one pass finishes a level, at most one pass writes the next
octave's start image and only for an exact half, a stream or strips head has no separate smoothing pass, a resampled start image goes to
the plane that makes the last pass land in Lt); a table of the expected choice for every level of six shapes under the default switches and
under every switch set that tests/test_strip_kernels_gpu.py forces, written by hand from the rules; and every size threshold hit exactly and
one pixel below, single and as a batch of four."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (160, 80), (161, 83), (640, 320), (641, 321)]
N_OCTAVES = {(64, 48): 1, (160, 80): 2, (161, 83): 2, (640, 320): 4, (641, 321): 4}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("akaze_plan") / "libakaze_plan_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "cpp", "akaze_plan_host.cpp"), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def LF_MAX_STEPS(plan):
    return plan.akaze_plan_fused_max_steps()   # level_fused_kernel's capacity (csrc/akaze_plan.h; akaze_level_fused.hip asserts its own against it)


def plan_levels(plan, w, h):
    info, finfo, tau = np.zeros((16, 6), np.int32), np.zeros((16, 3), np.float32), np.zeros((16, 64), np.float32)
    n = plan.akaze_plan_levels(w, h, info.ctypes.data_as(C.c_void_p), finfo.ctypes.data_as(C.c_void_p), tau.ctypes.data_as(C.c_void_p))
    return n, info, finfo, tau


@pytest.mark.parametrize("w,h", SIZES)
def test_levels_equal_the_oracle(plan, w, h):
    import oracle
    rng = np.random.default_rng(w * 1000 + h)
    ref = oracle.akaze((rng.random((h, w)) * 255).astype(np.uint8)).levels
    n, info, finfo, tau = plan_levels(plan, w, h)
    assert n == len(ref) == 4 * N_OCTAVES[(w, h)]
    for i, lv in enumerate(ref):
        got = dict(zip(("w", "h", "octave", "sigma_size", "border", "nsteps"), (int(v) for v in info[i])))
        assert got == {k: lv[k] for k in got}, i
        for j, k in enumerate(("esigma", "etime", "ratio")):
            assert finfo[i, j].view(np.uint32) == np.float32(lv[k]).view(np.uint32), (i, k)
        assert len(lv["tau"]) == lv["nsteps"]
        assert np.array_equal(tau[i, :lv["nsteps"]].view(np.uint32), lv["tau"].view(np.uint32)), i


@pytest.mark.parametrize("ssize,dsize", [(161, 80), (83, 41), (641, 320), (160, 80)])
def test_area_tables(plan, ssize, dsize):
    ofs, wgt, cnt = np.full((dsize, 4), -7, np.int32), np.zeros((dsize, 4), np.float32), np.zeros(dsize, np.int32)
    plan.akaze_plan_area_tables(ssize, dsize, ofs.ctypes.data_as(C.c_void_p), wgt.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
    assert cnt.min() >= 1 and cnt.max() <= 4
    ulp = float(np.spacing(np.float32(1.0)))
    for d in range(dsize):
        o, w = ofs[d, :cnt[d]], wgt[d, :cnt[d]]
        assert o.min() >= 0 and o.max() < ssize, d
        assert np.all(np.diff(o) == 1), d                     # consecutive source pixels
        assert abs(float(np.sum(w.astype(np.float64))) - 1.0) <= 4 * ulp, d
        if ssize == 2 * dsize:
            assert list(o) == [2 * d, 2 * d + 1] and list(w) == [0.5, 0.5], d


@pytest.mark.parametrize("w,h", SIZES)
def test_launch_plan(plan, LF_MAX_STEPS, w, h):
    n, info, _, _ = plan_levels(plan, w, h)
    out = np.zeros(4 + 3 * 18, np.int32)
    for level in range(1, n):
        nsteps = int(info[level, 5])
        for batch in (1, 4):
            for level_fuse in (0, 1, 2):
                for level_strip in (0, 1, 2):
                    for fused_max in (LF_MAX_STEPS, 3):
                        launches = plan.akaze_plan_level(w, h, level, batch, level_fuse, level_strip, fused_max, out.ctypes.data_as(C.c_void_p))
                        case = (level, batch, level_fuse, level_strip, fused_max)
                        fuse, fused_level, try_strips = int(out[1]), bool(out[2]), bool(out[3])
                        passes = out[4:4 + 3 * launches].reshape(launches, 3)
                        assert launches >= 1 and int(passes[:, 1].sum()) == nsteps, case
                        assert list(passes[:, 0]) == [int(passes[:q, 1].sum()) for q in range(launches)], case
                        for q in range(launches):
                            depth = fused_max if (q == 0 and fused_level) else fuse
                            assert 1 <= passes[q, 1] <= depth, case
                        assert passes[-1, 2] == 1, case            # the last pass lands in Lt
                        assert list(passes[::-1, 2]) == [(q + 1) % 2 for q in range(launches)], case   # and the passes before it alternate
                        assert fuse in (4, 8) and fused_level == (level_fuse == 2 or (level_fuse == 1 and fuse == 8)), case
                        if try_strips:
                            assert not fused_level and level_strip and passes[0, 1] <= 4, case


# ---- which kernel family serves a level -------------------------------------------------------------------------------------------------
SWITCHES = ("nld_strip", "sf_strip", "base_strip", "level_strip", "level_fuse", "level_stream", "doh_strip", "half_fuse", "fork")
START = ("prev", "written", "half", "area")
SMOOTH = ("-", "tiles", "strips")
HEAD = ("-", "stream", "strips", "fused")


def switches(**kw):
    v = dict.fromkeys(SWITCHES, 1)
    v.update(kw)
    return (C.c_int * 9)(*(v[k] for k in SWITCHES))


def render(out, n, ints):
    """One string per level: Hessian kernel (S strips / F fused), start image (and the plane a resampled one goes to), separate smoothing
    pass, head with its steps, the FED passes behind it (s strips / t tiles, with their steps), H if the last pass writes the half image."""
    lines = []
    for i in range(n):
        doh, start, in_lt, smooth, head, launches, half_pass = (int(v) for v in out[i * ints:i * ints + 7])
        if i == 0:
            lines.append("SF"[1 - doh])
            continue
        passes = out[i * ints + 7:i * ints + 7 + 4 * launches].reshape(launches, 4)
        first = 1 if head else 0
        assert half_pass in (-1, launches - 1), i
        lines.append(" ".join([
            "SF"[1 - doh], START[start] + ((">Lt" if in_lt else ">P") if start >= 2 else ""), SMOOTH[smooth],
            HEAD[head] + str(passes[0, 1]) if head else "-", "+".join("ts"[q[2]] + str(q[1]) for q in passes[first:]) or "-", "H" if half_pass >= 0 else "-"]))
    return lines


def extraction_plan(plan, w, h, batch, sw):
    ints = plan.akaze_plan_ints_per_level()
    out = np.zeros(16 * ints, np.int32)
    n = plan.akaze_plan_extraction(w, h, batch, sw, out.ctypes.data_as(C.c_void_p))
    assert n > 0, "the plan breaks an invariant (see stderr)"
    return render(out, n, ints)


def level_plan(plan, w, h, sigma_size, nsteps, batch, sw):
    ints = plan.akaze_plan_ints_per_level()
    out = np.zeros(2 * ints, np.int32)
    assert plan.akaze_plan_one_level(w, h, sigma_size, nsteps, batch, sw, out.ctypes.data_as(C.c_void_p)) == 2
    return render(out, 2, ints)


@pytest.mark.parametrize("w,h", SIZES + [(512, 512), (1024, 1024), (2048, 2048), (4096, 4096), (3001, 2003)])
def test_plan_invariants_under_every_switch_setting(plan, w, h):
    ints = plan.akaze_plan_ints_per_level()
    out = np.zeros(16 * ints, np.int32)
    for batch in (1, 4):
        for code in range(3 ** 6 * 4):
            v = [code // 3 ** k % 3 for k in range(6)]
            sw = switches(nld_strip=v[0], sf_strip=v[1], level_strip=v[2], level_fuse=v[3], level_stream=v[4], doh_strip=v[5],
                          half_fuse=code // 3 ** 6 % 2, fork=code // 3 ** 6 // 2)
            assert plan.akaze_plan_extraction(w, h, batch, sw, out.ctypes.data_as(C.c_void_p)) > 0, (batch, list(sw))


# The expected choice per level, by hand from the rules (FED steps per level: 3 3 4 | 4 5 6 7 | 8 10 12 14 | 17 20 24 29; a level is small
# up to 2^20 pixels over the batch: groups of up to 8 steps, else up to 4, spread evenly). The shapes: (w, h, batch).
SHAPES = {"512": (512, 512, 1), "1024": (1024, 1024, 1), "2048": (2048, 2048, 1), "4096": (4096, 4096, 1), "odd": (3001, 2003, 1), "4x1024": (1024, 1024, 4)}


def fused(doh, first_start, steps, half, last_smooth=None):
    """an octave of levels with fused heads"""
    rows = [f"{doh} {first_start if j == 0 else 'prev'} - fused{n} - -" for j, n in enumerate(steps)]
    if half:
        rows[-1] = rows[-1][:-1] + "H"
    if last_smooth:
        rows[-1] = rows[-1].replace(" - fused", f" {last_smooth} fused")
    return rows


def tiles(doh, first_start, passes, smooth="tiles"):
    """an octave of levels without a head whose FED passes are given"""
    return [f"{doh} {first_start if j == 0 else 'prev'} {smooth} - {p} -" for j, p in enumerate(passes)]


def heads(doh, first_start, levels):
    """an octave of levels with a stream / strips head: (head, FED passes, half)"""
    return [f"{doh} {first_start if j == 0 else 'prev'} - {hd} {p} {hf}" for j, (hd, p, hf) in enumerate(levels)]


O1_FUSED, O2_FUSED, O3_FUSED = (4, 5, 6, 7), (8, 10, 12, 14), (17, 20, 24, 29)
O1_SMALL, O2_SMALL, O3_SMALL = ("t4", "t5", "t6", "t7"), ("t8", "t5+t5", "t6+t6", "t7+t7"), ("t6+t6+t5", "t7+t7+t6", "t8+t8+t8", "t8+t7+t7+t7")
STRIP_HEADS_O0 = [("strips3", "-", "-"), ("strips3", "-", "-"), ("strips4", "-", "-")]
STRIP_HEADS_O1 = [("strips4", "-", "-"), ("strips3", "s2", "-"), ("strips3", "s3", "-"), ("strips4", "s3", "-")]
STREAM_HEADS_O0 = [("stream3", "-", "-"), ("stream3", "-", "-"), ("stream4", "-", "H")]
STREAM_HEADS_O1 = [("stream4", "-", "-"), ("stream3", "s2", "-"), ("stream3", "s3", "-"), ("stream4", "s3", "-")]


def with_half(levels):
    return levels[:-1] + [levels[-1][:2] + ("H",)]


def default_table(last):
    """default switches; `last`: the separate smoothing pass of the last level (the fork is on) or None (off)"""
    return {
        "512": ["F"] + fused("F", "prev", (3, 3, 4), True) + fused("F", "written", O1_FUSED, True) + fused("F", "written", O2_FUSED, False, last and last["512"]),
        "1024": ["F"] + fused("F", "prev", (3, 3, 4), True) + fused("F", "written", O1_FUSED, True) + fused("F", "written", O2_FUSED, True)
                + fused("F", "written", O3_FUSED, False, last and last["1024"]),
        "2048": ["F"] + heads("F", "prev", STRIP_HEADS_O0) + fused("F", "half>P", O1_FUSED, True) + fused("F", "written", O2_FUSED, True)
                + fused("F", "written", O3_FUSED, False, last and last["2048"]),
        "4096": ["S"] + heads("S", "prev", STREAM_HEADS_O0) + heads("F", "written", with_half(STRIP_HEADS_O1)) + fused("F", "written", O2_FUSED, True)
                + fused("F", "written", O3_FUSED, False, last and last["4096"]),
        "odd": ["F"] + heads("F", "prev", STRIP_HEADS_O0) + heads("F", "area>P", STRIP_HEADS_O1) + fused("F", "area>P", O2_FUSED, True)
               + fused("F", "written", O3_FUSED, False, last and last["odd"]),
        "4x1024": ["F"] + heads("F", "prev", STRIP_HEADS_O0) + fused("F", "half>P", O1_FUSED, True) + fused("F", "written", O2_FUSED, True)
                  + fused("F", "written", O3_FUSED, False, last and last["4x1024"]),
    }


ALL_TILES = dict.fromkeys(SHAPES, "tiles")


def level_fused_table():
    """APDS_LEVEL_FUSE=2 APDS_LEVEL_STRIP=0: a fused head on every level"""
    t = {}
    for name, doh0 in (("512", "F"), ("1024", "F"), ("2048", "F"), ("4096", "S"), ("4x1024", "F")):
        t[name] = [doh0] + fused(doh0, "prev", (3, 3, 4), True) + fused("F", "written", O1_FUSED, True)
        t[name] += fused("F", "written", O2_FUSED, False, "tiles") if name == "512" else fused("F", "written", O2_FUSED, True) + fused("F", "written", O3_FUSED, False, "tiles")
    t["odd"] = ["F"] + fused("F", "prev", (3, 3, 4), False) + fused("F", "area>P", O1_FUSED, False) + fused("F", "area>P", O2_FUSED, True) + fused("F", "written", O3_FUSED, False, "tiles")
    return t


def separate_table(half_fuse):
    """no head anywhere: APDS_LEVEL_FUSE=0 APDS_LEVEL_STRIP=0 APDS_LEVEL_STREAM=0, and with half_fuse = 0 also APDS_DOH_STRIP=0 APDS_HALF_FUSE=0"""
    def h(rows):   # the last level of the octave writes the half image
        return rows[:-1] + [rows[-1][:-1] + "H"] if half_fuse else rows
    after = "written" if half_fuse else "half>P"
    S = "S" if half_fuse else "F"
    return {
        "512": ["F"] + tiles("F", "prev", ("t3", "t3", "t4")) + tiles("F", "half>P", O1_SMALL) + tiles("F", "half>P", O2_SMALL),
        "1024": ["F"] + h(tiles("F", "prev", ("s3", "s3", "s4"))) + tiles("F", after, O1_SMALL) + tiles("F", "half>P", O2_SMALL) + tiles("F", "half>P", O3_SMALL),
        "2048": ["F"] + h(tiles("F", "prev", ("s3", "s3", "s4"), "strips")) + tiles("F", after, ("s4", "t5", "t6", "t7")) + tiles("F", "half>P", O2_SMALL)
                + tiles("F", "half>P", O3_SMALL),
        "4096": [S] + h(tiles(S, "prev", ("s3", "s3", "s4"), "strips")) + h(tiles("F", after, ("s4", "s3+s2", "s3+s3", "s4+s3"), "strips")) + tiles("F", after, O2_SMALL)
                + tiles("F", "half>P", O3_SMALL),
        "odd": ["F"] + tiles("F", "prev", ("s3", "s3", "s4"), "strips") + tiles("F", "area>P", ("s4", "s3+s2", "s3+s3", "s4+s3")) + tiles("F", "area>P", O2_SMALL)
               + tiles("F", "half>P", O3_SMALL),
        "4x1024": ["F"] + h(tiles("F", "prev", ("s3", "s3", "s4"), "strips")) + tiles("F", after, ("s4", "t5", "t6", "t7")) + tiles("F", "half>P", O2_SMALL)
                  + tiles("F", "half>P", O3_SMALL),
    }


def strip_head_table(stream):
    """APDS_LEVEL_STRIP=2 APDS_LEVEL_FUSE=0 with APDS_LEVEL_STREAM=0 (level_strip heads wherever pass 0 has at most 4 steps), or with
    APDS_LEVEL_STREAM=2 APDS_DOH_STRIP=2 (streaming heads there instead, and the streaming Hessian kernel on every level)"""
    o0 = STREAM_HEADS_O0 if stream else STRIP_HEADS_O0
    o0_odd = STREAM_HEADS_O0[:2] + [("stream4", "-", "-")] if stream else STRIP_HEADS_O0
    o1 = STREAM_HEADS_O1 if stream else STRIP_HEADS_O1
    one = [("stream4" if stream else "strips4", "-", "-")]
    after = "written" if stream else "half>P"   # behind an octave that a head finishes: only the streaming head writes the half image
    S = "S" if stream else "F"
    def small_o1(start):   # an octave of 4 5 6 7 steps in groups of up to 8: a head for 4, then tiles
        return heads(S, start, one) + tiles(S, "prev", O1_SMALL[1:])
    return {
        "512": [S] + heads(S, "prev", o0) + small_o1(after) + tiles(S, "half>P", O2_SMALL),
        "1024": [S] + heads(S, "prev", o0) + small_o1(after) + tiles(S, "half>P", O2_SMALL) + tiles(S, "half>P", O3_SMALL),
        "2048": [S] + heads(S, "prev", o0) + small_o1(after) + tiles(S, "half>P", O2_SMALL) + tiles(S, "half>P", O3_SMALL),
        "4096": ["S"] + heads("S", "prev", o0) + heads(S, after, with_half(o1)) + tiles(S, "written", O2_SMALL) + tiles(S, "half>P", O3_SMALL),
        "odd": [S] + heads(S, "prev", o0_odd) + heads(S, "area>P", o1) + tiles(S, "area>P", O2_SMALL) + tiles(S, "half>P", O3_SMALL),
        "4x1024": [S] + heads(S, "prev", o0) + small_o1(after) + tiles(S, "half>P", O2_SMALL) + tiles(S, "half>P", O3_SMALL),
    }


FAMILY_TABLE = [
    # (name, switches, expected levels per shape, expected base stage per shape: 0 the strip pass, 1 the separate kernels)
    ("default, forking", {}, default_table(ALL_TILES), {"512": 1, "1024": 1, "2048": 0, "4096": 0, "odd": 0, "4x1024": 0}),
    ("default, APDS_AKAZE_FORK=0", {"fork": 0}, default_table(None), None),
    ("APDS_NLD_STRIP=2 APDS_SF_STRIP=2 APDS_BASE_STRIP=2", {"nld_strip": 2, "sf_strip": 2, "base_strip": 2},
     default_table({"512": "tiles", "1024": "tiles", "2048": "strips", "4096": "strips", "odd": "strips", "4x1024": "tiles"}), dict.fromkeys(SHAPES, 0)),
    ("APDS_LEVEL_STRIP=2 APDS_LEVEL_FUSE=0 APDS_LEVEL_STREAM=0", {"level_strip": 2, "level_fuse": 0, "level_stream": 0}, strip_head_table(False), None),
    ("APDS_LEVEL_FUSE=2 APDS_LEVEL_STRIP=0 (with and without APDS_FED_SHRINK=0)", {"level_fuse": 2, "level_strip": 0}, level_fused_table(), None),
    ("the round-2 path", {"level_fuse": 0, "level_strip": 0, "doh_strip": 0, "level_stream": 0, "half_fuse": 0}, separate_table(0), None),
    ("APDS_DOH_STRIP=2 APDS_LEVEL_STREAM=2 APDS_LEVEL_STRIP=2 APDS_LEVEL_FUSE=0", {"doh_strip": 2, "level_stream": 2, "level_strip": 2, "level_fuse": 0},
     strip_head_table(True), None),
    ("APDS_LEVEL_FUSE=0 APDS_LEVEL_STRIP=0 APDS_LEVEL_STREAM=0", {"level_fuse": 0, "level_strip": 0, "level_stream": 0}, separate_table(1), None),
]


@pytest.mark.parametrize("name,sw,levels,base", FAMILY_TABLE, ids=[t[0] for t in FAMILY_TABLE])
def test_family_table(plan, name, sw, levels, base):
    for shape, (w, h, batch) in SHAPES.items():
        got = extraction_plan(plan, w, h, batch, switches(**sw))
        assert got == levels[shape], (name, shape, [(i, g, e) for i, (g, e) in enumerate(zip(got, levels[shape])) if g != e])
        if base:
            assert plan.akaze_plan_base(h, w, 4, C.c_longlong(4 * w), C.c_longlong(4096), C.c_longlong(4 * w * h), batch, switches(**sw)) == base[shape], (name, shape)


def test_the_4096_frame_under_the_defaults_reads_as_the_design_says(plan):
    got = extraction_plan(plan, 4096, 4096, 1, switches())
    assert [g.split()[0] for g in got] == ["S"] * 4 + ["F"] * 12                                   # strip Hessian: octave 0
    assert [g.split()[3].rstrip("0123456789") for g in got[1:]] == ["stream"] * 3 + ["strips"] * 4 + ["fused"] * 8
    assert [i for i, g in enumerate(got) if g.endswith("H")] == [3, 7, 11]


@pytest.mark.parametrize("batch", [1, 4])
def test_size_thresholds_exactly_and_one_pixel_below(plan, batch):
    """Every `>=` of the rules: the size that meets it exactly and the one a pixel narrower or lower (w x h over the whole batch)."""
    def lv(w, h, nsteps=4, sigma=2, **sw):
        return level_plan(plan, w, h, sigma, nsteps, batch, switches(**sw))
    def px(log2):   # a level of exactly 2^log2 pixels over the batch, and its width
        w = (1 << log2) // 1024 // batch
        return w, 1024
    # streaming Hessian kernel: 2^23 pixels; 64 x 64 when forced
    w, h = px(23)
    assert lv(w, h)[0] == "S" and lv(w - 1, h)[0] == "F" and lv(w, h - 1)[0] == "F"
    assert lv(64, 64, doh_strip=2)[0] == "S" and lv(63, 64, doh_strip=2)[0] == "F" and lv(64, 63, doh_strip=2)[0] == "F"
    assert lv(w, h, sigma=1)[0] == "F" and lv(w, h, sigma=5)[0] == "F" and lv(w, h, sigma=4)[0] == "S"
    # streaming head: 2^23 pixels; 64 x 32 when forced; level_strip_kernel below it
    assert lv(w, h)[1].split()[3] == "stream4" and lv(w - 1, h)[1].split()[3] == "strips4" and lv(w, h - 1)[1].split()[3] == "strips4"
    forced = dict(level_stream=2, level_strip=2, level_fuse=0)
    assert lv(64, 32, **forced)[1].split()[3] == "stream4" and lv(63, 32, **forced)[1].split()[3] == "strips4" and lv(64, 31, **forced)[1].split()[3] == "strips4"
    assert lv(2, 2, **forced)[1].split()[2:5] == ["-", "strips4", "-"] and lv(1, 2, **forced)[1].split()[2:5] == ["tiles", "-", "t4"]
    assert lv(2, 1, **forced)[1].split()[2:5] == ["tiles", "-", "t4"]
    # fused level up to 2^20 pixels, a strips head from 2^20 on (at exactly 2^20 the level is still small: fused)
    w, h = px(20)
    assert lv(w, h)[1].split()[3] == "fused4" and lv(w + 1, h)[1].split()[3] == "strips4" and lv(w, h + 1)[1].split()[3] == "strips4"
    assert lv(w, h, level_fuse=0)[1].split()[3] == "strips4" and lv(w - 1, h, level_fuse=0)[1].split()[3] == "-" and lv(w, h - 1, level_fuse=0)[1].split()[3] == "-"
    # FED strip passes: 2^20 pixels, at most 4 steps
    off = dict(level_fuse=0, level_strip=0)
    assert lv(w, h, **off)[1].split()[4] == "s4" and lv(w - 1, h, **off)[1].split()[4] == "t4" and lv(w, h - 1, **off)[1].split()[4] == "t4"
    assert lv(w, h, 5, **off)[1].split()[4] == "t5" and lv(w - 1, h, nld_strip=2, **off)[1].split()[4] == "s4"
    # smooth_flow on strips: 2^21 pixels; when forced, an interior tile (131 x 67)
    w, h = px(21)
    assert lv(w, h, **off)[1].split()[2] == "strips" and lv(w - 1, h, **off)[1].split()[2] == "tiles" and lv(w, h - 1, **off)[1].split()[2] == "tiles"
    f2 = dict(sf_strip=2, **off)
    assert lv(131, 67, **f2)[1].split()[2] == "strips" and lv(130, 67, **f2)[1].split()[2] == "tiles" and lv(131, 66, **f2)[1].split()[2] == "tiles"
    # base stage: 2^21 pixels
    def base(rows, cols, ch=1, img=4096, stride=None, **sw):
        stride = stride or cols * ch
        return plan.akaze_plan_base(rows, cols, ch, C.c_longlong(stride), C.c_longlong(img), C.c_longlong(rows * stride), batch, switches(**sw))
    assert base(h, w) == 0 and base(h, w - 1) == 1 and base(h - 1, w) == 1 and base(h, w - 1, base_strip=2) == 0 and base(h, w, base_strip=0) == 1
    assert base(h, w, 4) == 0 and base(h, w, 4, img=4097) == 1 and base(h, w, 3, img=4097) == 0 and base(h, w, 4, stride=4 * w + 2) == 1
