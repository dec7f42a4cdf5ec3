"""Inputs for the AKAZE tie tests: images whose exact symmetry, periodicity or hard edges give many keypoints the SAME response, so that
every order-dependent decision of the detection-to-keypoint tail is actually decided: the strict comparisons of the extremum test
(plateaus, mirrored neighbours), the sequential cross-level suppression ("weaker" between equal responses depends on who comes first), the
max_points cut ("ties by detection order"), the first maximum among equal sector sums of the orientation and the 2 x 2 subpixel solve
whose off-diagonal term is exactly 0. Used by test_akaze_tie_inputs_cpu.py (which shows on the oracle alone that every input ties as much
as it claims and that the cuts land where they claim) and by test_akaze_ties_gpu.py.

Every generator is pure numpy and seeded; `synth` is the package's synth module (make_tile). A case's figures (keypoints, distinct
responses, longest run of equal responses, octaves, number of class_ids) are the oracle's, measured once and kept here as the
precondition the CPU test checks at half their value: they are conditions on the INPUT, the kernels never see them.

Also here: `suppress_depth`, the readiness rule of csrc/akaze_suppress.hip's header restated on candidate planes, and
`suppress_rounds`, a round-by-round model of what suppress_round_body actually does (it lets more candidates through than the header's
rule), both used to find out how many rounds an image's suppression passes need."""
from collections import namedtuple

import numpy as np

# name, make(synth) -> HxW u8, then the oracle's figures for the grey image: keypoints, distinct responses, longest run of equal
# responses, the octaves present and the number of distinct class_ids
Case = namedtuple("Case", "name make kp distinct longest octaves class_ids")


def checkerboard(h, w, cell, shift=0):
    """0 / 255 cells of `cell` pixels; `shift` moves the pattern by that many pixels in x and y (an asymmetric image frame)"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((y + shift) // cell + (x + shift) // cell) & 1) * 255).astype(np.uint8)


def mirror4(t):
    """t and its three flips as a 2 x 2 mosaic: symmetric about both centre lines"""
    return np.ascontiguousarray(np.block([[t, t[:, ::-1]], [t[::-1], t[::-1, ::-1]]]))


def periodic(t, n):
    return np.ascontiguousarray(np.tile(t, (n, n)))


def gaussian_lattice(h, w, pitch, sigma, amplitude=100.0, base=60.0):
    """one Gaussian blob per pitch x pitch cell, centred on the PIXEL pitch // 2 of the cell (a centre between two pixels would make the
    peak a 2 x 2 plateau, which the strict extremum test rejects: no keypoint at all). The neighbours' tails are left out, so every
    cell holds the same bytes."""
    gy = np.exp(-0.5 * (((np.arange(h) % pitch) - pitch // 2) / sigma) ** 2)
    gx = np.exp(-0.5 * (((np.arange(w) % pitch) - pitch // 2) / sigma) ** 2)
    return np.clip(np.rint(base + amplitude * gy[:, None] * gx[None, :]), 0, 255).astype(np.uint8)


def kron_images():
    """(binary 8 px blocks, ternary 16 px blocks), both 384 x 384, drawn one after the other as uint8 from default_rng(4)"""
    rng = np.random.default_rng(4)
    a = np.kron(rng.integers(0, 2, (48, 48), dtype=np.uint8) * np.uint8(255), np.ones((8, 8), np.uint8))
    b = np.kron(rng.integers(0, 3, (24, 24), dtype=np.uint8) * np.uint8(127), np.ones((16, 16), np.uint8))
    return a, b


CASES = [
    Case("checker16_256", lambda synth: checkerboard(256, 256, 16), 576, 4, 242, (0,), 2),
    Case("checker32_256", lambda synth: checkerboard(256, 256, 32), 280, 7, 100, (0, 1), 4),
    Case("checker32_512", lambda synth: checkerboard(512, 512, 32), 1944, 7, 676, (0, 1), 4),
    Case("checker24_384", lambda synth: checkerboard(384, 384, 24), 1160, 2, 676, (0,), 2),
    Case("mirror128", lambda synth: mirror4(synth.make_tile(128, 128, 3, channels=1)), 40, 10, 4, (0, 1), 4),
    Case("mirror160x192", lambda synth: mirror4(synth.make_tile(160, 192, 4, channels=1)), 88, 22, 4, (0, 1), 5),
    Case("periodic96x4", lambda synth: periodic(synth.make_tile(96, 96, 9, channels=1), 4), 174, 27, 12, (0, 1), 4),
    Case("periodic128x3", lambda synth: periodic(synth.make_tile(128, 128, 9, channels=1), 3), 144, 41, 9, (0, 1), 4),
    Case("lattice32", lambda synth: gaussian_lattice(384, 384, 32, 3.0), 164, 2, 100, (0,), 2),
    Case("lattice48", lambda synth: gaussian_lattice(384, 384, 48, 5.0), 88, 3, 36, (0, 1), 3),
    Case("lattice64", lambda synth: gaussian_lattice(384, 384, 64, 8.0), 52, 4, 16, (0, 1), 4),
    Case("kron_binary8", lambda synth: kron_images()[0], 1556, 1334, 17, (0, 1, 2), 9),
    Case("kron_ternary16", lambda synth: kron_images()[1], 1020, 637, 36, (0, 1, 2), 9),
]
CASE = {c.name: c for c in CASES}

# one case of each family as BGR with unequal channels and as BGRA: the same pattern in every channel, scaled by 1, 3/4 and 1/2 and
# rounded. The grey value is then a function of the pattern's value alone, so every symmetry of the pattern survives the grey weights.
COLOUR_OF = ("checker32_256", "mirror128", "periodic96x4", "lattice48", "kron_binary8")


def coloured(g, channels):
    out = np.empty(g.shape + (channels,), np.uint8)
    for c, (num, den) in enumerate(((1, 1), (3, 4), (1, 2))):
        out[..., c] = (g.astype(np.int64) * num * 2 + den) // (2 * den)          # round half up, in integers
    if channels == 4:
        out[..., 3] = 255
    return out


def all_inputs(synth):
    """[(name, image)]: every grey case, then the colour variants `<name>_bgr` and `<name>_bgra`"""
    out = [(c.name, c.make(synth)) for c in CASES]
    grey = dict(out)
    for name in COLOUR_OF:
        out.append((name + "_bgr", coloured(grey[name], 3)))
        out.append((name + "_bgra", coloured(grey[name], 4)))
    return out


ALL_NAMES = [c.name for c in CASES] + [n + s for n in COLOUR_OF for s in ("_bgr", "_bgra")]


def flat_image():
    return np.full((384, 384), 128, np.uint8)


def batch_images(synth):
    """the five same-sized images of the batch test, in its order"""
    return np.stack([CASE["lattice48"].make(synth), flat_image(), CASE["periodic96x4"].make(synth), CASE["kron_binary8"].make(synth),
                     CASE["lattice32"].make(synth)])


# --- ties and cuts -------------------------------------------------------------------------------------------------------------------
def ranked(resp):
    """detection indices in the order of the max_points rule: response descending, ties by detection order (a stable sort)"""
    return np.argsort(-np.asarray(resp, np.float64), kind="stable")


def runs(resp):
    """[(a, b)]: the ranks [a, b) of every run of two or more equal responses in the ranked order"""
    s = np.asarray(resp)[ranked(resp)]
    out, a = [], 0
    for i in range(1, len(s) + 1):
        if i == len(s) or s[i] != s[a]:
            if i - a >= 2:
                out.append((a, i))
            a = i
    return out


def tie_figures(resp):
    """(keypoints, distinct responses, longest run of equal responses)"""
    if len(resp) == 0:
        return 0, 0, 0
    _, counts = np.unique(np.asarray(resp), return_counts=True)
    return len(resp), len(counts), int(counts.max())


def tie_cuts(resp):
    """[(max_points, inside)] from the uncut responses: for the longest run [a, b) of equal responses and for the first run of length
    2 to 4, the cuts a (just before the run), a + 1, (a + b) // 2 and b - 1 (inside it: ranks mp - 1 and mp are equal) and b (just
    after). max_points = 0 means "no limit" and is left out."""
    rs = runs(resp)
    if not rs:
        return []
    picked = [max(rs, key=lambda r: (r[1] - r[0], -r[0]))]
    short = [r for r in rs if 2 <= r[1] - r[0] <= 4 and r != picked[0]]
    if short:
        picked.append(short[0])
    cuts = {}
    for a, b in picked:
        for mp in (a, a + 1, (a + b) // 2, b - 1, b):
            if mp >= 1:
                cuts[mp] = cuts.get(mp, False) or a < mp < b
    return sorted(cuts.items())


def cut_rows(resp, mp):
    """the detection indices that max_points = mp keeps, in output order: the first mp of the stable descending order"""
    return ranked(resp)[:mp] if 0 < mp < len(resp) else np.arange(len(resp))


# --- suppression depth ---------------------------------------------------------------------------------------------------------------
STAMP_PERIOD = 253          # suppress_tail_kernel retires its stamps when round % 253 == 0: a pass needs 254 rounds to get there


def _pass_geometry(phase, lvl, sigma_size, ratio):
    """(other level, diff, search radius in the other level's pixels, interaction distance D in this level's) as suppress_round_body"""
    if phase == 0:
        other = lvl - 1
        diff = ratio[lvl] // ratio[other]
        return other, diff, sigma_size[lvl] * diff, 2 * sigma_size[lvl]
    other = lvl + 1
    diff = ratio[other] // ratio[lvl]
    radius = sigma_size[other]
    return other, diff, radius, (2 * radius + 1) * diff


def suppress_depth(candidates_per_level, sigma_size, ratio, phases=(0, 1)):
    """Rounds per (phase, level) under the readiness rule of akaze_suppress.hip's header: a candidate runs in the first round in which no
    EARLIER (row-major) candidate of its own level within the interaction distance D is still pending, so its depth is 1 + the largest
    depth among those earlier candidates, and a pass needs as many rounds as its deepest candidate. candidates_per_level: one boolean
    plane per level (the oracle's extremum mask); sigma_size, ratio: per level, integers. Passes: phase 0 for levels 1 .. L-1 (against
    the level below), phase 1 for levels 0 .. L-2 (against the level above). This is an UPPER bound on what the kernel needs: see
    suppress_rounds."""
    L = len(candidates_per_level)
    out = {}
    for phase in phases:
        for lvl in (range(1, L) if phase == 0 else range(0, L - 1)):
            D = _pass_geometry(phase, lvl, sigma_size, ratio)[3]
            m = np.asarray(candidates_per_level[lvl]) != 0
            h, w = m.shape
            depth = np.zeros((h + D, w + 2 * D), np.int32)            # padded: row y -> y + D, column x -> x + D
            for y, x in zip(*np.nonzero(m)):                           # row-major
                above = depth[y:y + D, x:x + 2 * D + 1]                # rows y - D .. y - 1, columns x - D .. x + D
                left = depth[y + D, x:x + D]                           # row y, columns x - D .. x - 1
                depth[y + D, x + D] = 1 + max(int(above.max()) if D else 0, int(left.max()) if D else 0)
            out[(phase, lvl)] = int(depth.max())
    return out


def _first_victim(mask, px, py, radius):
    """find_neighbor_point: the first live point, row-major, of the half-open square [-radius, radius) that lies in the disc"""
    h, w = mask.shape
    y0, y1, x0, x1 = max(py - radius, 0), min(py + radius, h), max(px - radius, 0), min(px + radius, w)
    if y0 >= y1 or x0 >= x1:
        return None
    win = mask[y0:y1, x0:x1]
    if not win.any():
        return None
    ys, xs = np.nonzero(win)
    ok = (ys + y0 - py) ** 2 + (xs + x0 - px) ** 2 <= radius * radius
    if not ok.any():
        return None
    i = int(np.argmax(ok))
    return int(ys[i] + y0), int(xs[i] + x0)


def suppress_rounds(mask0_per_level, ldet_per_level, sigma_size, ratio):
    """A round-by-round model of suppress_round_body on the oracle's planes. Returns ({(phase, level): rounds}, final masks).
    mask0_per_level: the extremum masks BEFORE suppression (oracle PLANE_MASK0), ldet_per_level: PLANE_LDET.

    Per round and pending candidate c, on the state at the start of the round: v = the first live keypoint of the other level in c's
    search window. No v: c is finished and never blocks anyone. Otherwise c waits iff an earlier (row-major) candidate of its level
    within D that is still pending has v inside ITS search window; else c runs: it deletes v if its response is greater, and is done.
    (The header's rule ignores v; this one is what the kernel does, and it needs far fewer rounds on a lattice whose windows hold one
    victim each.) The final masks must equal the oracle's PLANE_MASK1: the CPU test asserts that, which ties the model to the
    sequential order it stands for."""
    L = len(mask0_per_level)
    masks = [np.array(m != 0) for m in mask0_per_level]
    rounds = {}
    for phase in (0, 1):
        snap = [m.copy() for m in masks]                                # the iterated levels' snapshots of this phase
        for lvl in (range(1, L) if phase == 0 else range(0, L - 1)):
            other, diff, radius, D = _pass_geometry(phase, lvl, sigma_size, ratio)
            live = masks[other]
            pending = snap[lvl].copy()
            h, w = pending.shape
            cand = list(zip(*np.nonzero(pending)))
            n = 0
            while cand:
                n += 1
                acts, still = [], []
                for y, x in cand:
                    y, x = int(y), int(x)
                    px, py = (x * diff, y * diff) if phase == 0 else (x // diff, y // diff)
                    v = _first_victim(live, px, py, radius)
                    if v is None:
                        acts.append((y, x, None))
                        continue
                    y0, x0, x1 = max(y - D, 0), max(x - D, 0), min(x + D + 1, w)
                    blocked = False
                    for ey, ex in zip(*np.nonzero(pending[y0:y + 1, x0:x1])):
                        ey, ex = int(ey) + y0, int(ex) + x0
                        if not (ey < y or ex < x):
                            continue
                        qx, qy = (ex * diff, ey * diff) if phase == 0 else (ex // diff, ey // diff)
                        dx, dy = v[1] - qx, v[0] - qy
                        if -radius <= dx < radius and -radius <= dy < radius and dx * dx + dy * dy <= radius * radius:
                            blocked = True
                            break
                    if blocked:
                        still.append((y, x))
                    else:
                        acts.append((y, x, v))
                for y, x, v in acts:                                    # the ready ones cannot touch each other's victims
                    pending[y, x] = False
                    if v is not None and ldet_per_level[lvl][y, x] > ldet_per_level[other][v]:
                        live[v] = False
                cand = still
            rounds[(phase, lvl)] = n
    return rounds, masks


def oracle_planes(oracle_mod, img):
    """(mask0 per level, mask1 per level, Ldet per level, sigma_size, ratio) of one oracle run"""
    ref = oracle_mod.akaze(img, keep_planes=True)
    n = len(ref.levels)
    m0 = [ref.plane(i, oracle_mod.PLANE_MASK0) for i in range(n)]
    m1 = [ref.plane(i, oracle_mod.PLANE_MASK1) for i in range(n)]
    ld = [ref.plane(i, oracle_mod.PLANE_LDET) for i in range(n)]
    return m0, m1, ld, [lv["sigma_size"] for lv in ref.levels], [int(lv["ratio"]) for lv in ref.levels]


# --- the deepest suppression inputs found ------------------------------------------------------------------------------------------------
def checker5_128x4096():
    """5-pixel cells: a keypoint at every cell centre of levels 0, 1 and 2, one every 5 pixels along 4096-pixel rows. Under the header's
    rule five passes are chains of more than 800 rounds each (three stamp periods). Under the kernel's rule every candidate runs in
    round 1: the distance-D scan calls nearly every candidate blocked, each has a victim (the same cell's keypoint of the other
    level), and no earlier candidate's search window holds it, so the victim test has to release every one of them. Levels 1 and 2
    are deleted completely, and half of what is left shares one response."""
    return checkerboard(128, 4096, 5)


def blocks_128x4096():
    """binary 4 x 4 blocks: the densest irregular keypoints found, and with them the most rounds under the kernel's rule"""
    rng = np.random.default_rng(1)
    return np.kron(rng.integers(0, 2, (32, 1024), dtype=np.uint8) * np.uint8(255), np.ones((4, 4), np.uint8))


DEEP_IMAGES = {"checker5": checker5_128x4096, "blocks": blocks_128x4096}
