"""Inputs of the estimator border tests: shared by test_estimator_borders_gpu.py (HIP path against the oracle) and
test_estimator_border_inputs_cpu.py (the oracle alone: does every input sit on the border it names?). Not a test module.

Every number below is derived from a named constant of csrc/homography.hip, csrc/homography_refit.hip, csrc/homography.h,
csrc/homography_rho.hip or csrc/pnp.hip, and update_num_iters restates csrc/ransac_loop.h; the constants are restated here so that a
change of one of them in the source shows up against this table in review."""
import numpy as np

# ---- csrc/homography.h, csrc/homography_refit.hip --------------------------------------------------------------------------------------
HOST_REFIT_MAX = 256                       # homography.h: refit on the host up to this many selected points, reduce_kernel above
RED_BLOCKS, RED_THREADS = 64, 256          # homography_refit.hip: reduce_kernel's grid
RED_STRIDE = RED_BLOCKS * RED_THREADS      # 16384: thread (b, t) adds the points b * 256 + t + 16384 j
# ---- csrc/homography.hip ---------------------------------------------------------------------------------------------------------------
HT = 8                                     # hypotheses per block of score_kernel
COOP_PER_BLOCK = 16                        # models per block of hypothesis_coop_kernel
RANSAC_FIRST_BATCH = 512                   # config().ransac_batch (APDS_RANSAC_BATCH's default, csrc/runtime.cpp)
RANSAC_MAX_BATCH = 4096                    # ransac(): max_batch's cap
SCORE_THREADS = 256                        # score_kernel / pnp_score_kernel: points per pass of a part
KTH_THREADS = 1024                         # kth_select_kernel's block
# ---- csrc/homography_rho.hip -----------------------------------------------------------------------------------------------------------
RHO_WORD, RHO_BLOCK, RHO_GRID_CAP = 64, 256, 1024
RHO_GRID_POINTS = RHO_BLOCK * RHO_GRID_CAP  # 262144: above this rho_inlier_bits_kernel's blocks take a second stride
# ---- csrc/pnp.hip ----------------------------------------------------------------------------------------------------------------------
PNP_HT = 4                                 # hypotheses per block of pnp_score_kernel
PNP_THREADS = 32                           # models per block of pnp_hypothesis_kernel (EPnP)
P3P_THREADS = 64                           # models per block of p3p_hypothesis_kernel (P3P, AP3P)
PNP_BATCH = 2048                           # config().pnp_batch (pnp_ransac_core: batch)

LMEDS, RANSAC, RHO = 4, 8, 16


def ransac_batch_sizes(max_iters):
    """first_batch, max_batch of csrc/homography.hip's ransac()"""
    first = max(8, min(RANSAC_FIRST_BATCH, max(max_iters, 8)))
    return first, max(first, min(RANSAC_MAX_BATCH, max(max_iters, 8)))


def pnp_batch_size(iterations):
    """batch of csrc/pnp.hip's pnp_ransac_core, the first and every later batch alike"""
    return max(PNP_HT, min(PNP_BATCH, max(iterations, 1)))


def ransac_batches(max_iters, sizes=None):
    """The batch sizes B that speculative_ransac (csrc/ransac_loop.h) hands to find_homography_device's launches while the budget stays at
    max_iters (first_batch / max_batch / the loop's `iter + B < niters`), and the point parts of each score_kernel launch. sizes: another
    (first, later) pair, e.g. PnP's."""
    first, cap = sizes or ransac_batch_sizes(max_iters)
    out, it = [], 0
    while it < max(max_iters, 1):
        B = min(first if it == 0 else cap, max(max_iters, 1) - it)
        out.append(B)
        it += B
    return out


def score_parts(B, ht=HT):
    """`parts` of the scoring launch: max(1, min(64, ceil(256 * 8 / ceil(B / HT))))"""
    return max(1, min(64, -(-256 * 8 // -(-B // ht))))


def update_num_iters(p, ep, model_points, max_iters):
    """cv::RANSACUpdateNumIters (ptsetreg.cpp), restated from OpenCV (the product's: update_num_iters in csrc/ransac_loop.h)"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, np.finfo(np.float64).tiny)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < np.finfo(np.float64).tiny:
        return 0
    num, denom = np.log(num), np.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


# ---- homography inputs -----------------------------------------------------------------------------------------------------------------
def planted_set(synth, n, inlier_idx, seed, extent, noise=0.0):
    """n pairs on one homography (noise-free unless asked), every pair outside inlier_idx pushed 30 to 80 pixels off it: the inlier set of a
    threshold of a few pixels is inlier_idx exactly, whatever model of the inliers the estimator ends on."""
    src, dst, H, _ = synth.make_ransac_set(n, seed=seed, inlier_frac=1.1, noise=noise, extent=extent)
    flag = np.zeros(n, bool)
    flag[np.asarray(inlier_idx)] = True
    rng = np.random.default_rng(seed)
    ang, rad = rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 80, n)
    off = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np.float32)
    dst = dst.copy()
    dst[~flag] += off[~flag]
    return src, dst, flag


# HOST_REFIT_MAX by inlier count: (method, n, inliers, extent). LMEDS cuts at max(2.5 * 1.4826 * ... * sqrt(median), 0.001) pixels, and the
# median of noise-free inliers is binary32 rounding: with coordinates below 128 that rounding (~1e-5 px) stays far under the 0.001 floor,
# so all planted inliers pass; RANSAC's 3 px threshold does not care about the extent.
EXACT_INLIER_CASES = [(RANSAC, 400, HOST_REFIT_MAX, 1024.0), (RANSAC, 400, HOST_REFIT_MAX + 1, 1024.0),
                      (LMEDS, 400, HOST_REFIT_MAX, 64.0), (LMEDS, 400, HOST_REFIT_MAX + 1, 64.0)]


def exact_inlier_set(synth, method, n, count, extent):
    seed = 0xB0DE0000 + 16 * count + method
    idx = np.random.default_rng(seed ^ 0x55).permutation(n)[:count]
    return planted_set(synth, n, idx, seed, extent)


# Reduction mask in one block. The issue asks for n = 20000 with ~300 inliers that all have index below 256. That set cannot exist: only
# 256 indices lie below 256, and RANSAC draws its samples uniformly over n, so 300 inliers in 20000 give an all-inlier sample with
# probability (300 / 20000)^4 = 5e-8 per iteration. More generally a block of reduce_kernel owns 256 indices per RED_STRIDE, so a selection
# of more than HOST_REFIT_MAX points inside one block needs n > RED_STRIDE and an inlier share of at most 512 / 16640 = 3 %, which neither
# RANSAC nor LMEDS reaches in a budget the oracle can walk. The nearest reachable case: n = 1200 (blocks 0 to 4 own points, blocks 5 to 63
# own none), the 300 inliers at indices 0 to 299, i.e. block 0 full, block 1 up to thread 43, and blocks 2, 3, 4 iterate over points
# that the mask switches off - partial sums of exact zeros from both kinds of empty block.
MASK_BLOCK_N, MASK_BLOCK_INLIERS = 1200, HOST_REFIT_MAX + 44


def mask_block_set(synth):
    return planted_set(synth, MASK_BLOCK_N, np.arange(MASK_BLOCK_INLIERS), 0xB10C, 1024.0)


# Scoring tails: max_iters -> batches B (ransac_batches): 1 -> [1]; 7 -> [7]; 8 -> [8]; 9 -> [9]; 17 -> [17]; 513 -> [512, 1];
# 4097 + 5 -> [512, 3590]; 512 + 4096 + 3 -> [512, 4096, 3] (the only one in which max_batch's cap binds). B % HT = 1, 7, 0, 1, 1, (0, 1),
# (0, 6), (0, 0, 3); B % COOP_PER_BLOCK = 1, 7, 8, 9, 1, (0, 1), (0, 6), (0, 0, 3). parts (score_parts): 64 for B <= 256, 32 for B = 512,
# 5 for B = 3590, 4 for B = 4096, so per = ceil(n / parts) is 5 / 9 / 52 / 65 for n = 257, 16 / 32 / 200 / 250 for n = 1000 and
# 33 / 65 / 410 / 513 for n = 2049: never a multiple of SCORE_THREADS, and at n = 2049 more than one pass per part.
SCORE_TAIL_ITERS = [1, 7, 8, 9, 17, RANSAC_FIRST_BATCH + 1, RANSAC_MAX_BATCH + 1 + 5, RANSAC_FIRST_BATCH + RANSAC_MAX_BATCH + 3]
SCORE_TAIL_N = [SCORE_THREADS + 1, 1000, 8 * SCORE_THREADS + 1]
# For the one-batch budgets the seed is chosen (tools: a loop over seeds on the oracle) so that the LAST hypothesis of the budget is the one
# RANSAC ends on - the hypothesis whose index the `min(h0 + h, B - 1)` clamp and the `h0 + h < B` guard decide. The CPU file asserts it.
SCORE_TAIL_SEEDS = {
    (7, 257): 0x5C0E057C, (7, 1000): 0x5C0E05AD, (7, 2049): 0x5C0E09D8,
    (8, 257): 0x5C0E0457, (8, 1000): 0x5C0E0678, (8, 2049): 0x5C0E0A01,
    (9, 257): 0x5C0E03AB, (9, 1000): 0x5C0E062D, (9, 2049): 0x5C0E0A44,
    (17, 257): 0x5C0E055A, (17, 1000): 0x5C0E082B, (17, 2049): 0x5C0E0C55,
}
LAST_WINS_ITERS = [7, 8, 9, 17]


def score_tail_cases():
    return [(k, n) for k in SCORE_TAIL_ITERS for n in SCORE_TAIL_N if k <= RANSAC_MAX_BATCH + 6 or n == SCORE_TAIL_N[0]]


def score_tail_set(synth, max_iters, n):
    seed = SCORE_TAIL_SEEDS.get((max_iters, n), 0x5C0E0000 + 64 * max_iters + n)
    src, dst, _, _ = synth.make_ransac_set(n, seed=seed, inlier_frac=0.1, noise=0.5, extent=1024.0)
    return src, dst


SCORE_TAIL_THR, SCORE_TAIL_CONF = 3.0, 0.995

# LMEDS select: kth_select_kernel's block of KTH_THREADS strides over n, kth = n / 2
LMEDS_N = [5, 6, KTH_THREADS - 1, KTH_THREADS, KTH_THREADS + 1, 2 * KTH_THREADS - 1, 2 * KTH_THREADS, 2 * KTH_THREADS + 1]


def lmeds_set(synth, n):
    src, dst, _, _ = synth.make_ransac_set(n, seed=0x1ED50000 + n, inlier_frac=1.1 if n < 10 else 0.75, noise=0.3, extent=1024.0)
    return src, dst


def lmeds_zero_median_set():
    """Integer source points and an integer translation: binary32 reprojection through a 4-point model of them is exact, every error is
    0.0f, the median is 0.0f and the radix select's prefix stays 0 through its three passes."""
    rng = np.random.default_rng(0x2E80)
    src = rng.permutation(64 * 64)[:600]
    src = np.stack([src % 64, src // 64], 1).astype(np.float32) * 4
    return src, src + np.array([7, -3], np.float32)


def lmeds_ties_set(synth):
    """1500 pairs, 187 distinct ones eight times each and one four times (1500 = 8 * 187 + 4): sorted errors come in runs of eight equal
    values and the k-th (k = 750) lies inside a run."""
    src, dst, _, _ = synth.make_ransac_set(188, seed=0x71E5, inlier_frac=0.75, noise=0.3, extent=1024.0)
    return np.tile(src, (8, 1))[:1500].copy(), np.tile(dst, (8, 1))[:1500].copy()


def lmeds_minority_set(synth):
    src, dst, _, _ = synth.make_ransac_set(1000, seed=0x3077, inlier_frac=0.3, noise=0.3, extent=1024.0)
    return src, dst


# RHO bit rows: one RHO_WORD-bit word per wave, RHO_BLOCK points per block
RHO_N = [5, RHO_WORD - 1, RHO_WORD, RHO_WORD + 1, RHO_BLOCK - 1, RHO_BLOCK, RHO_BLOCK + 1, 4 * RHO_BLOCK + 1, 16 * RHO_BLOCK + 1]
RHO_STRIDE_N = RHO_GRID_POINTS + RHO_WORD + 1     # 262209: grid-stride path, last block past the last word, n % 64 = 1


def rho_set(synth, n):
    src, dst, _, _ = synth.make_ransac_set(n, seed=0x0B170000 + n, inlier_frac=1.1 if n < 10 else 0.6, noise=0.5, extent=1024.0)
    return src, dst


def rho_on_threshold_set():
    """Distinct integer source points under an integer translation, and every third pair exactly 3 pixels off it along x: for the exact
    translation (which binary32 elimination on these integers returns) their squared error is 9.0f == maxDsq for a threshold of 3, the one
    value at which `<=` and `<` part."""
    rng = np.random.default_rng(0x0E9)
    xs, ys = rng.permutation(512)[:300], rng.permutation(512)[:300]       # no two points share an x or a y (RHO rejects such samples)
    src = np.stack([xs, ys], 1).astype(np.float32)
    dst = src + np.array([16, -8], np.float32)
    dst[2::3, 0] += 3
    return src, dst


FUZZ_N = [5, 8, 30, 200, 3000]
FUZZ_FRAC, FUZZ_NOISE, FUZZ_THR = [0.2, 0.5, 0.9, 1.1], [0.0, 0.3, 1.5], [0.5, 1.0, 3.0, 7.5]
FUZZ_ITERS, FUZZ_CONF, FUZZ_EXTENT = [10, 200, 2000], [0.9, 0.995], [64, 1024, 4096]
RHO_FUZZ_SEED, RHO_FUZZ_CASES = 16, 120


def rho_fuzz_cases(synth):
    """120 seeded RHO cases over test_fuzz_gpu.py::test_homography_random_sets' parameter lists (n without its 4: four pairs never reach
    RHO). Yields (case, src, dst, thr, iters, conf)."""
    rng = np.random.default_rng(RHO_FUZZ_SEED)
    for case in range(RHO_FUZZ_CASES):
        n = int(rng.choice(FUZZ_N))
        frac, noise, thr = float(rng.choice(FUZZ_FRAC)), float(rng.choice(FUZZ_NOISE)), float(rng.choice(FUZZ_THR))
        iters, conf, extent = int(rng.choice(FUZZ_ITERS)), float(rng.choice(FUZZ_CONF)), float(rng.choice(FUZZ_EXTENT))
        src, dst, _, _ = synth.make_ransac_set(n, seed=7000 + case, inlier_frac=frac, noise=noise, extent=extent)
        yield case, src, dst, thr, iters, conf


# ---- PnP inputs ------------------------------------------------------------------------------------------------------------------------
def _rotation(rvec):
    th = np.linalg.norm(rvec)
    k = rvec / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def planar_pnp_set(synth, n, seed, frac, noise, tilt):
    """make_pnp_set's correspondences with the object points pressed onto a plane (optionally tilted and off the origin) and the inliers'
    pixels re-projected from the planted pose (test_pnp_gpu.py's planar construction)."""
    obj, img, K, rvec, tvec, flag = synth.make_pnp_set(n, seed=seed, inlier_frac=frac, noise=noise)
    rng = np.random.default_rng(seed)
    obj = obj.copy()
    obj[:, 2] = 0.0
    if tilt:
        obj = obj @ _rotation(rng.normal(size=3)).T + np.array([3.0, -2.0, 5.0])
    cam = obj[flag] @ _rotation(rvec).T + tvec
    img = img.copy()
    img[flag] = cam[:, :2] / cam[:, 2:3] * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]]) + rng.normal(0, noise, (int(flag.sum()), 2))
    return obj, img, K


PNP_SWEEP_METHODS = ["SOLVEPNP_ITERATIVE", "SOLVEPNP_AP3P", "SOLVEPNP_SQPNP", "SOLVEPNP_IPPE", "SOLVEPNP_IPPE_SQUARE"]
PNP_PLANAR_METHODS = ("SOLVEPNP_IPPE", "SOLVEPNP_IPPE_SQUARE")
PNP_SWEEP_SEED, PNP_SWEEP_CASES = 62, 60


def pnp_sweep_cases(synth):
    """60 seeded cases over test_fuzz_gpu.py::test_pnp_random_sets' parameter lists with the methods that test leaves out, by their
    SolvePnPMethod names. Yields (case, method name, obj, img, K, iters, thr, conf)."""
    rng = np.random.default_rng(PNP_SWEEP_SEED)
    for case in range(PNP_SWEEP_CASES):
        n = int(rng.choice([4, 5, 6, 9, 40, 400, 5000]))
        frac, noise = float(rng.choice([0.3, 0.6, 0.95, 1.1])), float(rng.choice([0.0, 0.4, 2.0]))
        name = str(rng.choice(PNP_SWEEP_METHODS))
        iters, thr, conf = int(rng.choice([5, 100, 1000])), float(rng.choice([1.0, 3.0, 8.0])), float(rng.choice([0.9, 0.99]))
        tilt = bool(rng.integers(0, 2))
        if name in PNP_PLANAR_METHODS:
            obj, img, K = planar_pnp_set(synth, n, 900 + case, frac, noise, tilt)
        else:
            obj, img, K = synth.make_pnp_set(n, seed=900 + case, inlier_frac=frac, noise=noise)[:3]
        yield case, name, obj, img, K, iters, thr, conf


# Border cases of the PnP RANSAC loop (EPnP, P3P, AP3P). One batch of B = iterations hypotheses (iterations <= PNP_BATCH):
# 33 % PNP_HT = 1, 66 % PNP_HT = 2, 131 % PNP_HT = 3, and none of them is a multiple of PNP_THREADS (EPnP) or P3P_THREADS (P3P, AP3P):
# 33 = 32 + 1 = one EPnP block and one thread, 66 = 64 + 2, 131 = 2 * 64 + 3. ceil(B / PNP_HT) <= 33 blocks give parts = 62 to 64, so
# n = 255 / 256 / 257 leaves per = 4 or 5, and n = 64 * SCORE_THREADS + 1 is one past the most a full grid of parts covers in one pass
# (per = 257 at parts = 64: every part runs a second pass for a single point).
PNP_BORDER_METHODS = ["SOLVEPNP_EPNP", "SOLVEPNP_P3P", "SOLVEPNP_AP3P"]
PNP_BORDER_ITERS = [PNP_THREADS + 1, P3P_THREADS + 2, 2 * P3P_THREADS + 3]
PNP_BORDER_N = [SCORE_THREADS - 1, SCORE_THREADS, SCORE_THREADS + 1, 64 * SCORE_THREADS + 1]


def pnp_border_set(synth, n):
    return synth.make_pnp_set(n, seed=0xB0D0 + n, inlier_frac=0.45, noise=0.5)[:3]
