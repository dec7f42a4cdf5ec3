"""GPU: the float pipeline (apds_pipeline_create_float, APDS_PIPELINE_MATCH_L2_RATIO; csrc/pipeline.cpp, csrc/pipeline_match.cpp): M-SURF descriptors, the resident L2
train set's top-2, the L2 ratio filter, then matched points, homography, pose and lens as in every pipeline.

Frames are 256 x 256 (synth.py; about 190 keypoints). Every streamed frame is compared with the serial composition of the public device
calls: apds_dev_akaze_extract_float -> apds_dev_l2_topk (the exact kernel) -> the rule of get_knn_matches_l2 applied to the downloaded
keys on the host (sqrt of d^2 in f32, d0 < d1 * fs in f32, both keys present) -> apds_dev_points_from_matches -> (lens) ->
apds_dev_find_homography and, with pose, apds_dev_pnp_correspondences -> (lens) -> apds_dev_pnp_solver_ransac: counts equal, H / rvec /
tvec bit for bit. DBs of 2, 129 and 3000 rows (the descriptors of the rolled frames first, random unit rows behind them); max_points
forcing K = 1, 128, 129; a frame without keypoints; pose on every DB, a lens on one; the contract errors; no growth over fifty frames; a
byte-row ratio pipeline before and after a float one in the same process."""
import ctypes as C
import gc
from importlib import import_module

import numpy as np
import pytest

import lens_reference as lr

pytestmark = pytest.mark.gpu

T = 256
FS, THR, ITERS, CONF = 0.8, 3.0, 2000, 0.995
KMAT = np.array([[900.0, 0, 128], [0, 900.0, 128], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)
DB_SIZES = [2, 129, 3000]
ORDER = [0, 1, 2, 1, 0, 0]            # frame 2 has no keypoints
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


class Scene:
    def __init__(self, pkg):
        import torch
        self.torch, self.pkg, self.pl = torch, pkg, import_module(pkg.__name__ + ".pipeline")
        fe, synth = pkg.feature_extraction, pkg.synth
        self.tiles = [synth.make_tile(T, T, frame_index=70 + i, blobs_per_mpx=20000) for i in range(2)]
        blank = np.zeros_like(self.tiles[0])
        blank[..., 3] = 255
        self.tiles.append(blank)
        self.frames = [torch.from_numpy(f).to("cuda:0") for f in self.tiles]
        ex = [fe.akaze_keypoint_descriptor_extraction(np.roll(f, (19, 23), axis=(0, 1)).copy(), descriptor="kaze") for f in self.tiles[:2]]
        mldb = [fe.akaze_keypoint_descriptor_extraction_def(np.roll(f, (19, 23), axis=(0, 1)).copy(), None) for f in self.tiles[:2]]
        assert min(len(e.keypoints) for e in ex) >= 150 and np.asarray(ex[0].descriptors).shape[1] == 64
        rng = np.random.default_rng(11)
        n = max(DB_SIZES)
        self.db_kps = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
        self.db_kps["x"], self.db_kps["y"] = rng.uniform(0, T - 1, n).astype(np.float32), rng.uniform(0, T - 1, n).astype(np.float32)
        rows, _, _ = synth.make_l2_set(n, 1, dim=64, seed=0x4C32D000)
        self.db_f32 = rows
        self.db61 = synth.make_descriptor_db(n)                     # the byte-row DB of the ratio pipeline run beside the float one
        for i in range(2):
            self.db_f32[150 * i:150 * i + 150] = np.asarray(ex[i].descriptors, np.float32)[:150]
            self.db61[150 * i:150 * i + 150] = mldb[i].descriptors[:150]
            self.db_kps[150 * i:150 * i + 150] = np.asarray(ex[i].keypoints)[:150]
        self.db_xyz = np.stack([self.db_kps["x"] * 3.0, self.db_kps["y"] * 3.0, 40.0 * np.sin(self.db_kps["x"] / 17.0) + 1000.0], 1).astype(np.float64)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.torch.cuda.synchronize()
        return t

    def db_tensors(self, nd):
        xy = np.stack([self.db_kps["x"][:nd], self.db_kps["y"][:nd]], 1)
        return self.up(self.db_f32[:nd]), self.up(xy)

    def byte_tensors(self, nd):
        rows = np.zeros((nd, 64), np.uint8)
        rows[:, :61] = self.db61[:nd]
        return self.up(rows), self.up(np.stack([self.db_kps["x"][:nd], self.db_kps["y"][:nd]], 1))

    def pose(self, nd):
        return self.pl.PoseStage(self.db_xyz[:nd], KMAT, **POSE)


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    return Scene(gpu_pkg)


def serial(sc, f, nd, max_points=8192, pose=None, lens=None):
    """one frame through the public device calls on the null stream; the ratio rule on the host"""
    torch, pkg = sc.torch, sc.pkg
    L, check, ptr = pkg.lib(), pkg._lib.check, pkg._lib.ptr
    cap = max_points
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")     # noqa: E731
    kps, desc, keys = z((cap, 7), torch.float32), z((cap, 64), torch.float32), z((cap, 2), torch.int64)
    p1, p2, mask = z((cap, 2), torch.float32), z((cap, 2), torch.float32), z(cap, torch.uint8)
    img, obj = z((cap, 2), torch.float32), z((cap, 3), torch.float32)
    db, db_xy = sc.db_tensors(nd)
    tkps = z((nd, 7), torch.float32)
    tkps[:, 0:2] = db_xy
    torch.cuda.synchronize()
    frame = sc.frames[f]
    n = C.c_int(0)
    check(L.apds_dev_akaze_extract_float(frame.data_ptr(), T, T, 4, frame.stride(0), None, 0, 0, cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
    K = n.value
    out = dict(status=0, n_keypoints=K, n_matches=0, n_inliers=0, H=None)
    m = np.zeros(0, pkg._lib.DMATCH_DTYPE)
    if K:
        check(L.apds_dev_l2_topk(desc.data_ptr(), K, db.data_ptr(), nd, 64, 0, 2, keys.data_ptr(), None))
        check(L.apds_stream_synchronize(None))
        k = keys[:K].cpu().numpy().view(np.uint64)
        d = np.sqrt((k >> np.uint64(32)).astype(np.uint32).view(np.float32))                      # f32 sqrt, correctly rounded
        keep = np.flatnonzero((k[:, 0] != EMPTY) & (k[:, 1] != EMPTY) & (d[:, 0] < d[:, 1] * np.float32(FS)))
        m = np.zeros(len(keep), pkg._lib.DMATCH_DTYPE)
        m["query_idx"], m["train_idx"], m["distance"] = keep, (k[keep, 0] & np.uint64(0xFFFFFFFF)).astype(np.int32), d[keep, 0]
    M = out["n_matches"] = len(m)
    matches = sc.up(m.view(np.int32).reshape(-1, 4)) if M else z((1, 4), torch.int32)
    if lens is not None:
        Kl, dl = np.ascontiguousarray(lens[0], np.float64), np.ascontiguousarray(lens[1], np.float64)
    if M >= 4:
        check(L.apds_dev_points_from_matches(kps.data_ptr(), K, tkps.data_ptr(), nd, matches.data_ptr(), M, 0, p1.data_ptr(), p2.data_ptr(), None))
        if lens is not None:
            check(L.apds_dev_undistort_points(p1.data_ptr(), M, 8, ptr(Kl), ptr(dl), len(dl), lens[2], None))
        H = np.zeros(9, np.float64)
        rc = L.apds_dev_find_homography(p1.data_ptr(), p2.data_ptr(), M, 8, THR, ITERS, CONF, ptr(H), mask.data_ptr(), None)
        assert rc in (0, pkg._lib.ERR_EMPTY)
        check(L.apds_stream_synchronize(None))
        if rc == 0:
            out["H"], out["n_inliers"] = H.reshape(3, 3), int(np.count_nonzero(mask[:M].cpu().numpy()))
    if pose is not None:
        origin, Kc = np.ascontiguousarray(pose.origin), np.ascontiguousarray(pose.K)
        check(L.apds_dev_pnp_correspondences(kps.data_ptr(), K, pose.db_xyz_dev.data_ptr(), nd, ptr(origin), matches.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None))
        if lens is not None:
            check(L.apds_dev_undistort_points(img.data_ptr(), M, 8, ptr(Kl), ptr(dl), len(dl), lens[2], None))
        rv, tv, ni, found = np.zeros(3), np.zeros(3), C.c_int(0), C.c_int(0)
        rc = L.apds_dev_pnp_solver_ransac(obj.data_ptr(), img.data_ptr(), M, ptr(Kc), pose.iter_count, pose.reproj_thres, pose.confidence, pose.method, ptr(rv), ptr(tv),
                                          None, C.byref(ni), C.byref(found), None)
        check(L.apds_stream_synchronize(None))
        out["pose"] = sc.pl.pose_dict_of(rc, found.value, M, ni.value, rv, tv) if rc == 0 else sc.pl.pose_dict_of(rc, 0, M, 0, np.zeros(3), np.zeros(3))
    return out


def same(got, want, i):
    for k in ("status", "n_keypoints", "n_matches", "n_inliers"):
        assert got[k] == want[k], (i, k, got, want)
    assert (got["H"] is None) == (want["H"] is None), (i, got, want)
    if want["H"] is not None:
        assert np.array_equal(got["H"].view(np.uint64), want["H"].view(np.uint64)), (i, got["H"], want["H"])
    if "pose" in want:
        a, b = got["pose"], want["pose"]
        for k in ("status", "found", "n_correspondences", "n_inliers"):
            assert a[k] == b[k], (i, k, a, b)
        assert np.array_equal(a["rvec"].view(np.uint64), b["rvec"].view(np.uint64)) and np.array_equal(a["tvec"].view(np.uint64), b["tvec"].view(np.uint64)), (i, a, b)


def streamed(sc, nd, order, max_points=8192, pose=None, lens=None):
    """the float pipeline over the first nd rows: every frame of `order` submitted before the first poll"""
    db, db_xy = sc.db_tensors(nd)
    pipe = sc.pl.StreamedFramePipeline(db, db_xy, max_points=max_points, slots=max(6, len(order)), pose=pose, matcher="l2", lens=lens)
    try:
        pipe.prepare(sc.frames[0].shape, FS, THR, ITERS, CONF)
        for f in order:
            ptr, stride, on_dev = pipe.frame_args(sc.frames[f])
            sc.pkg._lib.check(sc.pkg.lib().apds_pipeline_submit(pipe._pipe, ptr, stride, on_dev, None))
        out = [pipe.poll() for _ in order]
        assert pipe.poll(wait=False) is None
        return out
    finally:
        pipe.close()


@pytest.mark.parametrize("nd", DB_SIZES)
def test_frames_and_poses_equal_the_serial_composition(scene, nd):
    pose = scene.pose(nd)
    want = {f: serial(scene, f, nd, pose=pose) for f in set(ORDER)}
    assert want[2]["n_keypoints"] == 0 and want[2]["n_matches"] == 0 and want[0]["n_keypoints"] >= 150
    if nd == 3000:
        assert want[0]["H"] is not None and want[1]["H"] is not None and want[0]["pose"]["status"] == 0
    got = streamed(scene, nd, ORDER, pose=pose)
    for i, (f, g) in enumerate(zip(ORDER, got)):
        same(g, want[f], i)
    assert got[2]["pose"]["status"] == scene.pkg._lib.ERR_ASSERT


@pytest.mark.parametrize("cap", [1, 128, 129])
def test_max_points_at_the_tile_borders(scene, cap):
    want = {f: serial(scene, f, 3000, max_points=cap) for f in (0, 1)}
    assert want[0]["n_keypoints"] == cap and want[1]["n_keypoints"] == cap
    got = streamed(scene, 3000, [0, 1, 0], max_points=cap)
    for i, (f, g) in enumerate(zip([0, 1, 0], got)):
        same(g, want[f], i)


def test_lens_reaches_both_stages(scene):
    lens = (KMAT, np.array(lr.SET_A), 5)
    pose = scene.pose(3000)
    want = [serial(scene, f, 3000, pose=pose, lens=lens) for f in (0, 1)]
    got = streamed(scene, 3000, [0, 1], pose=pose, lens=lens)
    for i in (0, 1):
        same(got[i], want[i], i)
    plain = streamed(scene, 3000, [0], pose=pose)[0]
    assert plain["n_matches"] == got[0]["n_matches"] and not np.array_equal(plain["H"], got[0]["H"])


def _create(sc, nd, float_rows):
    pkg, torch = sc.pkg, sc.torch
    L, check = pkg.lib(), pkg._lib.check
    db, db_xy = sc.db_tensors(nd) if float_rows else sc.byte_tensors(nd)
    kp = torch.zeros((nd, 7), dtype=torch.float32, device="cuda:0")
    kp[:, 0:2] = db_xy
    torch.cuda.synchronize()
    p = pkg._lib.PipelineParams(rows=T, cols=T, channels=4, max_points=8192, filter_strength=FS, homography_method=8)
    h = C.c_void_p()
    if float_rows:
        rc = L.apds_pipeline_create_float(C.byref(h), db.data_ptr(), nd, 0, kp.data_ptr(), nd, C.byref(p))
    else:
        rc = L.apds_pipeline_create(C.byref(h), db.data_ptr(), nd, 0, None, kp.data_ptr(), nd, C.byref(p))
    return rc, h, (db, kp)


def test_contract_errors(scene):
    pkg = scene.pkg
    L, check, BAD = pkg.lib(), pkg._lib.check, pkg._lib.ERR_BAD_ARG
    rc, h, keep = _create(scene, 129, True)
    check(rc)
    try:
        for other in (0, 1, -1, 3):
            assert L.apds_pipeline_set_matcher(h, other) == BAD
        assert L.apds_pipeline_set_matcher(h, 2) == 0                  # its own matcher, named: nothing changes
        r = pkg._lib.FrameResult()
        check(L.apds_pipeline_submit(h, scene.frames[0].data_ptr(), T * 4, 1, None))
        check(L.apds_pipeline_poll(h, C.byref(r), 1))
        assert r.status == 0 and r.n_keypoints >= 150 and r.n_matches > 4
        assert L.apds_pipeline_set_matcher(h, 2) == BAD                # after the first submit, as for every matcher
    finally:
        check(L.apds_pipeline_destroy(h))
    rc, h, keep = _create(scene, 129, False)                           # a byte-row pipeline never takes the float matcher
    check(rc)
    try:
        assert L.apds_pipeline_set_matcher(h, 2) == BAD
        assert L.apds_pipeline_set_matcher(h, 0) == 0
    finally:
        check(L.apds_pipeline_destroy(h))
    assert _create(scene, 1, True)[0] == pkg._lib.ERR_ASSERT           # fewer than two rows, as apds_pipeline_create
    db, db_xy = scene.db_tensors(129)
    with pytest.raises(ValueError):                                    # the fronts: "l2" goes with float32 rows, and only with them
        scene.pl.StreamedFramePipeline(scene.byte_tensors(129)[0], db_xy, matcher="l2")
    fp = scene.pl.FramePipeline(db, db_xy, max_points=8192)
    with pytest.raises(pkg.ApdsError):
        fp.step(scene.frames[0], FS, matcher="ratio")
    with pytest.raises(ValueError):                                    # no sharded float matcher: a group is refused, not dropped
        scene.pl.FramePipeline(db, db_xy, group=object(), max_points=8192)


def test_serial_front_gives_the_same_frames(scene):
    db, db_xy = scene.db_tensors(3000)
    fp = scene.pl.FramePipeline(db, db_xy, max_points=8192)
    got = streamed(scene, 3000, [0, 1])
    for f in (0, 1):
        s = fp.step(scene.frames[f], FS, THR, ITERS, CONF, matcher="l2")
        assert (s["n_keypoints"], s["n_matches"], s["n_inliers"]) == (got[f]["n_keypoints"], got[f]["n_matches"], got[f]["n_inliers"])
        assert s["H"] is not None and np.array_equal(s["H"], got[f]["H"])


def test_nothing_grows_over_fifty_frames(scene, capsys):
    """Two measures. The library's own account of its device workspaces (apds_workspace_info: bytes held by every thread's slabs and the
    slab cache, allocations made for them) must stand still EXACTLY over fifty frames: that is every allocation the float path makes per
    call (the stage threads' scratch, the screen's candidate buffers), and it does not depend on anything else in the process or on the
    device. The device's free memory, as the other pipelines' tests read it, catches what would bypass the workspaces; objects of earlier
    tests that are still waiting for the collector are released first, so that their device memory does not come back in between.
    (Measured on the MI355X: 0 bytes and 0 allocations in every one of 45 windows of ten frames, after twelve and after two warm-up frames.)"""
    torch, info = scene.torch, scene.pkg._lib.workspace_info
    db, db_xy = scene.db_tensors(3000)
    pipe = scene.pl.StreamedFramePipeline(db, db_xy, max_points=8192, matcher="l2", pose=scene.pose(3000))
    try:
        pipe.run(scene.frames[:2], 12)                   # every slot, every stage thread's workspace has been through a frame
        gc.collect()
        torch.cuda.synchronize()
        slabs0, free0 = info(), torch.cuda.mem_get_info()[0]
        a, _ = pipe.run(scene.frames[:2], 50)
        torch.cuda.synchronize()
        slabs1, free1 = info(), torch.cuda.mem_get_info()[0]
        with capsys.disabled():
            print(f"\n[float pipeline, 50 frames] workspace bytes {slabs0[0]} -> {slabs1[0]}, allocations {slabs0[1]} -> {slabs1[1]}, device free {free0} -> {free1}")
        assert slabs1 == slabs0 and slabs0[0] > 0
        assert abs(free1 - free0) < 4 << 20
        assert all(r["n_matches"] > 4 for r in a)
    finally:
        pipe.close()


def _ratio_run(sc):
    db, db_xy = sc.byte_tensors(3000)
    pipe = sc.pl.StreamedFramePipeline(db, db_xy, max_points=8192, matcher="ratio")
    try:
        got, _ = pipe.run(sc.frames, 6)
        return [[r["status"], r["n_keypoints"], r["n_matches"], r["n_inliers"], None if r["H"] is None else r["H"].tobytes()] for r in got]
    finally:
        pipe.close()


def test_float_pipeline_leaves_no_state_behind(scene):
    before = _ratio_run(scene)
    assert before[0][2] > 4
    streamed(scene, 3000, ORDER, pose=scene.pose(3000))
    assert _ratio_run(scene) == before
