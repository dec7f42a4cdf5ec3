"""GPU: apds_pipeline_create_table on a FLOAT keypoint table (csrc/pipeline.cpp, csrc/pipeline_match.cpp): workers extract M-SURF rows, the matcher is the L2 ratio
matcher for life, and each frame's train set is its slot's view of the table, the screen's train side written by the select's gather
(apds_db_view_l2_train).

The table holds about 3000 rows over two levels of detail: the M-SURF rows of two frames rolled by (19, 23) first, random unit rows behind
them. Frames are 256 x 256. Selections that return 0 rows, 1 row, 2 rows, a region, a whole level of detail and more rows than the view
holds. Every streamed frame equals the serial composition of public calls: apds_db_view_select -> apds_dev_akaze_extract_float ->
apds_dev_l2_topk (the exact kernel) over the view's rows -> the ratio rule of get_knn_matches_l2 on the host -> apds_dev_points_from_matches
-> apds_dev_find_homography and, with pose, apds_dev_pnp_correspondences -> apds_dev_pnp_solver_ransac: counts equal, H / rvec / tvec bit for
bit. A view of fewer than two rows gives the frame the status it gives on a byte table (APDS_ERR_ASSERT, no matches)."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

from db_float_cases import Ex

pytestmark = pytest.mark.gpu

T = 256
FS, THR, ITERS, CONF = 0.8, 3.0, 2000, 0.995
KMAT = np.array([[900.0, 0, 128], [0, 900.0, 128], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)
DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
VIEW_CAP = 1200
# name -> (mode, value, box): images 1, 2 = the two rolled frames (level 0), 3 = one row (level 2), 4 = two rows (level 3), 5, 6 = filler
SELECTIONS = {"none": (0, 99, None), "one": (0, 3, None), "two": (0, 4, None), "region": (2, 0, (0.0, 0.0, 140.0, 255.0)), "level0": (1, 0, None),
              "over": (1, 1, None), "frame0": (0, 1, None), "frame1": (0, 2, None)}
PLAN = [(0, "frame0"), (1, "none"), (0, "one"), (1, "two"), (0, "region"), (1, "level0"), (0, "over"), (1, "frame1"), (0, "level0")]


class Scene:
    def __init__(self, pkg):
        import torch
        self.torch, self.pkg, self.pl = torch, pkg, import_module(pkg.__name__ + ".pipeline")
        fe, synth, fd = pkg.feature_extraction, pkg.synth, pkg.feature_database
        self.tiles = [synth.make_tile(T, T, frame_index=70 + i, blobs_per_mpx=20000) for i in range(2)]
        self.frames = [torch.from_numpy(f).to("cuda:0") for f in self.tiles]
        ex = [fe.akaze_keypoint_descriptor_extraction(np.roll(f, (19, 23), axis=(0, 1)).copy(), descriptor="kaze") for f in self.tiles]
        assert min(len(e.keypoints) for e in ex) >= 150
        rng = np.random.default_rng(12)

        def filler(n, seed):
            kp = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
            kp["x"], kp["y"] = rng.uniform(0, T - 1, n).astype(np.float32), rng.uniform(0, T - 1, n).astype(np.float32)
            kp["response"] = rng.uniform(1e-4, 1e-2, n).astype(np.float32)
            rows, _, _ = synth.make_l2_set(n, 1, dim=64, seed=seed)
            return Ex(kp, rows)

        self.table = fd.KeypointTable(4096, descriptor="kaze")
        for image_id, lod, e in ((1, 0, ex[0]), (2, 0, ex[1]), (3, 2, filler(1, 1)), (4, 3, filler(2, 2)), (5, 0, filler(900, 3)), (6, 1, filler(1700, 4))):
            self.table.create_keypoints(Ex(np.asarray(e.keypoints), np.asarray(e.descriptors, np.float32)), image_id, lod)
        assert 2900 <= len(self.table) <= 4096
        et = fd.ElevationTable()
        et.create_geotransform("dataset", DGT)
        assert self.table.world_coordinates(et) == 0
        self.sel = {k: self.pl.StreamedFramePipeline.selection(m, v, b or (0, 0, 0, 0)) for k, (m, v, b) in SELECTIONS.items()}
        self.view = self.table.view(VIEW_CAP)


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    sc = Scene(gpu_pkg)
    yield sc
    sc.view.close()
    sc.table.close()


def serial(sc, f, name, pose=None):
    torch, pkg = sc.torch, sc.pkg
    L, check, ptr = pkg.lib(), pkg._lib.check, pkg._lib.ptr
    cap = 8192
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")     # noqa: E731
    kps, desc, keys = z((cap, 7), torch.float32), z((cap, 64), torch.float32), z((cap, 2), torch.int64)
    p1, p2, mask = z((cap, 2), torch.float32), z((cap, 2), torch.float32), z(cap, torch.uint8)
    img, obj = z((cap, 2), torch.float32), z((cap, 3), torch.float32)
    torch.cuda.synchronize()
    mode, value, box = SELECTIONS[name]
    box = box or (0, 0, 0, 0)
    nv = sc.view._select(mode, value, box, pose is not None, None)
    rows, vkps, _, _, xyz, n2 = sc.view.device_pointers()
    assert n2 == nv
    frame = sc.frames[f]
    n = C.c_int(0)
    check(L.apds_dev_akaze_extract_float(frame.data_ptr(), T, T, 4, frame.stride(0), None, 0, 0, cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
    K = n.value
    out = dict(status=0, n_keypoints=K, n_matches=0, n_inliers=0, H=None)
    if nv < 2:
        out["status"] = pkg._lib.ERR_ASSERT
        if pose is not None:
            out["pose"] = sc.pl.pose_dict_of(pkg._lib.ERR_ASSERT, 0, 0, 0, np.zeros(3), np.zeros(3))
        return out
    check(L.apds_dev_l2_topk(desc.data_ptr(), K, rows, nv, 64, 0, 2, keys.data_ptr(), None))
    check(L.apds_stream_synchronize(None))
    k = keys[:K].cpu().numpy().view(np.uint64)
    d = np.sqrt((k >> np.uint64(32)).astype(np.uint32).view(np.float32))
    keep = np.flatnonzero((k[:, 0] != EMPTY) & (k[:, 1] != EMPTY) & (d[:, 0] < d[:, 1] * np.float32(FS)))
    m = np.zeros(len(keep), pkg._lib.DMATCH_DTYPE)
    m["query_idx"], m["train_idx"], m["distance"] = keep, (k[keep, 0] & np.uint64(0xFFFFFFFF)).astype(np.int32), d[keep, 0]
    M = out["n_matches"] = len(m)
    matches = z((max(M, 1), 4), torch.int32)
    if M:
        matches.copy_(torch.from_numpy(m.view(np.int32).reshape(-1, 4)))
    torch.cuda.synchronize()
    if M >= 4:
        check(L.apds_dev_points_from_matches(kps.data_ptr(), K, vkps, nv, matches.data_ptr(), M, 0, p1.data_ptr(), p2.data_ptr(), None))
        H = np.zeros(9, np.float64)
        rc = L.apds_dev_find_homography(p1.data_ptr(), p2.data_ptr(), M, 8, THR, ITERS, CONF, ptr(H), mask.data_ptr(), None)
        assert rc in (0, pkg._lib.ERR_EMPTY)
        check(L.apds_stream_synchronize(None))
        if rc == 0:
            out["H"], out["n_inliers"] = H.reshape(3, 3), int(np.count_nonzero(mask[:M].cpu().numpy()))
    if pose is not None:
        origin, Kc = np.ascontiguousarray(pose.origin), np.ascontiguousarray(pose.K)
        check(L.apds_dev_pnp_correspondences(kps.data_ptr(), K, xyz, nv, ptr(origin), matches.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None))
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


def streamed(sc, plan, pose=None):
    pipe = sc.pl.StreamedFramePipeline.from_table(sc.table, per_frame_view=True, view_capacity=VIEW_CAP, max_points=8192, slots=max(6, len(plan)), pose=pose)
    try:
        assert pipe.float_rows
        pipe.prepare(sc.frames[0].shape, FS, THR, ITERS, CONF)
        for f, s in plan:
            pipe.submit_select(sc.frames[f], sc.sel[s])
        out = [pipe.poll() for _ in plan]
        assert pipe.poll(wait=False) is None
        return out
    finally:
        pipe.close()


@pytest.mark.parametrize("with_pose", [False, True])
def test_frames_equal_the_serial_composition(scene, with_pose):
    pose = scene.pl.PoseStage.from_table(scene.table, KMAT, **POSE) if with_pose else None
    want = [serial(scene, f, s, pose) for f, s in PLAN]
    assert want[0]["H"] is not None and want[7]["H"] is not None and want[5]["n_matches"] >= 4
    assert [w["status"] for w in want[1:3]] == [scene.pkg._lib.ERR_ASSERT] * 2 and want[3]["status"] == 0
    got = streamed(scene, PLAN, pose)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)
    if with_pose:
        assert sum(w["pose"]["status"] == 0 and w["pose"]["found"] for w in want) >= 2


def test_matcher_is_l2_for_life_and_byte_pipelines_are_untouched(scene):
    pkg, pl = scene.pkg, scene.pl
    L, BAD = pkg.lib(), pkg._lib.ERR_BAD_ARG
    fd = pkg.feature_database

    def byte_run():
        bt = fd.KeypointTable(512)
        try:
            e = pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(np.roll(scene.tiles[0], (19, 23), axis=(0, 1)).copy(), None)
            bt.create_keypoints(e, 1, 0)
            p = pl.StreamedFramePipeline.from_table(bt, per_frame_view=True, max_points=8192)
            try:
                p.prepare(scene.frames[0].shape, FS, THR, ITERS, CONF)
                p.submit_select(scene.frames[0], pl.StreamedFramePipeline.selection(0, 1))
                r = p.poll()
                return r["status"], r["n_keypoints"], r["n_matches"], r["n_inliers"], None if r["H"] is None else r["H"].tobytes()
            finally:
                p.close()
        finally:
            bt.close()

    before = byte_run()
    assert before[0] == 0 and before[2] >= 4
    pipe = pl.StreamedFramePipeline.from_table(scene.table, per_frame_view=True, view_capacity=VIEW_CAP, max_points=8192)
    try:
        h = pipe.prepare(scene.frames[0].shape, FS, THR, ITERS, CONF)
        for matcher in (pkg._lib.PIPELINE_MATCH_CROSSCHECK, pkg._lib.PIPELINE_MATCH_RATIO, 7):
            assert L.apds_pipeline_set_matcher(h, matcher) == BAD
        assert L.apds_pipeline_set_matcher(h, pkg._lib.PIPELINE_MATCH_L2_RATIO) == 0
        pipe.submit_select(scene.frames[0], scene.sel["frame0"])
        assert pipe.poll()["status"] == 0
    finally:
        pipe.close()
    with pytest.raises(ValueError):
        pl.StreamedFramePipeline.from_table(scene.table, per_frame_view=True, matcher="crosscheck")
    with pytest.raises(ValueError):
        pl.StreamedFramePipeline.from_table(scene.table)                 # a float table has no whole-table pipeline
    assert byte_run() == before
