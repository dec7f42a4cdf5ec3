"""GPU: the streamed pipeline with a lens (apds_pipeline_set_lens, csrc/pipeline.cpp; the stages in csrc/pipeline_stages.cpp).

The frame and DB shapes of tests/test_pipeline_pose_gpu.py (768 x 768 frames, a 60000-row DB holding every frame rolled by (19, 23)), pose
enabled, coefficient set A with a camera of f = 2000 (4.8 px of distortion at the frame's corners: enough to move every matched point,
little enough that the 3 px homography keeps its consensus).
 * for three frames the streamed result equals, bit for bit, the serial composition of the public device calls with
   apds_dev_undistort_points placed after apds_dev_points_from_matches (in front of the homography) and after
   apds_dev_pnp_correspondences (in front of the solve): keypoint and match counts, H, inlier count, pose - on a plain pipeline and on a
   table pipeline (per-frame views);
 * the lens does reach both stages (H and the pose differ from the pipeline without one) and touches nothing else (counts equal);
 * a pipeline with an all-zero lens equals one that never called set_lens, field for field;
 * apds_pipeline_set_lens after the first submit is APDS_ERR_BAD_ARG."""
import ctypes as C

import numpy as np
import pytest

import lens_reference as lr

pytestmark = pytest.mark.gpu

T, NDB, NFRAMES = 768, 60000, 3
FS, THR, ITERS, CONF = 0.3, 3.0, 2000, 0.995
KMAT = np.array([[2000.0, 0, 384], [0, 2000.0, 384], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)
LENS_ITERS = 5
DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


class Scene:
    """the frames, the DB as plain device arrays (rows, keypoints, world points) and the same rows as a keypoint table"""

    def __init__(self, pkg):
        import torch
        from importlib import import_module
        self.pkg, self.pl = pkg, import_module(pkg.__name__ + ".pipeline")
        fe, synth = pkg.feature_extraction, pkg.synth
        tiles = [synth.make_tile(T, T, frame_index=40 + i) for i in range(NFRAMES)]
        self.frames = [torch.from_numpy(f).to("cuda:0") for f in tiles]
        ex = [fe.akaze_keypoint_descriptor_extraction_def(np.roll(f, (19, 23), axis=(0, 1)).copy(), None) for f in tiles]
        n_real = sum(len(e.keypoints) for e in ex)
        rng = np.random.default_rng(6)
        filler = np.zeros(NDB - n_real, pkg._lib.KEYPOINT_DTYPE)
        filler["x"], filler["y"] = rng.uniform(0, T - 1, len(filler)).astype(np.float32), rng.uniform(0, T - 1, len(filler)).astype(np.float32)
        filler["response"] = rng.uniform(0, 1e-4, len(filler)).astype(np.float32)
        fill_desc = synth.make_descriptor_db(len(filler))
        self.table = t = pkg.feature_database.KeypointTable(NDB)
        for i, e in enumerate(ex):
            t.create_keypoints(e, 1 + i, 0, 0, 0, (T, T))
        t.create_keypoints(_Ex(filler, fill_desc), 9, 0, 0, 0, (T, T))
        et = pkg.feature_database.ElevationTable()
        et.create_geotransform("dataset", DGT)
        assert t.world_coordinates(et) == 0
        # the plain DB: the table's own columns (rows in insertion order)
        rows64, kps, xyz, n = t.device_table()
        assert n == NDB and xyz
        self.db = self.pl._table_tensor(rows64, n * 64, "cuda:0", torch.uint8, (n, 64))
        self.db_kp = self.pl._table_tensor(kps, n * 28, "cuda:0", torch.float32, (n, 7))
        self.pose = self.pl.PoseStage.from_table(t, KMAT, **POSE)
        self.sel = self.pl.StreamedFramePipeline.selection(1, 0)          # the whole level of detail 0, by response

    def close(self):
        self.table.close()


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    sc = Scene(gpu_pkg)
    yield sc
    sc.close()


def serial(sc, frame, lens, table):
    """one frame through the public device calls; lens = (K, dist, iters) or None; table: the train set is apds_db_select's view"""
    import torch
    pkg, pose = sc.pkg, sc.pose
    L, check, ptr = pkg.lib(), pkg._lib.check, pkg._lib.ptr
    cap = pkg.feature_extraction.MAX_POINTS
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")     # noqa: E731
    kps, desc, keys, matches = z((cap, 7), torch.float32), z((cap, 64), torch.uint8), z((cap, 2), torch.int64), z((cap, 4), torch.int32)
    p1, p2, mask = z((cap, 2), torch.float32), z((cap, 2), torch.float32), z(cap, torch.uint8)
    img, obj = z((cap, 2), torch.float32), z((cap, 3), torch.float32)
    torch.cuda.synchronize()
    if lens is not None:
        Kl, dl = np.ascontiguousarray(lens[0], np.float64), np.ascontiguousarray(lens[1], np.float64)
    n = C.c_int(0)
    check(L.apds_dev_akaze_extract(frame.data_ptr(), T, T, 4, frame.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
    K = n.value
    if table:
        nv = C.c_int(0)
        check(L.apds_db_select(sc.table._h, sc.sel.mode, sc.sel.value, 0, 0, 0, 0, C.byref(nv)))
        rows64, tkps, vrows, _, nt = sc.table.view_device_pointers()
        row_ids = np.zeros(nt, np.int32)
        check(L.apds_dev_download(ptr(row_ids), vrows, row_ids.nbytes, None))
        xyz = torch.from_numpy(np.ascontiguousarray(pose.db_xyz[row_ids])).to("cuda:0")
        torch.cuda.synchronize()
        xyz_ptr = xyz.data_ptr()
    else:
        rows64, tkps, nt, xyz_ptr = sc.db.data_ptr(), sc.db_kp.data_ptr(), NDB, pose.db_xyz_dev.data_ptr()
    out = dict(n_keypoints=K, n_matches=0, n_inliers=0, status=0, H=None)
    check(L.apds_dev_hamming_topk(desc.data_ptr(), K, rows64, nt, 0, 2, keys.data_ptr(), None))
    M = C.c_int(0)
    check(L.apds_dev_ratio_filter(keys.data_ptr(), K, 2, FS, matches.data_ptr(), C.byref(M), None))
    M = out["n_matches"] = M.value
    assert M >= 4
    check(L.apds_dev_points_from_matches(kps.data_ptr(), K, tkps, nt, matches.data_ptr(), M, 0, p1.data_ptr(), p2.data_ptr(), None))
    if lens is not None:
        check(L.apds_dev_undistort_points(p1.data_ptr(), M, 8, ptr(Kl), ptr(dl), len(dl), lens[2], None))
    H = np.zeros(9, np.float64)
    rc = L.apds_dev_find_homography(p1.data_ptr(), p2.data_ptr(), M, 8, THR, ITERS, CONF, ptr(H), mask.data_ptr(), None)
    assert rc in (0, pkg._lib.ERR_EMPTY)
    check(L.apds_stream_synchronize(None))
    out["p1"] = p1[:M].cpu().numpy()
    if rc == 0:
        out["H"], out["n_inliers"] = H.reshape(3, 3), int(np.count_nonzero(mask[:M].cpu().numpy()))
    origin = np.ascontiguousarray(pose.origin)
    check(L.apds_dev_pnp_correspondences(kps.data_ptr(), K, xyz_ptr, nt, ptr(origin), matches.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None))
    if lens is not None:
        check(L.apds_dev_undistort_points(img.data_ptr(), M, 8, ptr(Kl), ptr(dl), len(dl), lens[2], None))
    rv, tv, ni, found = np.zeros(3), np.zeros(3), C.c_int(0), C.c_int(0)
    Kc = np.ascontiguousarray(pose.K)
    rc = L.apds_dev_pnp_solver_ransac(obj.data_ptr(), img.data_ptr(), M, ptr(Kc), pose.iter_count, pose.reproj_thres, pose.confidence, pose.method, ptr(rv), ptr(tv),
                                      None, C.byref(ni), C.byref(found), None)
    check(L.apds_stream_synchronize(None))
    out["pose"] = sc.pl.pose_dict_of(rc, found.value, M, ni.value, rv, tv) if rc == 0 else sc.pl.pose_dict_of(rc, 0, M, 0, np.zeros(3), np.zeros(3))
    # the matched image points the two stages saw are the reference's undistortion of the frame's keypoints, rounded once
    m = matches[:M].cpu().numpy()
    src = kps[:K].cpu().numpy()[m[:, 0], 0:2]
    want = src if lens is None else lr.undistort_points_f32_ref(src, lens[0], lens[1], lens[2])
    assert np.array_equal(out.pop("p1").view(np.uint32), want.view(np.uint32))
    assert np.array_equal(img[:M].cpu().numpy().view(np.uint32), want.view(np.uint32))
    return out


def streamed(sc, lens, table, count=NFRAMES):
    SP = sc.pl.StreamedFramePipeline
    if table:
        pipe = SP.from_table(sc.table, per_frame_view=True, view_capacity=NDB, pose=sc.pose, lens=lens)
    else:
        pipe = SP(sc.db, None, db_kp=sc.db_kp, pose=sc.pose, lens=lens)
    try:
        got, _ = pipe.run(sc.frames, count, filter_strength=FS, reproj_thr=THR, max_iters=ITERS, confidence=CONF, selections=[sc.sel] if table else None)
        return got
    finally:
        pipe.close()


def same(got, want, i):
    for k in ("status", "n_keypoints", "n_matches", "n_inliers"):
        assert got[k] == want[k], (i, k, got, want)
    assert (got["H"] is None) == (want["H"] is None), (i, got, want)
    if want["H"] is not None:
        assert np.array_equal(got["H"].view(np.uint64), want["H"].view(np.uint64)), (i, got["H"], want["H"])
    a, b = got["pose"], want["pose"]
    for k in ("status", "found", "n_correspondences", "n_inliers"):
        assert a[k] == b[k], (i, k, a, b)
    assert np.array_equal(a["rvec"].view(np.uint64), b["rvec"].view(np.uint64)) and np.array_equal(a["tvec"].view(np.uint64), b["tvec"].view(np.uint64)), (i, a, b)


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_streamed_frames_equal_the_serial_composition_with_the_lens(scene, table):
    lens = (KMAT, np.array(lr.SET_A), LENS_ITERS)
    want = [serial(scene, f, lens, table) for f in scene.frames]
    assert all(w["n_matches"] > 100 and w["pose"]["status"] == 0 for w in want) and any(w["H"] is not None for w in want)
    got = streamed(scene, lens, table)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)
    # the lens reaches both stages and nothing else
    off = streamed(scene, None, table)
    for g, o in zip(got, off):
        assert (g["n_keypoints"], g["n_matches"], g["status"], g["pose"]["n_correspondences"]) == (o["n_keypoints"], o["n_matches"], o["status"], o["pose"]["n_correspondences"])
    assert any(g["H"] is not None and o["H"] is not None and not np.array_equal(g["H"], o["H"]) for g, o in zip(got, off))
    assert any(g["pose"]["found"] and o["pose"]["found"] and not np.array_equal(g["pose"]["rvec"], o["pose"]["rvec"]) for g, o in zip(got, off))


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_an_all_zero_lens_equals_no_lens(scene, table):
    off = streamed(scene, None, table)
    zero = streamed(scene, (KMAT, np.zeros(5), LENS_ITERS), table)
    for i, (g, o) in enumerate(zip(zero, off)):
        same(g, o, i)
    want = [serial(scene, f, None, table) for f in scene.frames]
    for i, (g, w) in enumerate(zip(off, want)):
        same(g, w, i)


def test_set_lens_after_the_first_submit_is_refused(scene):
    pkg = scene.pkg
    L, ptr = pkg.lib(), pkg._lib.ptr
    pipe = scene.pl.StreamedFramePipeline(scene.db, None, db_kp=scene.db_kp)
    Kc, d = np.ascontiguousarray(KMAT), np.array(lr.SET_A)
    try:
        h = pipe.prepare(scene.frames[0].shape, FS, THR, ITERS, CONF)
        assert L.apds_pipeline_set_lens(h, ptr(Kc), ptr(d), 3, 5) == pkg._lib.ERR_BAD_ARG          # argument errors first
        assert L.apds_pipeline_set_lens(h, ptr(Kc), ptr(d), 4, 5) == 0                             # before the first submit: accepted (and again)
        assert L.apds_pipeline_set_lens(h, ptr(Kc), ptr(d), 4, 0) == 0
        p, stride, on_dev = pipe.frame_args(scene.frames[0])
        pkg._lib.check(L.apds_pipeline_submit(h, p, stride, on_dev, None))
        assert L.apds_pipeline_set_lens(h, ptr(Kc), ptr(d), 4, 5) == pkg._lib.ERR_BAD_ARG
        assert pipe.poll()["status"] == 0
        assert L.apds_pipeline_set_lens(h, ptr(Kc), ptr(d), 4, 5) == pkg._lib.ERR_BAD_ARG
    finally:
        pipe.close()
