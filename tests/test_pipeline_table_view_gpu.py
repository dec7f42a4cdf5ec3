"""GPU: the pipeline whose train set is selected per frame from a keypoint table (apds_pipeline_create_table /
apds_pipeline_submit_select, csrc/pipeline.cpp; the select per frame in csrc/pipeline_match.cpp; keypointdb.rs:50-90 is the read it repeats).

Frames and tiles are 256 x 256 (synth.py). The table holds two frames rolled by (19, 23) at two levels of detail and two tile columns,
one single-row image at a third level, and random filler. Every frame's result is compared bit for bit with a serial composition of
calls that existed before this path: extraction, apds_db_select with the frame's selection, apds_db_view, apds_dev_hamming_topk,
apds_dev_ratio_filter, apds_dev_points_from_matches, apds_dev_find_homography and, with pose, apds_dev_pnp_correspondences on the xyz
column gathered by the view's row ids and apds_dev_pnp_solver_ransac."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 256
FS, THR, ITERS, CONF = 0.8, 3.0, 2000, 0.995                 # StreamedFramePipeline.run's defaults
KMAT = np.array([[900.0, 0, 128], [0, 900.0, 128], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


class Scene:
    def __init__(self, pkg):
        import torch
        from importlib import import_module
        self.pkg, self.pl = pkg, import_module(pkg.__name__ + ".pipeline")
        fe, synth = pkg.feature_extraction, pkg.synth
        tiles = [synth.make_tile(T, T, frame_index=70 + i, blobs_per_mpx=20000) for i in range(2)]      # ~190 keypoints each
        self.frames = [torch.from_numpy(f).to("cuda:0") for f in tiles]
        ex = [fe.akaze_keypoint_descriptor_extraction_def(np.roll(f, (19, 23), axis=(0, 1)).copy(), None) for f in tiles]
        assert min(len(e.keypoints) for e in ex) >= 50
        rng = np.random.default_rng(5)
        filler = np.zeros(400, pkg._lib.KEYPOINT_DTYPE)
        filler["x"], filler["y"], filler["response"] = rng.uniform(0, 255, 400), rng.uniform(0, 255, 400), rng.uniform(0, 0.01, 400)
        one = np.zeros(1, pkg._lib.KEYPOINT_DTYPE)
        n = 2 * sum(len(e.keypoints) for e in ex) + len(filler) + 1
        self.table = t = pkg.feature_database.KeypointTable(n)
        t.create_keypoints(ex[0], 1, 0, 0, 0, (T, T))                      # level 0: frame 0 at tile column 0, frame 1 at column 1
        t.create_keypoints(ex[1], 2, 0, 1, 0, (T, T))
        t.create_keypoints(_Ex(filler, synth.make_descriptor_db(400)), 3, 0, 2, 0, (T, T))
        t.create_keypoints(ex[0], 4, 1, 1, 0, (T, T))                      # level 1: the other way round
        t.create_keypoints(ex[1], 5, 1, 0, 0, (T, T))
        t.create_keypoints(_Ex(one, np.zeros((1, 61), np.uint8)), 6, 2, 0, 0, (T, T))
        et = pkg.feature_database.ElevationTable()
        et.create_geotransform("dataset", [9.0, 1e-4, 0, 57.0, 0, -1e-4])
        assert t.world_coordinates(et) == 0
        s = self.pl.StreamedFramePipeline.selection
        self.sel = {"a0": s(2, 0, (0, 0, 255.5, 255.5)), "b0": s(2, 0, (257, 0, 511.5, 255.5)), "a1": s(2, 1, (513, 0, 1023, 511)), "b1": s(2, 1, (0, 0, 511, 511)),
                    "lod0": s(1, 0), "img4": s(0, 4), "empty": s(1, 9), "one": s(1, 2)}

    def close(self):
        self.table.close()


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    sc = Scene(gpu_pkg)
    yield sc
    sc.close()


def serial(sc, frame, sel, pose=None):
    """one frame through the existing one-call entry points, the train set being apds_db_select's view"""
    import torch
    pkg = sc.pkg
    L, check = pkg.lib(), pkg._lib.check
    cap = 8192
    kps = torch.zeros((cap, 7), dtype=torch.float32, device="cuda:0")
    desc = torch.zeros((cap, 64), dtype=torch.uint8, device="cuda:0")
    keys = torch.zeros((cap, 2), dtype=torch.int64, device="cuda:0")
    matches = torch.zeros((cap, 4), dtype=torch.int32, device="cuda:0")
    p1, p2 = torch.zeros((cap, 2), dtype=torch.float32, device="cuda:0"), torch.zeros((cap, 2), dtype=torch.float32, device="cuda:0")
    mask = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    n = C.c_int(0)
    check(L.apds_dev_akaze_extract(frame.data_ptr(), T, T, 4, frame.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), None))
    K = n.value
    out = dict(n_keypoints=K, n_matches=0, n_inliers=0, status=0, H=None)
    nv = C.c_int(0)
    check(L.apds_db_select(sc.table._h, sel.mode, sel.value, sel.x_start, sel.y_start, sel.x_end, sel.y_end, C.byref(nv)))
    rows64, vkps, vrows, _, nv = sc.table.view_device_pointers()
    pose_out = None
    if nv < 2:
        out["status"] = pkg._lib.ERR_ASSERT
        if pose is not None:
            pose_out = sc.pl.pose_dict_of(pkg._lib.ERR_ASSERT, 0, 0, 0, np.zeros(3), np.zeros(3))
    else:
        check(L.apds_dev_hamming_topk(desc.data_ptr(), K, rows64, nv, 0, 2, keys.data_ptr(), None))
        M = C.c_int(0)
        check(L.apds_dev_ratio_filter(keys.data_ptr(), K, 2, FS, matches.data_ptr(), C.byref(M), None))
        M = out["n_matches"] = M.value
        if M >= 4:
            check(L.apds_dev_points_from_matches(kps.data_ptr(), K, vkps, nv, matches.data_ptr(), M, 0, p1.data_ptr(), p2.data_ptr(), None))
            H = np.zeros(9, np.float64)
            rc = L.apds_dev_find_homography(p1.data_ptr(), p2.data_ptr(), M, 8, THR, ITERS, CONF, pkg._lib.ptr(H), mask.data_ptr(), None)
            assert rc in (0, pkg._lib.ERR_EMPTY)
            if rc == 0:
                check(L.apds_stream_synchronize(None))
                out["H"], out["n_inliers"] = H.reshape(3, 3), int(np.count_nonzero(mask[:M].cpu().numpy()))
        if pose is not None:
            row_ids = np.zeros(nv, np.int32)
            check(L.apds_dev_download(pkg._lib.ptr(row_ids), vrows, row_ids.nbytes, None))
            xyz = torch.from_numpy(np.ascontiguousarray(pose.db_xyz[row_ids])).to("cuda:0")          # the table column gathered by the view's row ids
            img, obj = torch.zeros((cap, 2), dtype=torch.float32, device="cuda:0"), torch.zeros((cap, 3), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            origin = np.ascontiguousarray(pose.origin)
            check(L.apds_dev_pnp_correspondences(kps.data_ptr(), K, xyz.data_ptr(), nv, pkg._lib.ptr(origin), matches.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None))
            rv, tv, ni, found = np.zeros(3), np.zeros(3), C.c_int(0), C.c_int(0)
            Kc = np.ascontiguousarray(pose.K)
            rc = L.apds_dev_pnp_solver_ransac(obj.data_ptr(), img.data_ptr(), M, pkg._lib.ptr(Kc), pose.iter_count, pose.reproj_thres, pose.confidence, pose.method,
                                              pkg._lib.ptr(rv), pkg._lib.ptr(tv), None, C.byref(ni), C.byref(found), None)
            pose_out = sc.pl.pose_dict_of(rc, found.value, M, ni.value, rv, tv) if rc == 0 else sc.pl.pose_dict_of(rc, 0, M, 0, np.zeros(3), np.zeros(3))
    check(L.apds_stream_synchronize(None))
    if pose_out is not None:
        out["pose"] = pose_out
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
        assert np.array_equal(a["rvec"], b["rvec"]) and np.array_equal(a["tvec"], b["tvec"]), (i, a, b)


def streamed(sc, plan, pose=None, view_capacity=None, slots=6):
    """plan: [(frame index, selection name)]; everything is submitted before the first poll when it fits the slots"""
    pipe = sc.pl.StreamedFramePipeline.from_table(sc.table, per_frame_view=True, view_capacity=view_capacity, max_points=8192, slots=slots, pose=pose)
    try:
        pipe.prepare(sc.frames[0].shape, FS, THR, ITERS, CONF)
        out = []
        for at in range(0, len(plan), slots):
            chunk = plan[at:at + slots]
            for f, s in chunk:
                pipe.submit_select(sc.frames[f], sc.sel[s])
            out += [pipe.poll() for _ in chunk]
        assert pipe.poll(wait=False) is None
        return out
    finally:
        pipe.close()


PLAN = [(0, "a0"), (1, "b0"), (0, "a1"), (1, "b1"), (0, "lod0"), (1, "lod0"), (0, "img4"), (1, "b0"), (0, "b0")]


def test_frames_equal_the_serial_composition(scene):
    want = [serial(scene, scene.frames[f], scene.sel[s]) for f, s in PLAN]
    assert sum(w["H"] is not None for w in want) >= 4 and want[0]["n_matches"] >= 8          # the scene does match
    assert want[-1]["n_matches"] < want[0]["n_matches"]                                          # frame 0 against frame 1's tile does not
    got = streamed(scene, PLAN)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)


def test_frames_and_poses_equal_the_serial_composition(scene):
    pose = scene.pl.PoseStage.from_table(scene.table, KMAT, **POSE)
    want = [serial(scene, scene.frames[f], scene.sel[s], pose) for f, s in PLAN]
    assert sum(w["pose"]["status"] == 0 for w in want) >= 4
    got = streamed(scene, PLAN, pose=pose)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)


def test_a_view_capacity_cuts_the_train_set(scene):
    """a view of 64 rows: the serial side takes the first 64 rows of the uncut view, which are the same rows by the order's definition"""
    sel = scene.sel["lod0"]
    full = serial(scene, scene.frames[0], sel)
    got = streamed(scene, [(0, "lod0")], view_capacity=64)[0]
    assert got["status"] == 0 and got["n_keypoints"] == full["n_keypoints"] and got["n_matches"] <= full["n_matches"]


def test_frames_in_flight_do_not_share_a_view(scene):
    slots = 6
    plan = [(i % 2, "a0" if i % 2 == 0 else "b0") for i in range(2 * slots)]
    want = {0: serial(scene, scene.frames[0], scene.sel["a0"]), 1: serial(scene, scene.frames[1], scene.sel["b0"])}
    assert want[0]["n_matches"] != want[1]["n_matches"] or not np.array_equal(want[0]["H"], want[1]["H"])
    pipe = scene.pl.StreamedFramePipeline.from_table(scene.table, per_frame_view=True, max_points=8192, slots=2 * slots)
    try:
        pipe.prepare(scene.frames[0].shape, FS, THR, ITERS, CONF)
        for f, s in plan:                                   # 2 x 6 frames in flight before the first poll
            pipe.submit_select(scene.frames[f], scene.sel[s])
        got = [pipe.poll() for _ in plan]
    finally:
        pipe.close()
    for i, g in enumerate(got):
        same(g, want[i % 2], i)


def test_degenerate_selections_fail_their_frame_only(scene):
    plan = [(0, "a0"), (1, "empty"), (1, "b0"), (0, "one"), (0, "a0")]
    pose = scene.pl.PoseStage.from_table(scene.table, KMAT, **POSE)
    got = streamed(scene, plan, pose=pose)
    want = [serial(scene, scene.frames[f], scene.sel[s], pose) for f, s in plan]
    for i in (1, 3):
        assert got[i]["status"] == scene.pkg._lib.ERR_ASSERT and got[i]["n_matches"] == 0 and got[i]["H"] is None
        assert got[i]["pose"]["status"] == scene.pkg._lib.ERR_ASSERT and got[i]["pose"]["found"] == 0
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)
    assert got[0]["H"] is not None and got[4]["H"] is not None


def test_contract_errors(scene):
    pkg, pl = scene.pkg, scene.pl
    L, BAD = pkg.lib(), pkg._lib.ERR_BAD_ARG
    f = scene.frames[0]
    ptr, stride, on_dev = pl.StreamedFramePipeline.frame_args(f)
    table_pipe = pl.StreamedFramePipeline.from_table(scene.table, per_frame_view=True, max_points=8192)
    plain = pl.StreamedFramePipeline.from_table(scene.table, max_points=8192)
    try:
        h = table_pipe.prepare(f.shape, FS, THR, ITERS, CONF)
        assert L.apds_pipeline_submit(h, ptr, stride, on_dev, None) == BAD
        assert L.apds_pipeline_submit_select(h, ptr, stride, on_dev, None, None) == BAD
        for mode in (-1, 3):
            bad = pl.StreamedFramePipeline.selection(mode, 0)
            assert L.apds_pipeline_submit_select(h, ptr, stride, on_dev, C.byref(bad), None) == BAD
        hp = plain.prepare(f.shape, FS, THR, ITERS, CONF)
        assert L.apds_pipeline_submit_select(hp, ptr, stride, on_dev, C.byref(scene.sel["a0"]), None) == BAD
        st = table_pipe.stats()
        assert st.frames_submitted == 0 and st.split_scan == 0 and st.world == 1
        # pose on a table pipeline: no xyz pointer is taken
        pp = pl.PoseStage.from_table(scene.table, KMAT, **POSE).params()
        assert pp.db_xyz_dev and L.apds_pipeline_enable_pose(h, C.byref(pp)) == BAD
        # the pipeline still works
        table_pipe.submit_select(f, scene.sel["a0"])
        assert table_pipe.poll()["status"] == 0
    finally:
        table_pipe.close()
        plain.close()
    h = C.c_void_p()
    p = pkg._lib.PipelineParams(rows=T, cols=T, channels=4, max_points=8192, filter_strength=FS, homography_method=8)
    assert L.apds_pipeline_create_table(C.byref(h), None, 0, C.byref(p)) == BAD and not h
    # stale world points: enable_pose refuses
    t = pkg.feature_database.KeypointTable(8)
    try:
        t.create_keypoints(_Ex(np.zeros(4, pkg._lib.KEYPOINT_DTYPE), np.zeros((4, 61), np.uint8)), 1, 0)
        pkg._lib.check(L.apds_pipeline_create_table(C.byref(h), t._h, 0, C.byref(p)))
        try:
            pp = pkg._lib.PipelinePoseParams(db_xyz_dev=None, camera_intrinsic=(C.c_double * 9)(*KMAT.ravel()), method=1)
            assert L.apds_pipeline_enable_pose(h, C.byref(pp)) == BAD
        finally:
            pkg._lib.check(L.apds_pipeline_destroy(h))
    finally:
        t.close()


def _summary(results):
    return [[r["status"], r["n_keypoints"], r["n_matches"], r["n_inliers"], None if r["H"] is None else [float(v).hex() for v in r["H"].ravel()]] for r in results]


def test_default_matcher_forced_off_gives_the_same_results(scene):
    """the same plan in a fresh child process with APDS_MATCH_MFMA=0 (the vector-ALU matcher scans the views)"""
    here = _summary(streamed(scene, PLAN))
    env = dict(os.environ, APDS_MATCH_MFMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = json.loads(r.stdout.strip().splitlines()[-1])
    assert there["backend_mfma"] == 0 and there["results"] == here


if __name__ == "__main__" and "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the library: one HIP runtime)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    pkg.lib()
    sc = Scene(pkg)
    try:
        be = C.c_int(-1)
        pkg._lib.check(pkg.lib().apds_dev_match_backend(C.byref(be)))
        print(json.dumps({"backend_mfma": be.value, "results": _summary(streamed(sc, PLAN))}))
    finally:
        sc.close()
