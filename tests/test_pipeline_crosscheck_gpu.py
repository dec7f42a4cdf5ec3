"""GPU: the streamed pipeline with the reference's second matcher (apds_pipeline_set_matcher, APDS_PIPELINE_MATCH_CROSSCHECK;
get_bruteforce_matches, lib.rs:116-126).

Frames are 256 x 256 (synth.py), the smallest the pipeline tests use. Every frame of a cross-check pipeline is compared with the serial
composition of the HOST one-call entry points: extraction -> apds_get_bruteforce_matches -> apds_get_points_from_matches ->
apds_find_homography and, with pose on, apds_pnp_solver_ransac: counts equal, H / rvec / tvec bit for bit. Whole-DB pipelines of 383, 384,
385 and 3000 rows (the borders of the swapped scan's 384 train columns per workgroup), made of the descriptors of the rolled frames plus
random rows; a table pipeline with alternating selections and every slot in flight; max_points forcing K = 1, 128, 129; a frame without
keypoints; a view with fewer than two rows; the contract errors; mode 0 set explicitly; no growth over 50 frames; the vector-ALU backend
in a child process."""
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
FS, THR, ITERS, CONF = 0.8, 3.0, 2000, 0.995                 # StreamedFramePipeline.run's defaults; apds_find_homography's are the last two
KMAT = np.array([[900.0, 0, 128], [0, 900.0, 128], [0, 0, 1]])
POSE = dict(method=1, iter_count=100, reproj_thres=8.0, confidence=0.99)
DB_SIZES = [383, 384, 385, 3000]


class _Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


class Scene:
    def __init__(self, pkg):
        import torch
        from importlib import import_module
        self.pkg, self.pl = pkg, import_module(pkg.__name__ + ".pipeline")
        fe, synth = pkg.feature_extraction, pkg.synth
        self.tiles = [synth.make_tile(T, T, frame_index=70 + i, blobs_per_mpx=20000) for i in range(2)]      # ~190 keypoints each
        blank = np.zeros_like(self.tiles[0])
        blank[..., 3] = 255
        self.tiles.append(blank)                                                                             # frame 2: no keypoints
        self.frames = [torch.from_numpy(f).to("cuda:0") for f in self.tiles]
        self.ex = [fe.akaze_keypoint_descriptor_extraction_def(np.roll(f, (19, 23), axis=(0, 1)).copy(), None) for f in self.tiles[:2]]
        assert min(len(e.keypoints) for e in self.ex) >= 150
        # the whole-DB train sets: 150 rows of each rolled frame, then random rows with random positions
        rng = np.random.default_rng(9)
        n = max(DB_SIZES)
        self.db_kps = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
        self.db_kps["x"], self.db_kps["y"] = rng.uniform(0, T - 1, n).astype(np.float32), rng.uniform(0, T - 1, n).astype(np.float32)
        self.db61 = synth.make_descriptor_db(n)
        for i, e in enumerate(self.ex):
            self.db61[150 * i:150 * i + 150] = e.descriptors[:150]
            self.db_kps[150 * i:150 * i + 150] = np.asarray(e.keypoints)[:150]
        self.db_xyz = np.stack([self.db_kps["x"] * 3.0, self.db_kps["y"] * 3.0, 40.0 * np.sin(self.db_kps["x"] / 17.0) + 1000.0], 1).astype(np.float64)
        # the table of the per-frame-view pipeline (tests/test_pipeline_table_view_gpu.py's layout)
        filler = np.zeros(400, pkg._lib.KEYPOINT_DTYPE)
        filler["x"], filler["y"], filler["response"] = rng.uniform(0, 255, 400), rng.uniform(0, 255, 400), rng.uniform(0, 0.01, 400)
        one = np.zeros(1, pkg._lib.KEYPOINT_DTYPE)
        rows = 2 * sum(len(e.keypoints) for e in self.ex) + len(filler) + 1
        self.table = t = pkg.feature_database.KeypointTable(rows)
        t.create_keypoints(self.ex[0], 1, 0, 0, 0, (T, T))
        t.create_keypoints(self.ex[1], 2, 0, 1, 0, (T, T))
        t.create_keypoints(_Ex(filler, synth.make_descriptor_db(400)), 3, 0, 2, 0, (T, T))
        t.create_keypoints(self.ex[0], 4, 1, 1, 0, (T, T))
        t.create_keypoints(self.ex[1], 5, 1, 0, 0, (T, T))
        t.create_keypoints(_Ex(one, np.zeros((1, 61), np.uint8)), 6, 2, 0, 0, (T, T))
        et = pkg.feature_database.ElevationTable()
        et.create_geotransform("dataset", [9.0, 1e-4, 0, 57.0, 0, -1e-4])
        assert t.world_coordinates(et) == 0
        s = self.pl.StreamedFramePipeline.selection
        self.sel = {"a0": s(2, 0, (0, 0, 255.5, 255.5)), "b0": s(2, 0, (257, 0, 511.5, 255.5)), "a1": s(2, 1, (513, 0, 1023, 511)), "b1": s(2, 1, (0, 0, 511, 511)),
                    "lod0": s(1, 0), "img4": s(0, 4), "empty": s(1, 9), "one": s(1, 2)}
        self._serial = {}

    def close(self):
        self.table.close()

    def db_tensors(self, nd):
        import torch
        rows = np.zeros((nd, 64), np.uint8)
        rows[:, :61] = self.db61[:nd]
        xy = np.stack([self.db_kps["x"][:nd], self.db_kps["y"][:nd]], 1)
        out = torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(xy)).to("cuda:0")
        torch.cuda.synchronize()
        return out

    def pose(self, nd):
        return self.pl.PoseStage(self.db_xyz[:nd], KMAT, **POSE)

    def view_on_host(self, sel):
        """apds_db_select's view of a selection, downloaded: (rows [n, 61], keypoints [n], table row ids [n])"""
        pkg = self.pkg
        L, check = pkg.lib(), pkg._lib.check
        nv = C.c_int(0)
        check(L.apds_db_select(self.table._h, sel.mode, sel.value, sel.x_start, sel.y_start, sel.x_end, sel.y_end, C.byref(nv)))
        rows64, vkps, vrows, _, nv = self.table.view_device_pointers()
        rows, kps, ids = np.zeros((nv, 64), np.uint8), np.zeros(nv, pkg._lib.KEYPOINT_DTYPE), np.zeros(nv, np.int32)
        if nv:
            check(L.apds_dev_download(pkg._lib.ptr(rows), rows64, rows.nbytes, None))
            check(L.apds_dev_download(pkg._lib.ptr(kps), vkps, kps.nbytes, None))
            check(L.apds_dev_download(pkg._lib.ptr(ids), vrows, ids.nbytes, None))
        return rows[:, :61].copy(), kps, ids


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    sc = Scene(gpu_pkg)
    yield sc
    sc.close()


def serial(sc, frame, train61, train_kps, max_points=None, pose=None, train_xyz=None):
    """one frame through the host one-call entry points; train_xyz: the train rows' world points when they are not pose.db_xyz's (a view)"""
    pkg = sc.pkg
    fe, L = pkg.feature_extraction, pkg.lib()
    ex = fe.akaze_keypoint_descriptor_extraction_def(sc.tiles[frame], max_points)
    kps, K = np.asarray(ex.keypoints), len(ex.keypoints)
    out = dict(status=0, n_keypoints=K, n_matches=0, n_inliers=0, H=None)
    m = np.zeros(0, pkg._lib.DMATCH_DTYPE)
    if len(train61) < 2:                     # what a train set of that size is to the pipeline
        out["status"] = pkg._lib.ERR_ASSERT
        if pose is not None:
            out["pose"] = sc.pl.pose_dict_of(pkg._lib.ERR_ASSERT, 0, 0, 0, np.zeros(3), np.zeros(3))
        return out
    if K:
        m = fe.get_bruteforce_matches(ex.descriptors, train61)
    M = out["n_matches"] = len(m)
    if M >= 4:
        p1, p2 = fe.get_points_from_matches(kps, train_kps, m)
        H, mask = np.zeros(9, np.float64), np.zeros(M, np.uint8)
        rc = L.apds_find_homography(pkg._lib.ptr(p1), pkg._lib.ptr(p2), M, 8, THR, pkg._lib.ptr(H), pkg._lib.ptr(mask))
        assert rc in (0, pkg._lib.ERR_EMPTY)
        if rc == 0:
            out["H"], out["n_inliers"] = H.reshape(3, 3), int(np.count_nonzero(mask))
    if pose is not None:
        q, t = m["query_idx"], m["train_idx"]
        img = np.stack([kps["x"][q], kps["y"][q]], 1) if M else np.zeros((0, 2))
        if train_xyz is None:
            out["pose"] = pose.solve(img, t)
        else:
            held, pose.db_xyz = pose.db_xyz, train_xyz
            try:
                out["pose"] = pose.solve(img, t)
            finally:
                pose.db_xyz = held
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


def streamed_db(sc, nd, order, matcher="crosscheck", max_points=8192, pose=None):
    """the whole-DB pipeline over the first nd rows: results of the frames `order` names, all submitted before the first poll"""
    db, db_xy = sc.db_tensors(nd)
    pipe = sc.pl.StreamedFramePipeline(db, db_xy, max_points=max_points, slots=max(6, len(order)), pose=pose, matcher=matcher)
    try:
        pipe.prepare(sc.frames[0].shape, FS, THR, ITERS, CONF)
        ids = C.c_int64(0)
        for f in order:
            ptr, stride, on_dev = pipe.frame_args(sc.frames[f])
            sc.pkg._lib.check(sc.pkg.lib().apds_pipeline_submit(pipe._pipe, ptr, stride, on_dev, C.byref(ids)))
        out = [pipe.poll() for _ in order]
        assert pipe.poll(wait=False) is None
        return out
    finally:
        pipe.close()


ORDER = [0, 1, 2, 1, 0, 0]            # frame 2 has no keypoints


@pytest.mark.parametrize("nd", DB_SIZES)
def test_whole_db_frames_equal_the_serial_composition(scene, oracle_mod, nd):
    pose = scene.pose(nd)
    want = {f: serial(scene, f, scene.db61[:nd], scene.db_kps[:nd], pose=pose) for f in set(ORDER)}
    assert want[0]["H"] is not None and want[1]["H"] is not None and want[2]["n_keypoints"] == 0 and want[2]["n_matches"] == 0
    # the count is the cross-check's, by the CPU oracle, and on these inputs it is not the ratio matcher's
    ex = scene.pkg.feature_extraction.akaze_keypoint_descriptor_extraction_def(scene.tiles[0], None)
    assert want[0]["n_matches"] == len(oracle_mod.get_bruteforce_matches(ex.descriptors, scene.db61[:nd]))
    assert want[0]["n_matches"] != len(oracle_mod.get_knn_matches(ex.descriptors, scene.db61[:nd], 2, FS))
    got = streamed_db(scene, nd, ORDER, pose=pose)
    for i, (f, g) in enumerate(zip(ORDER, got)):
        same(g, want[f], i)
    assert got[0]["pose"]["status"] == 0 and got[0]["pose"]["n_correspondences"] == got[0]["n_matches"]
    assert got[2]["pose"]["status"] == scene.pkg._lib.ERR_ASSERT
    # the ratio pipeline over the same rows reports another count: the matcher is really switched
    ratio = streamed_db(scene, nd, [0], matcher="ratio")[0]
    assert ratio["n_matches"] != got[0]["n_matches"]


@pytest.mark.parametrize("cap", [1, 128, 129])
def test_max_points_at_the_tile_borders_of_the_streamed_side(scene, cap):
    want = {f: serial(scene, f, scene.db61[:385], scene.db_kps[:385], max_points=cap) for f in (0, 1)}
    assert want[0]["n_keypoints"] == cap and want[1]["n_keypoints"] == cap
    got = streamed_db(scene, 385, [0, 1, 0], max_points=cap)
    for i, (f, g) in enumerate(zip([0, 1, 0], got)):
        same(g, want[f], i)


PLAN = [(0, "a0"), (1, "b0"), (0, "a1"), (1, "b1"), (0, "lod0"), (1, "lod0"), (0, "img4"), (1, "b0"), (0, "b0"), (2, "a0"), (0, "empty"), (1, "one")]


def streamed_table(sc, plan, pose=None, matcher="crosscheck"):
    pipe = sc.pl.StreamedFramePipeline.from_table(sc.table, per_frame_view=True, max_points=8192, slots=len(plan), pose=pose, matcher=matcher)
    try:
        pipe.prepare(sc.frames[0].shape, FS, THR, ITERS, CONF)
        for f, s in plan:                                   # every frame in flight before the first poll
            pipe.submit_select(sc.frames[f], sc.sel[s])
        out = [pipe.poll() for _ in plan]
        assert pipe.poll(wait=False) is None
        return out
    finally:
        pipe.close()


def serial_table(sc, plan, pose=None):
    out = []
    for f, s in plan:
        rows, kps, ids = sc.view_on_host(sc.sel[s])
        out.append(serial(sc, f, rows, kps, pose=pose, train_xyz=None if pose is None else pose.db_xyz[ids]))
    return out


def test_table_pipeline_frames_and_poses_equal_the_serial_composition(scene):
    pose = scene.pl.PoseStage.from_table(scene.table, KMAT, **POSE)
    want = serial_table(scene, PLAN, pose)
    assert sum(w["H"] is not None for w in want) >= 4 and sum(w["pose"]["status"] == 0 for w in want) >= 4
    got = streamed_table(scene, PLAN, pose=pose)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)
    # a view with fewer than two rows: today's status, in both modes
    ratio = streamed_table(scene, PLAN[-3:], matcher="ratio")
    for r in (got[-2], got[-1], ratio[-2], ratio[-1]):
        assert r["status"] == scene.pkg._lib.ERR_ASSERT and r["n_matches"] == 0 and r["H"] is None
    assert got[-3]["status"] == 0 and got[-3]["n_keypoints"] == 0


def _native(sc, nd, matcher, frames, shard=None):
    """create -> (set_matcher) -> submit / poll through the bound C functions; returns (set_matcher's status, results)"""
    import torch
    pkg = sc.pkg
    L, check = pkg.lib(), pkg._lib.check
    db, db_xy = sc.db_tensors(nd)
    kp = torch.zeros((nd, 7), dtype=torch.float32, device="cuda:0")
    kp[:, 0:2] = db_xy
    torch.cuda.synchronize()
    p = pkg._lib.PipelineParams(rows=T, cols=T, channels=4, max_points=8192, filter_strength=FS, homography_method=8)
    h = C.c_void_p()
    check(L.apds_pipeline_create(C.byref(h), None if shard else db.data_ptr(), 0 if shard else nd, 0, shard, kp.data_ptr(), nd, C.byref(p)))
    out, rc = [], 0
    try:
        if matcher is not None:
            rc = L.apds_pipeline_set_matcher(h, matcher)
        for f in frames:
            check(L.apds_pipeline_submit(h, sc.frames[f].data_ptr(), T * 4, 1, None))
        r = pkg._lib.FrameResult()
        for _ in frames:
            check(L.apds_pipeline_poll(h, C.byref(r), 1))
            out.append((r.status, r.n_keypoints, r.n_matches, r.n_inliers, r.homography_found, tuple(r.H)))
        late = L.apds_pipeline_set_matcher(h, 1) if frames else None
    finally:
        check(L.apds_pipeline_destroy(h))
    return rc, out, late


def test_contract_errors_and_the_explicit_default(scene):
    pkg = scene.pkg
    L, check, BAD = pkg.lib(), pkg._lib.check, pkg._lib.ERR_BAD_ARG
    assert L.apds_pipeline_set_matcher(None, 1) == BAD
    for bad in (-1, 2, 7):
        assert _native(scene, 385, bad, [])[0] == BAD
    # mode 0 set explicitly == nothing set; after the first submit the matcher is fixed
    rc0, explicit, late = _native(scene, 385, 0, [0, 1, 0])
    _, default, late2 = _native(scene, 385, None, [0, 1, 0])
    assert rc0 == 0 and explicit == default and late == BAD and late2 == BAD
    rc1, cross, _ = _native(scene, 385, 1, [0, 1, 0])
    assert rc1 == 0 and [c[2] for c in cross] != [d[2] for d in default]
    # a pipeline over a shard handle: the cross-check is not built, the ratio matcher is untouched
    db, _ = scene.db_tensors(385)
    cid, sh = pkg._lib.CommId(), C.c_void_p()
    check(L.apds_comm_id_create(pkg._lib.TRANSPORT_LOOPBACK, C.byref(cid)))
    check(L.apds_shard_create(C.byref(sh), 0, 1, pkg._lib.TRANSPORT_LOOPBACK, C.byref(cid), None, db.data_ptr(), 385, 0))
    try:
        assert _native(scene, 385, 1, [], shard=sh)[0] == pkg._lib.ERR_NOT_IMPLEMENTED
        assert _native(scene, 385, 3, [], shard=sh)[0] == BAD
        rc, sharded, _ = _native(scene, 385, 0, [0, 1], shard=sh)
        assert rc == 0 and sharded == default[:2]
    finally:
        check(L.apds_shard_destroy(sh))
    with pytest.raises(ValueError):
        scene.pl.StreamedFramePipeline(db, None, matcher="both")


def test_serial_front_gives_the_same_frames(scene):
    db, db_xy = scene.db_tensors(3000)
    fp = scene.pl.FramePipeline(db, db_xy, max_points=8192)
    got = streamed_db(scene, 3000, [0, 1])
    for f in (0, 1):
        s = fp.step(scene.frames[f], FS, THR, ITERS, CONF, matcher="crosscheck")
        assert (s["n_keypoints"], s["n_matches"], s["n_inliers"]) == (got[f]["n_keypoints"], got[f]["n_matches"], got[f]["n_inliers"])
        assert np.array_equal(s["H"], got[f]["H"])


def test_nothing_grows_over_fifty_frames(scene):
    import torch
    db, db_xy = scene.db_tensors(3000)
    whole = scene.pl.StreamedFramePipeline(db, db_xy, max_points=8192, matcher="crosscheck", pose=scene.pose(3000))
    table = scene.pl.StreamedFramePipeline.from_table(scene.table, per_frame_view=True, max_points=8192, matcher="crosscheck")
    sels = [scene.sel["a0"], scene.sel["b1"], scene.sel["lod0"]]
    try:
        whole.run(scene.frames[:2], 12)                  # every slot, every stage thread's workspace has been through a frame
        table.run(scene.frames[:2], 12, selections=sels)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        a, _ = whole.run(scene.frames[:2], 50)
        b, _ = table.run(scene.frames[:2], 50, selections=sels)
        torch.cuda.synchronize()
        assert abs(torch.cuda.mem_get_info()[0] - free0) < 4 << 20
        assert all(r["n_matches"] > 4 for r in a) and all(r["status"] == 0 for r in b)
    finally:
        whole.close()
        table.close()


def _summary(results):
    return [[r["status"], r["n_keypoints"], r["n_matches"], r["n_inliers"], None if r["H"] is None else [float(v).hex() for v in r["H"].ravel()]] for r in results]


def _both(sc):
    return {"db385": _summary(streamed_db(sc, 385, ORDER)), "db3000": _summary(streamed_db(sc, 3000, ORDER)), "table": _summary(streamed_table(sc, PLAN))}


def test_vector_backend_gives_the_same_results(scene):
    """the same frames in a fresh child process with APDS_MATCH_MFMA=0: the vector-ALU kernel serves the swapped scan directly"""
    here = _both(scene)
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
        print(json.dumps({"backend_mfma": be.value, "results": _both(sc)}))
    finally:
        sc.close()
