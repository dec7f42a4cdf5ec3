"""GPU: the pose stage of the streamed pipeline (apds_pipeline_enable_pose / apds_pipeline_poll_pose, csrc/pipeline.cpp; pose_worker in csrc/pipeline_stages.cpp) and the two device entry
points it is made of - apds_dev_pnp_correspondences (matches -> 2D-3D pairs, re-centred on an origin) and apds_dev_pnp_solver_ransac (the
RANSAC loop of apds_pnp_solver_ransac on device floats).

 * the device solver equals the host-array one on float-representable inputs (golden fixtures and seeded cases, every method, n = 3, 4, 5);
 * the gather equals numpy bit for bit and rejects an index outside the DB;
 * the mission chain (DB keypoint pixels -> world points -> streamed pose) equals the serial one-call path frame by frame, for four methods;
 * an anchor from the construction of the frames (a DB camera and its lateral move), not from either implementation;
 * enabling pose changes no frame result; frames without enough matches report APDS_ERR_ASSERT and the stream goes on; no memory growth;
 * a world-1 shard handle gives the one-GPU poses; a g++-built host (tests/cpp/pipeline_pose_test.cpp) runs the whole cycle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden  # noqa: E402

DGT = [9.0, 1e-4, 0, 57.0, 0, -1e-4]
EGT = [8.99, 3e-4, 0, 57.01, 0, -3e-4]
EPNP, ITERATIVE, P3P, AP3P, SQPNP, IPPE = 1, 0, 2, 5, 8, 6


def _setup(pkg, T=768, ndb=60000, nframes=3):
    """test_streamed_pipeline_gpu.py's set-up: the DB holds the descriptors (and keypoint pixels) of every frame rolled by (19, 23) rows /
    columns, then random rows."""
    import torch
    from importlib import import_module
    pl = import_module(pkg.__name__ + ".pipeline")
    L, check, synth = pkg.lib(), pkg._lib.check, pkg.synth
    dev = torch.device("cuda:0")
    frames_np = [synth.make_tile(T, T, frame_index=40 + i) for i in range(nframes)]
    frames = [torch.from_numpy(f).to(dev) for f in frames_np]
    cap = pkg.feature_extraction.MAX_POINTS
    kps = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    desc = torch.empty((cap, 64), dtype=torch.uint8, device=dev)
    rows, xy = [], []
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for f in frames_np:
            rolled = torch.from_numpy(np.roll(f, (19, 23), axis=(0, 1)).copy()).to(dev)
            n = C.c_int(0)
            check(L.apds_dev_akaze_extract(rolled.data_ptr(), T, T, 4, rolled.stride(0), cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n),
                                           pl.torch_stream()))
            rows.append(desc[:n.value].clone())
            xy.append(kps[:n.value, 0:2].clone())
            torch.cuda.synchronize()
    rows, xy = torch.cat(rows), torch.cat(xy)
    P = rows.shape[0]
    pad = np.zeros((ndb - P, 64), np.uint8)
    pad[:, :61] = synth.make_descriptor_db(ndb - P)
    db = torch.cat([rows, torch.from_numpy(pad).to(dev)]).contiguous()
    db_xy = torch.zeros((ndb, 2), dtype=torch.float32, device=dev)
    db_xy[:P] = xy
    torch.cuda.synchronize()
    return pl, frames, db, db_xy


@pytest.fixture(scope="module")
def scene(gpu_pkg):
    return _setup(gpu_pkg)


def _world(pkg, db_xy):
    """DB keypoint pixels -> ECEF metres through apds_get_world_coordinates (a geotransform and an elevation table as in
    test_world_coordinates_gpu.py)."""
    t = pkg.feature_database.ElevationTable()
    t.create_geotransform("dataset", DGT)
    t.create_geotransform("elevation", EGT)
    yy, xx = np.mgrid[0:500, 0:600]
    t.add_elevation_data(80 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + np.random.default_rng(4).uniform(0, 3, (500, 600)))
    return t.get_world_coordinates_batch(db_xy.cpu().numpy().astype(np.float64))


def _host_solve(pkg, obj, img, K, iters, thr, conf, method):
    n = len(obj)
    o = np.zeros((max(n, 1), 3)); o[:n] = obj
    i = np.zeros((max(n, 1), 2)); i[:n] = img
    rv, tv, inl = np.zeros(3), np.zeros(3), np.full(max(n, 1), -1, np.int32)
    ni, found = C.c_int(-1), C.c_int(-1)
    K = np.ascontiguousarray(K, np.float64)
    rc = pkg.lib().apds_pnp_solver_ransac(pkg._lib.ptr(o), pkg._lib.ptr(i), n, pkg._lib.ptr(K), iters, thr, conf, method, pkg._lib.ptr(rv), pkg._lib.ptr(tv),
                                          pkg._lib.ptr(inl), C.byref(ni), C.byref(found))
    return rc, found.value, rv, tv, inl[:max(ni.value, 0)].copy()


def _dev_solve(pkg, obj, img, K, iters, thr, conf, method, with_inliers=True):
    import torch
    n = len(obj)
    o = torch.zeros((max(n, 1), 3), dtype=torch.float32, device="cuda:0")
    i = torch.zeros((max(n, 1), 2), dtype=torch.float32, device="cuda:0")
    if n:
        o[:n] = torch.from_numpy(np.ascontiguousarray(obj, np.float32))
        i[:n] = torch.from_numpy(np.ascontiguousarray(img, np.float32))
    torch.cuda.synchronize()
    rv, tv, inl = np.zeros(3), np.zeros(3), np.full(max(n, 1), -1, np.int32)
    ni, found = C.c_int(-1), C.c_int(-1)
    K = np.ascontiguousarray(K, np.float64)
    rc = pkg.lib().apds_dev_pnp_solver_ransac(o.data_ptr(), i.data_ptr(), n, pkg._lib.ptr(K), iters, thr, conf, method, pkg._lib.ptr(rv), pkg._lib.ptr(tv),
                                              pkg._lib.ptr(inl) if with_inliers else None, C.byref(ni), C.byref(found), None)
    return rc, found.value, rv, tv, inl[:max(ni.value, 0)].copy() if with_inliers else ni.value


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1], (a[:2], b[:2])
    if a[0] == 0:
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_device_solver_equals_the_host_solver_on_the_fixtures(gpu_pkg):
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731 - float-representable inputs: both paths see the same floats
    obj, img, K = make_golden.pnp_inputs()
    obj, img = f32(obj), f32(img)
    g = np.load(os.path.join(ROOT, "tests", "golden", "pnp_400.npz"))
    g8 = np.load(os.path.join(ROOT, "tests", "golden", "pnp_sqpnp_400.npz"))
    for name, method, fx in (("epnp", EPNP, g), ("p3p", P3P, g), ("sqpnp", SQPNP, g8)):
        dev = _dev_solve(gpu_pkg, obj, img, K, 500, 3.0, 0.99, method)
        _same(dev, _host_solve(gpu_pkg, obj, img, K, 500, 3.0, 0.99, method))
        # (the fixtures were made from the doubles; solvePnPRansac rounds them to these floats first)
        assert dev[0] == 0 and dev[1] == 1 and np.array_equal(dev[4], fx[name + "_inliers"])
        assert np.array_equal(dev[2], fx[name + "_rvec"]) and np.array_equal(dev[3], fx[name + "_tvec"])
    po, pi, pK = make_golden.pnp_planar_inputs()
    po, pi = f32(po), f32(pi)
    g6 = np.load(os.path.join(ROOT, "tests", "golden", "pnp_ippe_400.npz"))
    dev = _dev_solve(gpu_pkg, po, pi, pK, 500, 3.0, 0.99, IPPE)
    _same(dev, _host_solve(gpu_pkg, po, pi, pK, 500, 3.0, 0.99, IPPE))
    assert dev[1] == 1 and np.array_equal(dev[4], g6["ippe_inliers"]) and np.array_equal(dev[2], g6["ippe_rvec"]) and np.array_equal(dev[3], g6["ippe_tvec"])


@pytest.mark.parametrize("n", [3, 4, 5, 6, 300])
def test_device_solver_equals_the_host_solver_for_every_method(gpu_pkg, n):
    for seed in (11, 12):
        obj, img, K, _, _, _ = gpu_pkg.synth.make_pnp_set(n, seed=0x5EED00 + seed * 7 + n, inlier_frac=0.7, noise=0.5)
        obj, img = np.asarray(obj, np.float32).astype(np.float64), np.asarray(img, np.float32).astype(np.float64)
        for method in range(9):
            want = _host_solve(gpu_pkg, obj, img, K, 200, 3.0, 0.99, method)
            got = _dev_solve(gpu_pkg, obj, img, K, 200, 3.0, 0.99, method)
            _same(got, want)
            if n < 4:
                assert got[0] == gpu_pkg._lib.ERR_ASSERT
            no_inl = _dev_solve(gpu_pkg, obj, img, K, 200, 3.0, 0.99, method, with_inliers=False)     # inliers = NULL: the count only
            assert no_inl[:2] == got[:2] and (got[0] != 0 or (np.array_equal(no_inl[2], got[2]) and no_inl[4] == len(got[4])))
    rc = _dev_solve(gpu_pkg, obj, img, K, 200, 3.0, 0.99, 9)[0]     # past cv::SolvePnPMethod (the count is checked first)
    assert rc == _host_solve(gpu_pkg, obj, img, K, 200, 3.0, 0.99, 9)[0] == (gpu_pkg._lib.ERR_ASSERT if n < 4 else gpu_pkg._lib.ERR_NOT_IMPLEMENTED)


def test_correspondence_gather_equals_numpy(gpu_pkg):
    import torch
    L, kd = gpu_pkg.lib(), gpu_pkg._lib.KEYPOINT_DTYPE
    rng = np.random.default_rng(21)
    nk, ndb, M = 5000, 70000, 3000
    kps = np.zeros(nk, kd)
    kps["x"], kps["y"] = rng.uniform(0, 4096, nk).astype(np.float32), rng.uniform(0, 4096, nk).astype(np.float32)
    xyz = np.array([3.5e6, 6.0e5, 5.3e6]) + rng.uniform(-3000, 3000, (ndb, 3))
    origin = xyz.mean(0)
    m = np.zeros(M, gpu_pkg._lib.DMATCH_DTYPE)
    m["query_idx"], m["train_idx"] = rng.integers(0, nk, M), rng.integers(0, ndb, M)
    dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to("cuda:0")     # noqa: E731
    dk, dx, dm = dev(kps), dev(xyz), dev(m)
    img = torch.zeros((M, 2), dtype=torch.float32, device="cuda:0")
    obj = torch.zeros((M, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    o = np.ascontiguousarray(origin)
    gpu_pkg._lib.check(L.apds_dev_pnp_correspondences(dk.data_ptr(), nk, dx.data_ptr(), ndb, gpu_pkg._lib.ptr(o), dm.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None))
    q, t = m["query_idx"], m["train_idx"]
    assert np.array_equal(img.cpu().numpy(), np.stack([kps["x"][q], kps["y"][q]], 1))
    want = np.float32(xyz[t] - origin)
    assert np.array_equal(obj.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a trainIdx past the DB's world points is rejected as apds_dev_points_from_matches rejects it
    m["train_idx"][17] = ndb
    dm = dev(m)
    torch.cuda.synchronize()
    rc = L.apds_dev_pnp_correspondences(dk.data_ptr(), nk, dx.data_ptr(), ndb, gpu_pkg._lib.ptr(o), dm.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None)
    assert rc == gpu_pkg._lib.ERR_OUT_OF_RANGE
    m["train_idx"][17], m["query_idx"][5] = 0, -1
    dm = dev(m)
    torch.cuda.synchronize()
    rc = L.apds_dev_pnp_correspondences(dk.data_ptr(), nk, dx.data_ptr(), ndb, gpu_pkg._lib.ptr(o), dm.data_ptr(), M, img.data_ptr(), obj.data_ptr(), None)
    assert rc == gpu_pkg._lib.ERR_OUT_OF_RANGE


def _equal_poses(a, b, i):
    pa, pb = a["pose"], b["pose"]
    assert (pa["status"], pa["found"], pa["n_correspondences"], pa["n_inliers"]) == (pb["status"], pb["found"], pb["n_correspondences"], pb["n_inliers"]), (i, pa, pb)
    assert np.array_equal(pa["rvec"], pb["rvec"]) and np.array_equal(pa["tvec"], pb["tvec"]), (i, pa, pb)


def test_mission_chain_streamed_poses_equal_the_serial_path(gpu_pkg, scene):
    """DB keypoint pixels -> ECEF (apds_get_world_coordinates) -> origin at their centroid -> 7 frames streamed with pose on, for four
    methods: every frame's pose equals the serial path (matches downloaded, pairs built on the host, apds_pnp_solver_ransac)."""
    pl, frames, db, db_xy = scene
    xyz = _world(gpu_pkg, db_xy)
    K = np.array([[4000.0, 0, 384], [0, 4000.0, 384], [0, 0, 1]])
    serial = pl.FramePipeline(db, db_xy)
    plain = pl.StreamedFramePipeline(db, db_xy)
    base, _ = plain.run(frames, 7, filter_strength=0.3)
    plain.close()
    for method in (EPNP, ITERATIVE, SQPNP, AP3P):
        pose = pl.PoseStage(xyz, K, method=method)
        assert np.array_equal(pose.origin, xyz.mean(0))
        want = [serial.step(frames[i % len(frames)], filter_strength=0.3, pose=pose) for i in range(7)]
        streamed = pl.StreamedFramePipeline(db, db_xy, pose=pose)
        try:
            got, _ = streamed.run(frames, 7, filter_strength=0.3)
        finally:
            streamed.close()
        for i, (a, b) in enumerate(zip(want, got)):
            _equal_poses(a, b, i)
            assert b["pose"]["status"] == 0 and b["pose"]["n_correspondences"] == b["n_matches"] > 100, (method, i, b["pose"])
            # enabling pose leaves the frame result as it was
            c = base[i]
            assert (b["n_keypoints"], b["n_matches"], b["n_inliers"], b["status"]) == (c["n_keypoints"], c["n_matches"], c["n_inliers"], c["status"])
            assert b["H"] is not None and np.array_equal(b["H"], c["H"])
        assert any(r["pose"]["found"] for r in got), method


def _rot(rv):
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def test_anchor_the_frame_camera_is_the_db_camera_moved_sideways(gpu_pkg, scene):
    """The DB points are made by back-projecting each DB keypoint (u, v) from a DB camera with R = I, focal length f = 500 px and principal
    point c = (384, 384) at depth Z = Z0 (1 + e s(u, v)), Z0 = 1000 m, e = 0.002, |s| <= 1 (relief). Every frame is the DB image shifted by
    (-23, -19) px, so its camera is the DB camera moved by C = (23, 19) Z0 / f = (46 m, 38 m, 0) with R = I: that camera sees a point of
    depth Z at u_db - 23 Z0 / Z, while the frame has it at u_db - 23. The construction is therefore exact up to a pixel error of
    23 |Z0/Z - 1| <= 23 e / (1 - e) = 0.046 px (relief), plus the keypoint noise: an integer shift moves the image content exactly, but the
    wrap-around seam changes AKAZE's global contrast factor a little, so take <= 0.1 px (matches at the seam are outliers; reproj_thres 3 px
    keeps them out). d = 0.15 px in all. The weak direction of a view of a near-plane is a rotation a about an in-plane axis traded against
    a translation a Z0: the two differ only by the second-order term f a th^2, th = 384 / 500 = 0.77 rad at the field's edge, so
    a <= d / (f th^2) = 5.1e-4 rad. Lateral camera error <= a Z0 + Z0 d / f = 0.81 m; depth error <= Z0 d / (f th) = 0.39 m (a scale change
    moves the edge by f th dZ / Z0). The bounds below are those times 3 (the estimates are first order): rotation 1.5e-3 rad, lateral
    2.4 m, depth 1.2 m; a pose that missed the move fails them by more than an order of magnitude. They hold for a solver that minimises
    the reprojection error (ITERATIVE: Levenberg-Marquardt; SQPNP: the global minimum of its objective). EPnP is not held to them: its four
    control points are ill-conditioned on points this close to a plane (0.023 rad of rotation traded against translation on a 3 % relief),
    a property of the method, not of the pipeline."""
    pl, frames, db, db_xy = scene
    f, c, Z0, e = 500.0, 384.0, 1000.0, 0.002
    uv = db_xy.cpu().numpy().astype(np.float64)
    s = np.sin(uv[:, 0] / 41.0) * np.cos(uv[:, 1] / 29.0)
    Z = Z0 * (1 + e * s)
    xyz = np.stack([(uv[:, 0] - c) * Z / f, (uv[:, 1] - c) * Z / f, Z], 1)
    K = np.array([[f, 0, c], [0, f, c], [0, 0, 1]])
    for method in (ITERATIVE, SQPNP):
        pose = pl.PoseStage(xyz, K, method=method, reproj_thres=3.0, iter_count=500)
        streamed = pl.StreamedFramePipeline(db, db_xy, pose=pose)
        try:
            got, _ = streamed.run(frames, 3, filter_strength=0.3)
        finally:
            streamed.close()
        for r in got:
            p = r["pose"]
            assert p["status"] == 0 and p["found"] == 1 and p["n_inliers"] > 100, p
            R = _rot(p["rvec"])
            centre = -R.T @ p["tvec"] + pose.origin           # the pose is relative to the origin
            angle = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
            print(method, "rotation %.2e rad, centre" % angle, centre)
            assert angle < 1.5e-3, (method, angle)
            assert abs(centre[0] - 46.0) < 2.4 and abs(centre[1] - 38.0) < 2.4 and abs(centre[2]) < 1.2, (method, centre)


def test_frames_without_enough_matches_report_assert_and_the_stream_goes_on(gpu_pkg):
    import torch
    pl, frames, db, db_xy = _setup(gpu_pkg, T=512, ndb=40000, nframes=2)
    xyz = _world(gpu_pkg, db_xy)
    K = np.array([[2000.0, 0, 256], [0, 2000.0, 256], [0, 0, 1]])
    rng = np.random.default_rng(3)
    blank = torch.zeros_like(frames[0])
    blank[..., 3] = 255
    noise = torch.from_numpy(rng.integers(0, 256, tuple(frames[0].shape), dtype=np.uint8)).to(frames[0].device)
    seq = [frames[0], blank, frames[1], noise, blank, blank, frames[0], noise, frames[1]]
    pose = pl.PoseStage(xyz, K)
    serial = pl.FramePipeline(db, db_xy)
    want = [serial.step(f, filter_strength=0.3, pose=pose) for f in seq]
    streamed = pl.StreamedFramePipeline(db, db_xy, pose=pose)
    try:
        got, _ = streamed.run(seq, len(seq), filter_strength=0.3)
    finally:
        streamed.close()
    for i, (a, b) in enumerate(zip(want, got)):
        assert b["status"] == 0 and a["n_matches"] == b["n_matches"], i
        _equal_poses(a, b, i)
        if b["n_matches"] < 4:
            assert b["pose"]["status"] == gpu_pkg._lib.ERR_ASSERT and b["pose"]["found"] == 0, (i, b["pose"])
    assert got[1]["n_keypoints"] == 0 and got[1]["pose"]["status"] == gpu_pkg._lib.ERR_ASSERT
    for i in (0, 2, 6, 8):
        assert got[i]["pose"]["status"] == 0 and got[i]["pose"]["n_correspondences"] > 100


def test_the_pose_thread_workspace_does_not_grow(gpu_pkg):
    import torch
    pl, frames, db, db_xy = _setup(gpu_pkg, T=512, ndb=70000, nframes=2)
    pose = pl.PoseStage(_world(gpu_pkg, db_xy), np.array([[2000.0, 0, 256], [0, 2000.0, 256], [0, 0, 1]]))
    streamed = pl.StreamedFramePipeline(db, db_xy, pose=pose)
    try:
        streamed.run(frames, 60, filter_strength=0.3)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            got, _ = streamed.run(frames, 120, filter_strength=0.3)
            assert all(r["pose"]["status"] == 0 for r in got)
        torch.cuda.synchronize()
        assert abs(torch.cuda.mem_get_info()[0] - free0) < 16 << 20
    finally:
        streamed.close()


def _native_poses(pkg, db, db_kp, shard, pose, frames, count):
    L, check = pkg.lib(), pkg._lib.check
    T = frames[0].shape[0]
    p = pkg._lib.PipelineParams(rows=T, cols=T, channels=4, filter_strength=0.3, homography_method=8)
    h = C.c_void_p()
    check(L.apds_pipeline_create(C.byref(h), None if shard else db.data_ptr(), 0 if shard else int(db.shape[0]), 0, shard, db_kp.data_ptr(), int(db.shape[0]),
                                 C.byref(p)))
    out = []
    try:
        pp = pose.params()
        check(L.apds_pipeline_enable_pose(h, C.byref(pp)))
        assert L.apds_pipeline_enable_pose(h, C.byref(pp)) == pkg._lib.ERR_BAD_ARG      # enabled once only
        for i in range(count):
            check(L.apds_pipeline_submit(h, frames[i % len(frames)].data_ptr(), T * 4, 1, None))
        assert L.apds_pipeline_enable_pose(h, C.byref(pp)) == pkg._lib.ERR_BAD_ARG       # after the first submit: refused
        r, fp = pkg._lib.FrameResult(), pkg._lib.FramePose()
        for i in range(count):
            check(L.apds_pipeline_poll_pose(h, C.byref(r), C.byref(fp), 1))
            assert r.frame == fp.frame == i and r.status == 0
            out.append((fp.status, fp.found, fp.n_correspondences, fp.n_inliers, tuple(fp.rvec), tuple(fp.tvec)))
    finally:
        check(L.apds_pipeline_destroy(h))
    return out


def test_a_world_one_shard_handle_gives_the_one_gpu_poses(gpu_pkg, scene):
    import torch
    pl, frames, db, db_xy = scene
    L, check = gpu_pkg.lib(), gpu_pkg._lib.check
    pose = pl.PoseStage(_world(gpu_pkg, db_xy), np.array([[4000.0, 0, 384], [0, 4000.0, 384], [0, 0, 1]]))
    db_kp = torch.zeros((db.shape[0], 7), dtype=torch.float32, device=db.device)
    db_kp[:, 0:2] = db_xy
    torch.cuda.synchronize()
    one = _native_poses(gpu_pkg, db, db_kp, None, pose, frames, 5)
    cid, sh = gpu_pkg._lib.CommId(), C.c_void_p()
    check(L.apds_comm_id_create(gpu_pkg._lib.TRANSPORT_LOOPBACK, C.byref(cid)))
    check(L.apds_shard_create(C.byref(sh), 0, 1, gpu_pkg._lib.TRANSPORT_LOOPBACK, C.byref(cid), None, db.data_ptr(), int(db.shape[0]), 0))
    try:
        sharded = _native_poses(gpu_pkg, db, db_kp, sh, pose, frames, 5)
    finally:
        check(L.apds_shard_destroy(sh))
    assert sharded == one
    assert all(p[0] == 0 and p[2] > 100 for p in one)


def test_a_cpp_host_streams_frames_with_pose(gpu_pkg, tmp_path):
    """tests/cpp/pipeline_pose_test.cpp (built by g++ as test_pipeline_pose_cpu.py builds it): create -> enable_pose -> submit / poll_pose ->
    destroy with frames in flight; every pose equals the one-call entry points' for that frame."""
    exe = str(tmp_path / "pipeline_pose_test")
    lib = os.path.join(ROOT, "cubesat-apds_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pipeline_pose_test.cpp"), "-o", exe, "-L", lib, "-lapds_hip", "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr[-4000:])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "... ok" in out.stdout and "0 failed" in out.stdout
