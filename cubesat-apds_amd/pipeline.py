"""Device-resident composition of the hot path and its multi-GPU form (python fronts of the C ABI's apds_shard_* and apds_pipeline_*).

frame (u8, HBM) -> AKAZE -> descriptors -> Hamming top-2 against a resident descriptor DB -> ratio test ->
matched points -> RANSAC homography.  The reference only chains these steps inside unit tests
(/root/reference/feature_extraction/src/lib.rs:197-249) and never calls find_homography_mat on the result; this
module is the composed pipeline the north-star metric (frames/s) is measured on.

Multi-GPU (one process per GPU, torch.distributed; backend "nccl" is RCCL on ROCm):
  * the descriptor DB is row-sharded: rank r holds rows [base_r, base_r + n_r) resident in its HBM;
  * frames are data-parallel: every rank extracts its own frame;
  * the only exchange is in the match step, and it lives behind the C ABI (apds_shard_*, csrc/shard_core.h): all-gather of the
    ranks' query descriptors, local top-k of ALL queries against the local shard, all-to-all of the per-shard top-k keys
    (packed u64 = distance << 32 | global row), then each rank merges the candidates of its own queries.
    u64 min-merge reproduces the single-GPU result exactly, including the lowest-index tie break.
torch is used for device buffers and streams only; every compute step is a libapds_hip kernel and the collectives are the library's
(RCCL; or the host-callback transport over a gloo group when several ranks share one GPU).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check, lib

EMPTY_KEY = -1  # 0xFFFF_FFFF_FFFF_FFFF as int64


def torch_stream():
    """torch's current HIP stream as the void* the C ABI takes, so kernels, torch ops and collectives are ordered on ONE
    stream. torch's default stream has handle 0, which the C ABI reads as "the calling thread's own stream" (a different,
    non-blocking stream): callers must therefore work inside `with torch.cuda.stream(torch.cuda.Stream())`."""
    h = torch.cuda.current_stream().cuda_stream
    if h == 0:
        raise RuntimeError("run the pipeline under an explicit torch.cuda.Stream (the default stream's handle is NULL)")
    return C.c_void_p(h)


def _gather_into(dist, group, dst, src):
    """all_gather_into_tensor that also works for the gloo rehearsal backend with device tensors (staged through the host). Used by
    bench.py's SETUP only (building the shared DB); the per-frame exchange is the C ABI's (apds_shard_*)."""
    if dist.get_backend(group) == "gloo" and src.is_cuda:
        d, s = torch.empty(dst.shape, dtype=dst.dtype), src.cpu()
        dist.all_gather_into_tensor(d.view(-1), s.view(-1), group=group)
        dst.copy_(d)
    else:
        dist.all_gather_into_tensor(dst.view(-1), src.view(-1), group=group)


def host_transport_from_group(dist, group):
    """apds_host_transport (include/apds.h) over a torch.distributed process group whose collectives take HOST tensors (gloo): the two
    callbacks wrap the library's staging buffers as tensors without copying. This is what carries the exchange step when several ranks
    share one GPU (the one-GPU rehearsal of bench.py, APDS_BENCH_BACKEND=gloo) and in the CPU tests. Returns the ctypes struct; it keeps
    the callback objects alive."""
    world = dist.get_world_size(group)

    def view(addr, n):
        if not n:
            return torch.empty(0, dtype=torch.uint8)
        return torch.from_numpy(np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint8)), shape=(int(n),)))

    def all_gather(_user, send, recv, nbytes):
        try:
            dist.all_gather_into_tensor(view(recv, nbytes * world), view(send, nbytes), group=group)
            return 0
        except Exception:   # noqa: BLE001 - an exception must not unwind through the C frames
            import traceback
            traceback.print_exc()
            return 1

    def all_to_all(_user, send, soff, sbytes, recv, roff, rbytes):
        try:
            so, sb, ro, rb = ([int(a[p]) for p in range(world)] for a in (soff, sbytes, roff, rbytes))
            # all_to_all_single wants the blocks back to back in rank order, which is how the matcher lays them out
            assert all(so[p] == sum(sb[:p]) for p in range(world)) and all(ro[p] == sum(rb[:p]) for p in range(world)), "blocks are not contiguous"
            dist.all_to_all_single(view(recv, sum(rb)), view(send, sum(sb)), output_split_sizes=rb, input_split_sizes=sb, group=group)
            return 0
        except Exception:   # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    ht = _lib.HostTransport(None, _lib.HOST_ALL_GATHER(all_gather), _lib.HOST_ALL_TO_ALL(all_to_all))
    ht._keep = (all_gather, all_to_all)
    return ht


class _DevBytes:
    """A library-owned device buffer as something torch.as_tensor can wrap without a copy (__cuda_array_interface__; ROCm builds read it too)."""

    def __init__(self, addr, nbytes):
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(addr), False), "version": 2, "strides": None}


def _table_tensor(addr, nbytes, device, dtype, shape):
    """A column of a KeypointTable (feature_database.py: device_table()) as a torch tensor on its memory, no copy."""
    return torch.as_tensor(_DevBytes(addr, nbytes), device=device).view(dtype).view(shape)


def device_transport_from_group(dist, group, device):
    """apds_device_transport (include/apds.h) over a torch.distributed process group whose collectives take DEVICE tensors ("nccl" = RCCL):
    the library's exchange buffers are wrapped as tensors in place and the collectives are issued on the stream the library names, so the
    exchange travels over torch's own RCCL communicator. The second way onto xGMI: bench.py falls back to it (--transport torch) if the
    library's own communicator (APDS_TRANSPORT_RCCL: ncclCommInitRank beside torch's) cannot be set up on a node."""
    world = dist.get_world_size(group)

    def view(addr, n):
        if not n:
            return torch.empty(0, dtype=torch.uint8, device=device)
        return torch.as_tensor(_DevBytes(addr, n), device=device)

    def all_gather(_user, send, recv, nbytes, stream):
        try:
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=device)):
                dist.all_gather_into_tensor(view(recv, nbytes * world), view(send, nbytes), group=group)
            return 0
        except Exception:   # noqa: BLE001 - an exception must not unwind through the C frames
            import traceback
            traceback.print_exc()
            return 1

    def all_to_all(_user, send, soff, sbytes, recv, roff, rbytes, stream):
        try:
            so, sb, ro, rb = ([int(a[p]) for p in range(world)] for a in (soff, sbytes, roff, rbytes))
            assert all(so[p] == sum(sb[:p]) for p in range(world)) and all(ro[p] == sum(rb[:p]) for p in range(world)), "blocks are not contiguous"
            with torch.cuda.stream(torch.cuda.ExternalStream(int(stream), device=device)):
                dist.all_to_all_single(view(recv, sum(rb)), view(send, sum(sb)), output_split_sizes=rb, input_split_sizes=sb, group=group)
            return 0
        except Exception:   # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    dt = _lib.DeviceTransport(None, _lib.DEV_ALL_GATHER(all_gather), _lib.DEV_ALL_TO_ALL(all_to_all))
    dt._keep = (all_gather, all_to_all)
    return dt


class GatheredQueries:
    """One frame's exchange slot of a shard handle (apds_shard_slot_create): the buffers live in the library; `merged` is where
    exchange_merge leaves the keys when the caller passes no output tensor."""

    def __init__(self, matcher, max_queries, kmax):
        self.matcher, self.kmax = matcher, kmax
        self.handle = C.c_void_p()
        check(lib().apds_shard_slot_create(matcher.handle, int(max_queries), int(kmax), C.byref(self.handle)))
        self.pad = -(-max(int(max_queries), 1) // 1024) * 1024
        self.merged = torch.empty((self.pad, kmax), dtype=torch.int64, device=matcher.rows.device)
        self.counts, self.total, self.nq = None, 0, 0

    def close(self):
        h, self.handle = self.handle, None
        if h and self.matcher.handle:
            lib().apds_shard_slot_destroy(self.matcher.handle, h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass


class ShardedMatcher:
    """Hamming k-NN of per-rank query sets against a row-sharded resident DB: a thin front of the C ABI's apds_shard_* (csrc/shard.cpp,
    csrc/shard_core.h), which owns the whole choreography - all-gather of the ranks' query rows, local top-k of all of them against the
    local shard with global row indices, all-to-all of the keys, u64-min merge (= the single-GPU result, lowest-index tie-break
    included). What this class adds is the choice of transport from the torch process group it is given:
      * no group / one rank: no exchange step, the scan is called directly;
      * a "nccl" group: the library's RCCL transport (its own communicator; rank 0's id travels through the torch group once), or -
        transport="torch" - device callbacks that run the same two collectives through torch.distributed on that group;
      * a "gloo" group: the host-callback transport over that group (several ranks on one GPU: rehearsal).
    The three steps are separate calls (gather_queries / scan_gathered / exchange_merge) so that a pipeline can issue frame i+1's query
    gather on another stream BEFORE frame i's key exchange. All collective calls must come from ONE thread in the same order on every
    rank. No per-frame allocations."""

    def __init__(self, local_rows64, index_base, group=None, pad_rows=32768, meta_group=None, kmax=2, always_exchange=False, transport="rccl"):
        self.rows = local_rows64            # borrowed by the shard handle for its whole life
        self.index_base = int(index_base)
        self.group = group
        self.meta_group = meta_group      # optional host-side (gloo) group for the per-frame query counts
        self.pad_rows = pad_rows          # smallest slot capacity (rows per rank)
        self.kmax = kmax
        self.always_exchange = always_exchange   # run the collectives even with one rank (RCCL self-test on a one-GPU box)
        self._own = None                  # slot of the plain knn() form
        self.handle = None
        self.transport = "none"
        if group is not None:
            import torch.distributed as dist
            self.dist = dist
            self.world = dist.get_world_size(group)
            self.rank = dist.get_rank(group)
        else:
            self.dist, self.world, self.rank = None, 1, 0
        if self.world == 1 and not (always_exchange and self.dist is not None):
            return
        L, dist = lib(), self.dist
        backend = dist.get_backend(group)
        h = C.c_void_p()
        n_rows = int(local_rows64.shape[0])
        if backend == "nccl" and transport == "torch":
            # the exchange over torch's own RCCL communicator: device callbacks on this group
            self._dev_transport = device_transport_from_group(dist, group, local_rows64.device)
            check(L.apds_shard_create(C.byref(h), self.rank, self.world, _lib.TRANSPORT_DEVICE, None, C.byref(self._dev_transport), local_rows64.data_ptr(), n_rows,
                                      self.index_base))
            self.transport = "device-callbacks (torch.distributed nccl)"
        elif backend == "nccl":
            # rank 0 creates the RCCL id; 128 bytes through the torch group; every rank then joins the library's own communicator
            cid = _lib.CommId()
            if self.rank == 0:
                check(L.apds_comm_id_create(_lib.TRANSPORT_RCCL, C.byref(cid)))
            t = torch.frombuffer(bytearray(bytes(cid)), dtype=torch.uint8).to(local_rows64.device)
            dist.broadcast(t, src=dist.get_global_rank(group, 0) if hasattr(dist, "get_global_rank") else 0, group=group)
            C.memmove(C.byref(cid), bytes(t.cpu().numpy().tobytes()), _lib.COMM_ID_BYTES)
            check(L.apds_shard_create(C.byref(h), self.rank, self.world, _lib.TRANSPORT_RCCL, C.byref(cid), None, local_rows64.data_ptr(), n_rows, self.index_base))
            self.transport = "rccl"
        else:
            self._host_transport = host_transport_from_group(dist, group)
            check(L.apds_shard_create(C.byref(h), self.rank, self.world, _lib.TRANSPORT_HOST, None, C.byref(self._host_transport), local_rows64.data_ptr(), n_rows,
                                      self.index_base))
            self.transport = "host-callbacks (%s)" % backend
        self.handle = h

    def close(self):
        if self._own is not None:
            self._own.close()
            self._own = None
        h, self.handle = self.handle, None
        if h:
            lib().apds_shard_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass

    def info(self):
        """{rank, world, rows, index_base, transport, rccl_version} as the library reports them."""
        if not self.handle:
            return dict(rank=0, world=1, rows=int(self.rows.shape[0]), index_base=self.index_base, transport="none (one rank)", rccl_version=None)
        r, w, ver, n, base, name = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_uint32(), C.c_char_p()
        check(lib().apds_shard_info(self.handle, C.byref(r), C.byref(w), C.byref(n), C.byref(base), C.byref(name), C.byref(ver)))
        return dict(rank=r.value, world=w.value, rows=n.value, index_base=base.value, transport=name.value.decode(), rccl_version=ver.value)

    def exchange_counts(self, nq):
        """Every rank's query count for one frame, as host ints, through the host-side group: no device work and no stream
        synchronisation, so the thread that later issues the match keeps queueing kernels ahead of the GPU. Must be called
        once per frame, in frame order, by the same thread on every rank."""
        if self.handle is None:
            return [int(nq)]
        if self.meta_group is None:
            return None
        t = torch.tensor([int(nq)], dtype=torch.int64)
        o = torch.empty(self.world, dtype=torch.int64)
        self.dist.all_gather_into_tensor(o, t, group=self.meta_group)
        return [int(v) for v in o.tolist()]

    def make_buffers(self, max_queries=None, k=None):
        """An exchange slot for frames of at most `max_queries` queries per rank (one per frame in flight)."""
        return GatheredQueries(self, max(self.pad_rows, int(max_queries or 0)), k or self.kmax)

    @staticmethod
    def _counts_arg(counts):
        return (C.c_int * len(counts))(*[int(c) for c in counts])

    def gather_queries(self, q_rows64, counts, buf):
        """Step (1) on the CURRENT stream (collective): afterwards the slot holds every rank's queries."""
        nq = int(q_rows64.shape[0])
        buf.counts, buf.total, buf.nq = list(counts), int(sum(counts)), nq
        check(lib().apds_shard_gather(self.handle, buf.handle, q_rows64.data_ptr() if nq else None, nq, self._counts_arg(counts), torch_stream()))
        return buf

    def scan_gathered(self, buf, k=2):
        """Step (2) on the CURRENT stream: this shard's top-k of every gathered query (no collective; waits for the gather's event)."""
        check(lib().apds_shard_scan(self.handle, buf.handle, k, torch_stream()))

    def exchange_merge(self, buf, k=2, out=None):
        """Steps (3)-(4) on the CURRENT stream (the one scan_gathered ran on; collective): all-to-all of the keys, then the per-query merge."""
        nq = buf.nq
        dst = out[:nq] if out is not None else buf.merged[:nq, :k] if k == buf.kmax else torch.empty((nq, k), dtype=torch.int64, device=self.rows.device)
        check(lib().apds_shard_exchange_merge(self.handle, buf.handle, k, dst.data_ptr() if nq else None, torch_stream()))
        return dst

    def match_gathered(self, buf, k=2, out=None):
        """Steps (2)-(4) on the CURRENT stream for a frame whose queries gather_queries() has put into `buf`."""
        self.scan_gathered(buf, k)
        return self.exchange_merge(buf, k, out=out)

    def knn(self, q_rows64, k=2, out=None, counts=None):
        """q_rows64: this rank's queries [Q_r, 64] u8. Returns [Q_r, k] int64 keys over the WHOLE DB. `counts`: every rank's
        query count (exchange_counts); without it the library exchanges them first, which costs a host synchronisation."""
        nq = int(q_rows64.shape[0])
        dst = out[:nq] if out is not None else torch.empty((nq, k), dtype=torch.int64, device=q_rows64.device)
        if self.handle is None:
            check(lib().apds_dev_hamming_topk(q_rows64.data_ptr(), nq, self.rows.data_ptr(), int(self.rows.shape[0]), self.index_base, k, dst.data_ptr(), torch_stream()))
            return dst
        check(lib().apds_shard_knn(self.handle, q_rows64.data_ptr() if nq else None, nq, self._counts_arg(counts) if counts is not None else None, k,
                                   dst.data_ptr() if nq else None, torch_stream()))
        return dst


def _matcher_code(matcher):
    """"ratio" | "crosscheck" | "l2" -> APDS_PIPELINE_MATCH_*"""
    try:
        return _lib.PIPELINE_MATCHERS[matcher]
    except (KeyError, TypeError):
        raise ValueError('matcher: "ratio" (get_knn_matches, lib.rs:94-114), "crosscheck" (get_bruteforce_matches, lib.rs:116-126) or "l2" '
                         '(float descriptors: get_knn_matches_l2)') from None


class L2TrainSet:
    """A resident float train set (apds_l2_train_*): rows_f32 is a [N, dim] float32 device tensor, borrowed (and kept alive) until close()
    and unchanged meanwhile. The norms, the bf16 copy and the largest norm the screen needs are made once, here. top2() gives the keys of
    apds_dev_l2_topk(k = 2) on the same rows, bit for bit, in either mode."""

    def __init__(self, rows_f32, index_base=0):
        if rows_f32.dtype != torch.float32 or rows_f32.dim() != 2 or not rows_f32.is_contiguous():
            raise ValueError("rows_f32: a contiguous [N, dim] float32 device tensor")
        self.rows, self.index_base = rows_f32, int(index_base)
        h = C.c_void_p()
        n, dim = int(rows_f32.shape[0]), int(rows_f32.shape[1])
        check(lib().apds_l2_train_create(C.byref(h), rows_f32.data_ptr() if n else None, n, dim, self.index_base))
        self._h = h
        self._owner = None
        self.mode_used, self.candidates_per_query = None, 0.0     # of the last top2()

    @classmethod
    def of_view(cls, view):
        """The train set a float KeypointTable's TableView keeps over its last selection (TableView.l2_train()): borrowed from the view, which
        it keeps alive; it follows every select of the view, and close() only lets go of it."""
        self = cls.__new__(cls)
        self.rows, self.index_base = None, 0
        self._h, self._owner = view.l2_train(), view
        self.mode_used, self.candidates_per_query = None, 0.0
        return self

    def info(self):
        """(n_train, dim, screen_ready)"""
        n, dim, ready = C.c_int64(0), C.c_int(0), C.c_int(0)
        check(lib().apds_l2_train_info(self._h, C.byref(n), C.byref(dim), C.byref(ready)))
        return n.value, dim.value, bool(ready.value)

    def top2(self, q, mode="screen", out=None):
        """q: [Q, dim] float32 device tensor -> [Q, 2] int64 keys (f32 bits of d^2 << 32 | row + index_base) on the CURRENT stream. What ran
        and the re-ranked rows per query are left in .mode_used ("exact" | "screen") and .candidates_per_query."""
        nq = int(q.shape[0])
        dst = out[:nq] if out is not None else torch.empty((nq, 2), dtype=torch.int64, device=q.device)
        used, cpq = C.c_int(-1), C.c_double(0)
        check(lib().apds_dev_l2_train_top2(self._h, q.data_ptr() if nq else None, nq, _lib.L2_MODES[mode], dst.data_ptr() if nq else None, torch_stream(),
                                           C.byref(used), C.byref(cpq)))
        self.mode_used, self.candidates_per_query = ("exact", "screen")[used.value], cpq.value
        return dst

    def close(self):
        h, self._h = self._h, None
        owner, self._owner = self._owner, None
        if h is not None and owner is None:     # (a view's train set is the view's)
            check(lib().apds_l2_train_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass


def dev_l2_ratio_filter(keys, filter_strength, out=None):
    """apds_dev_l2_ratio_filter on the CURRENT stream: keys [Q, k >= 2] int64 of an L2 matcher -> the matches of get_knn_matches_l2 as a
    [M, 4] int32 device tensor (16-byte cv::DMatch rows: query, train, image, distance as f32 bits) in query order - a view of `out`
    ([>= Q, 4] int32) when given."""
    nq, k = int(keys.shape[0]), int(keys.shape[1])
    dst = out if out is not None else torch.empty((max(nq, 1), 4), dtype=torch.int32, device=keys.device)
    n = C.c_int(0)
    check(lib().apds_dev_l2_ratio_filter(keys.data_ptr() if nq else None, nq, k, float(filter_strength), dst.data_ptr(), C.byref(n), torch_stream()))
    return dst[:n.value]


def dev_crosscheck_match(q_rows64, t_rows64, index_base=0, out=None):
    """apds_dev_crosscheck_match on the CURRENT stream: get_bruteforce_matches (BFMatcher crossCheck = true, lib.rs:116-126) of device rows
    [Q, 64] u8 against [N, 64] u8. Returns the matches as a [M, 4] int32 device tensor (16-byte cv::DMatch rows: query, train + index_base,
    image, distance as f32 bits) in query order - a view of `out` ([>= Q, 4] int32) when given."""
    nq, nt = int(q_rows64.shape[0]), int(t_rows64.shape[0])
    dst = out if out is not None else torch.empty((max(nq, 1), 4), dtype=torch.int32, device=q_rows64.device)
    n = C.c_int(0)
    check(lib().apds_dev_crosscheck_match(q_rows64.data_ptr() if nq else None, nq, t_rows64.data_ptr() if nt else None, nt, int(index_base), dst.data_ptr(),
                                          C.byref(n), torch_stream()))
    return dst[:n.value]


def dev_undistort_points(points, camera_matrix, dist_coeffs, iters=5):
    """apds_dev_undistort_points on the CURRENT stream, in place: `points` is a device tensor of f32 rows whose first two elements are
    (x, y) - [n, 2] points, [n, 7] keypoint rows (28 bytes), or any row stride of at least 8 bytes; only x and y are rewritten, each pair
    widened to f64, undistorted by `iters` steps (<= 0: 5) and rounded once. Returns `points`."""
    n = int(points.shape[0]) if points.dim() == 2 else -1
    if points.dtype != torch.float32 or n < 0 or points.shape[1] < 2 or (n > 0 and points.stride(1) != 1):
        raise ValueError("points: a [n, >= 2] float32 device tensor with unit column stride")
    K, d, pK, pd, nd = _lib.lens_args(camera_matrix, dist_coeffs)
    stride = int(points.stride(0)) * 4 if n > 1 else 4 * int(points.shape[1])     # (an empty or one-row tensor's row stride means nothing)
    check(lib().apds_dev_undistort_points(points.data_ptr() if n else None, n, stride, pK, pd, nd, int(iters), torch_stream()))
    return points


SOLVEPNP_EPNP = 1


class PoseStage:
    """The pose stage of a pipeline (apds_pipeline_enable_pose): every frame's ratio-filtered matches -> 2D-3D pairs -> PnP RANSAC
    (homographier::pnp_solver_ransac, mod.rs:320-369). db_xyz: [N_total, 3] world points (e.g. ECEF metres from
    feature_database.ElevationTable.get_world_coordinates_batch, elevationdb.rs:64-104) of EVERY DB row, indexed by global row like the
    DB keypoints. solvePnPRansac works in f32, which resolves ECEF magnitudes to 0.5 m only, so the points are re-centred on `origin` (in
    double, then rounded once) and the pose that comes back is relative to it; origin None = the centroid of db_xyz. method: APDS_SOLVEPNP_*
    (default EPnP, mod.rs:359); iter_count <= 0 -> 100, reproj_thres <= 0 -> 8.0, confidence outside (0, 1) -> 0.99 (solvePnPRansac's
    defaults)."""

    def __init__(self, db_xyz, camera_intrinsic, origin=None, method=SOLVEPNP_EPNP, iter_count=100, reproj_thres=8.0, confidence=0.99, device="cuda:0",
                 db_xyz_dev=None):
        xyz = db_xyz.detach().cpu().numpy() if isinstance(db_xyz, torch.Tensor) else np.asarray(db_xyz)
        self.db_xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        self.origin = np.asarray(self.db_xyz.mean(0) if origin is None else origin, np.float64).reshape(3).copy()
        self.K = np.ascontiguousarray(camera_intrinsic, np.float64).reshape(3, 3)
        self.method, self.iter_count, self.reproj_thres, self.confidence = int(method), int(iter_count), float(reproj_thres), float(confidence)
        # borrowed by the native pipeline for its whole life (db_xyz_dev: the same points already on the device, taken instead of an upload)
        self.db_xyz_dev = torch.from_numpy(self.db_xyz).to(device) if db_xyz_dev is None else db_xyz_dev

    @classmethod
    def from_table(cls, table, camera_intrinsic, origin=None, device="cuda:0", **kw):
        """The pose stage over the world points a KeypointTable holds on the device (table.world_coordinates() must have run since the last
        insert): the native pipeline reads the table's own xyz column. The stage keeps the table alive; the column holds until the table's
        next insert. The host copy (solve(), the default origin) is a download of that column."""
        _, _, xyz, n = table.device_table()
        if not xyz or n <= 0:
            raise ValueError("the table has no current world points: call table.world_coordinates(elevation_table) after the last insert")
        dev = _table_tensor(xyz, n * 24, device, torch.float64, (n, 3))
        self = cls(dev, camera_intrinsic, origin, device=device, db_xyz_dev=dev, **kw)
        self._table = table
        return self

    def params(self):
        return _lib.PipelinePoseParams(db_xyz_dev=self.db_xyz_dev.data_ptr(), origin=(C.c_double * 3)(*self.origin), camera_intrinsic=(C.c_double * 9)(*self.K.ravel()),
                                       method=self.method, iter_count=self.iter_count, reproj_thres=self.reproj_thres, confidence=self.confidence)

    def solve(self, img_xy, train_idx):
        """The established one-call path on host pairs: img_xy [M, 2] (the frame keypoints' pixels), train_idx [M] (global DB rows) ->
        apds_pnp_solver_ransac on (db_xyz[train_idx] - origin, img_xy). Returns the pose dict the pipeline gives."""
        M = int(len(train_idx))
        obj = np.zeros((max(M, 1), 3), np.float64)
        img = np.zeros((max(M, 1), 2), np.float64)
        obj[:M] = self.db_xyz[np.asarray(train_idx, np.int64)] - self.origin
        img[:M] = np.asarray(img_xy, np.float64)
        rvec, tvec = np.zeros(3, np.float64), np.zeros(3, np.float64)
        inl = np.zeros(max(M, 1), np.int32)
        n_inl, found = C.c_int(0), C.c_int(0)
        K = np.ascontiguousarray(self.K)
        rc = lib().apds_pnp_solver_ransac(_lib.ptr(obj), _lib.ptr(img), M, _lib.ptr(K), self.iter_count, self.reproj_thres, self.confidence, self.method,
                                          _lib.ptr(rvec), _lib.ptr(tvec), _lib.ptr(inl), C.byref(n_inl), C.byref(found))
        if rc != 0:
            return pose_dict_of(rc, 0, M, 0, np.zeros(3), np.zeros(3))
        return pose_dict_of(0, found.value, M, n_inl.value, rvec, tvec)


def pose_dict_of(status, found, n_correspondences, n_inliers, rvec, tvec):
    return dict(status=int(status), found=int(found), n_correspondences=int(n_correspondences), n_inliers=int(n_inliers),
                rvec=np.array(rvec, np.float64).reshape(3), tvec=np.array(tvec, np.float64).reshape(3))


class FramePipeline:
    """One rank's resident state: frames, DB shard (+ the DB rows' keypoint coordinates), output buffers."""

    def __init__(self, db_rows64, db_xy, index_base=0, group=None, max_points=(1 << 18) - 1, device="cuda:0"):
        self.dev = torch.device(device)
        self.stream = torch.cuda.Stream(self.dev)
        # float rows ([N, 64] float32: step(.., matcher="l2")) are held as they are; the Hamming matcher's front takes byte rows only
        self.float_rows = db_rows64.dtype == torch.float32
        if self.float_rows and group is not None:
            raise ValueError("float32 DB rows (the L2 matcher) are matched on one GPU: there is no sharded float matcher, group must be None")
        self.matcher = ShardedMatcher(db_rows64, index_base, group)
        self.desc_f32 = None               # [cap, 64] float32, made by the first float step
        self.db_xy_all = db_xy                      # [N_total, 2] f32 on device (replicated: 8 B/row)
        self.cap = max_points
        self.kps = torch.empty((self.cap, 7), dtype=torch.float32, device=self.dev)       # 28-byte cv::KeyPoint rows
        self.desc = torch.empty((self.cap, 64), dtype=torch.uint8, device=self.dev)
        self.matches = torch.empty((self.cap, 4), dtype=torch.int32, device=self.dev)     # 16-byte cv::DMatch rows
        self.p1 = torch.empty((self.cap, 2), dtype=torch.float32, device=self.dev)
        self.p2 = torch.empty((self.cap, 2), dtype=torch.float32, device=self.dev)
        self.mask = torch.empty(self.cap, dtype=torch.uint8, device=self.dev)

    def step(self, frame, filter_strength=0.8, reproj_thr=3.0, max_iters=2000, confidence=0.995, pose=None, matcher="ratio"):
        """frame: [H, W, C] u8 device tensor. Returns dict(n_keypoints, n_matches, H (3x3 numpy) or None, n_inliers), and with a PoseStage
        `pose` also "pose": the frame's matches downloaded, the pairs built on the host and solved by apds_pnp_solver_ransac (the
        established path the streamed pose stage is compared against). matcher "crosscheck": get_bruteforce_matches instead of the ratio
        matcher (one GPU; filter_strength is then unused)."""
        code = _matcher_code(matcher)
        if (code == _lib.PIPELINE_MATCH_L2_RATIO) != self.float_rows:
            raise _lib.ApdsError(_lib.ERR_BAD_ARG, 'matcher "l2" goes with float32 DB rows, and only with them')
        if code == _lib.PIPELINE_MATCH_CROSSCHECK and self.matcher.handle is not None:
            raise _lib.ApdsError(_lib.ERR_NOT_IMPLEMENTED, "the cross-check over a row-sharded train set is not built")
        with torch.cuda.stream(self.stream):
            out = self._step(frame, filter_strength, reproj_thr, max_iters, confidence, code)
            if pose is not None:
                M = out["n_matches"]
                m = self.matches[:M].cpu().numpy()
                kp = self.kps[:out["n_keypoints"]].cpu().numpy()
                out["pose"] = pose.solve(kp[m[:, 0], 0:2], m[:, 1])
            return out

    def _step(self, frame, filter_strength, reproj_thr, max_iters, confidence, matcher=_lib.PIPELINE_MATCH_RATIO):
        L = lib()
        h, w = frame.shape[0], frame.shape[1]
        ch = 1 if frame.dim() == 2 else frame.shape[2]
        n = C.c_int(0)
        if matcher == _lib.PIPELINE_MATCH_L2_RATIO:
            # the serial composition of the float pipeline: float extraction -> exact L2 top-2 -> L2 ratio filter
            if self.desc_f32 is None:
                self.desc_f32 = torch.empty((self.cap, 64), dtype=torch.float32, device=self.dev)
            check(L.apds_dev_akaze_extract_float(frame.data_ptr(), h, w, ch, frame.stride(0), None, 0, 0, self.cap, self.kps.data_ptr(), self.desc_f32.data_ptr(),
                                                 self.cap, C.byref(n), torch_stream()))
        else:
            check(L.apds_dev_akaze_extract(frame.data_ptr(), h, w, ch, frame.stride(0), self.cap, self.kps.data_ptr(), self.desc.data_ptr(), self.cap,
                                           C.byref(n), torch_stream()))
        K = n.value
        out = dict(n_keypoints=K, n_matches=0, H=None, n_inliers=0)
        if matcher == _lib.PIPELINE_MATCH_L2_RATIO:
            if K == 0:
                return out
            rows = self.matcher.rows
            keys = torch.empty((K, 2), dtype=torch.int64, device=self.dev)
            check(L.apds_dev_l2_topk(self.desc_f32.data_ptr(), K, rows.data_ptr(), int(rows.shape[0]), 64, self.matcher.index_base, 2, keys.data_ptr(), torch_stream()))
            M = int(dev_l2_ratio_filter(keys, filter_strength, out=self.matches).shape[0])
        elif matcher == _lib.PIPELINE_MATCH_CROSSCHECK:
            if K == 0:
                return out
            M = int(dev_crosscheck_match(self.desc[:K], self.matcher.rows, self.matcher.index_base, out=self.matches).shape[0])
        else:
            keys = self.matcher.knn(self.desc[:K], 2)
            if K == 0:
                return out
            nm = C.c_int(0)
            check(L.apds_dev_ratio_filter(keys.data_ptr(), K, 2, float(filter_strength), self.matches.data_ptr(), C.byref(nm), torch_stream()))
            M = nm.value
        out["n_matches"] = M
        if M < 4:
            return out
        # query_idx -> this frame's keypoints, train_idx -> DB row coordinates (28-byte rows with x,y first are not needed:
        # the DB side keeps only xy, so the gather is done on packed float2 rows)
        check(L.apds_dev_points_from_matches(self.kps.data_ptr(), K, self._db_kp_view().data_ptr(), self.db_xy_all.shape[0], self.matches.data_ptr(), M, 0,
                                             self.p1.data_ptr(), self.p2.data_ptr(), torch_stream()))
        H = np.zeros(9, np.float64)
        rc = L.apds_dev_find_homography(self.p1.data_ptr(), self.p2.data_ptr(), M, 8, float(reproj_thr), int(max_iters), float(confidence),
                                        _lib.ptr(H), self.mask.data_ptr(), torch_stream())
        if rc == 0:
            out["H"] = H.reshape(3, 3)
            out["n_inliers"] = int(self.mask[:M].sum().item())
        elif rc != _lib.ERR_EMPTY:
            check(rc)
        return out

    def _db_kp_view(self):
        if not hasattr(self, "_db_kp"):
            kp = torch.zeros((self.db_xy_all.shape[0], 7), dtype=torch.float32, device=self.dev)
            kp[:, 0:2] = self.db_xy_all
            self._db_kp = kp
        return self._db_kp


class StreamedFramePipeline:
    """The same path as FramePipeline, software-pipelined over a stream of frames - a FRONT of the library's own pipeline
    (apds_pipeline_create / _submit / _poll / _stats / _destroy, csrc/pipeline.cpp): the stage threads (two extraction workers, the match
    worker with its three streams, the homography worker), their HIP streams, events, slots and the starvation watch live inside
    libapds_hip.so, so a Rust or C++ host gets the same frames/s from four calls. What this class adds: the torch tensors behind the
    pointers (train rows, their keypoints, frames), the transport choice for a sharded DB (ShardedMatcher), and results as dicts."""

    def __init__(self, db_rows64, db_xy, index_base=0, group=None, max_points=(1 << 18) - 1, device="cuda:0", slots=6, reserve_cus=0,
                 n_cus=256, meta_group=None, extract_workers=None, transport="rccl", pose=None, db_kp=None, per_frame_table=None, view_capacity=None,
                 matcher="ratio", lens=None):
        import os
        # lens = (K, dist_coeffs, iters): apds_pipeline_set_lens - the image side of every frame's matches is undistorted on the device in
        # front of the homography and the pose (K is expected to be the pose stage's camera matrix); None: no lens
        self.lens = None if lens is None else (_lib.lens_args(lens[0], lens[1]), int(lens[2]) if len(lens) > 2 else 5)
        self.matcher_mode = _matcher_code(matcher)   # "ratio" | "crosscheck" (apds_pipeline_set_matcher; one GPU and per-frame-view pipelines)
        # "l2": the float pipeline (apds_pipeline_create_float) - db_rows64 is then [N, 64] float32; one GPU, a fixed train set
        # (or a per-frame view of a float KeypointTable: from_table chooses it)
        self.float_rows = self.matcher_mode == _lib.PIPELINE_MATCH_L2_RATIO
        float_table = per_frame_table is not None and getattr(per_frame_table, "is_float", False)
        if float_table != self.float_rows and per_frame_table is not None:
            raise ValueError('a float table\'s pipeline runs matcher "l2", a byte table\'s "ratio" or "crosscheck"')
        if self.float_rows and not float_table and (group is not None or db_rows64 is None or db_rows64.dtype != torch.float32
                                                    or db_rows64.dim() != 2 or db_rows64.shape[1] != 64 or not db_rows64.is_contiguous()):
            raise ValueError('matcher "l2": a contiguous [N, 64] float32 device tensor of train rows (or a float table\'s per-frame view), one GPU')
        self.dev = torch.device(device)
        self.per_frame_table = per_frame_table     # a KeypointTable: the train set is selected from it per frame (from_table)
        self.view_capacity = int(view_capacity) if view_capacity else 0
        self.matcher = None if per_frame_table is not None else ShardedMatcher(db_rows64, index_base, group, meta_group=meta_group, transport=transport)
        if per_frame_table is not None:
            self.n_db, kp = 0, None
        elif db_kp is not None:
            self.n_db = db_kp.shape[0]     # the 28-byte rows themselves, already on the device (from_table)
            kp = db_kp
        else:
            self.n_db = db_xy.shape[0]
            kp = torch.zeros((self.n_db, 7), dtype=torch.float32, device=self.dev)     # 28-byte cv::KeyPoint rows of ALL train rows (x, y used)
            kp[:, 0:2] = db_xy
        self.db_kp = kp
        self.cap = max_points
        self.n_slots = slots
        self.extract_workers = int(extract_workers if extract_workers is not None else os.environ.get("APDS_EXTRACT_WORKERS", "0") or 0)
        self.debug_extract_delay = float(os.environ.get("APDS_DEBUG_EXTRACT_DELAY_MS", "0")) * 1e-3    # test hook (seconds)
        self.cap_bytes = 0              # occupancy cap this pipeline's scans run with (set by the starvation watch; kept across re-creations)
        self.cap_events = []
        self.gap_log = []               # idle time of the match stream before each frame's main scan (ms; the first 16 of a run)
        self.gap_mean = None
        self._masked_stream_handle = None
        self._pipe, self._key = None, None
        self.pose = pose                # PoseStage or None: every result then carries "pose"
        if reserve_cus > 0:
            # keep `reserve_cus` CUs (spread evenly over the CU index space) out of the MATCH stream only
            words = (n_cus + 31) // 32
            mask = np.full(words, 0xFFFFFFFF, np.uint32)
            stride = n_cus // reserve_cus
            for cu in (r * stride for r in range(reserve_cus)):
                mask[cu // 32] &= ~np.uint32(1 << (cu % 32))
            h = C.c_void_p()
            check(lib().apds_stream_create(0, _lib.ptr(mask), words, C.byref(h)))
            self._masked_stream_handle = h
        torch.cuda.synchronize()

    @classmethod
    def from_table(cls, table, device="cuda:0", per_frame_view=False, view_capacity=None, **kw):
        """A pipeline whose database IS a KeypointTable (feature_database.py): the train rows and their keypoints are the table's own device
        columns (table.device_table()), nothing is downloaded or re-uploaded, and a match's train index is the table row (= id - 1). The
        pipeline keeps the table alive; nothing may be inserted into it while the pipeline lives. pose=PoseStage.from_table(table, ..) adds
        the pose stage on the table's world points.
        per_frame_view=True: every frame is matched against the rows ITS selection returns (keypointdb.rs:50-90, at most view_capacity
        rows, default 262143) instead of the whole table: run(frames, count, selections=[...]) / submit_select(). One GPU."""
        if getattr(table, "is_float", False):     # a float table: the L2 matcher on each frame's view (apds_db_view_l2_train), the only one it has
            if not per_frame_view:
                raise ValueError("a float table's pipeline selects its train set per frame: per_frame_view=True")
            kw.setdefault("matcher", "l2")
        if per_frame_view:
            self = cls(None, None, device=device, per_frame_table=table, view_capacity=view_capacity, **kw)
            self._table = table
            return self
        rows64, kps, _, n = table.device_table()
        if n <= 0:
            raise ValueError("the table is empty")
        self = cls(_table_tensor(rows64, n * 64, device, torch.uint8, (n, 64)), None, device=device,
                   db_kp=_table_tensor(kps, n * 28, device, torch.float32, (n, 7)), **kw)
        self._table = table
        return self

    # ---- the native handle ------------------------------------------------------------------------------------------------------------
    def _ensure(self, shape, filter_strength, reproj_thr, max_iters, confidence, timing):
        rows, cols = int(shape[0]), int(shape[1])
        ch = 1 if len(shape) == 2 else int(shape[2])
        key = (rows, cols, ch, float(filter_strength), float(reproj_thr), int(max_iters), float(confidence), bool(timing), float(self.debug_extract_delay),
               int(self.cap_bytes))
        if self._pipe is not None and key == self._key:
            return
        self._destroy_native()
        p = _lib.PipelineParams(rows=rows, cols=cols, channels=ch, max_points=int(self.cap), n_slots=int(self.n_slots), extract_workers=int(self.extract_workers),
                                filter_strength=float(filter_strength), homography_method=8, reproj_threshold=float(reproj_thr), max_iters=int(max_iters),
                                confidence=float(confidence), timing=1 if timing else 0, match_lds_cap=int(self.cap_bytes),
                                match_stream=self._masked_stream_handle, debug_extract_delay_ms=float(self.debug_extract_delay) * 1e3)
        h = C.c_void_p()
        m = self.matcher
        check(lib().apds_set_device(self.dev.index or 0))
        if self.per_frame_table is not None:
            check(lib().apds_pipeline_create_table(C.byref(h), self.per_frame_table._h, self.view_capacity, C.byref(p)))
        elif self.float_rows:
            check(lib().apds_pipeline_create_float(C.byref(h), m.rows.data_ptr(), int(m.rows.shape[0]), m.index_base, self.db_kp.data_ptr(), self.n_db, C.byref(p)))
        else:
            check(lib().apds_pipeline_create(C.byref(h), m.rows.data_ptr(), int(m.rows.shape[0]), m.index_base, m.handle, self.db_kp.data_ptr(), self.n_db, C.byref(p)))
        self._pipe, self._key = h, key

        def configured(rc):     # a setter that failed: its error text first, then no handle is left behind
            if rc != 0:
                why = lib().apds_last_error().decode("utf-8", "replace")
                self._pipe = None
                lib().apds_pipeline_destroy(h)
                raise _lib.ApdsError(rc, why)

        if self.matcher_mode not in (_lib.PIPELINE_MATCH_RATIO, _lib.PIPELINE_MATCH_L2_RATIO):     # (a pipeline that never asks runs the ratio matcher)
            configured(lib().apds_pipeline_set_matcher(h, self.matcher_mode))
        if self.lens is not None:
            (K, d, pK, pd, nd), iters = self.lens
            configured(lib().apds_pipeline_set_lens(h, pK, pd, nd, iters))
        if self.pose is not None:
            pp = self.pose.params()
            if self.per_frame_table is not None:
                pp.db_xyz_dev = None     # the views gather the table's own world points
            check(lib().apds_pipeline_enable_pose(h, C.byref(pp)))

    def enable_pose(self, pose):
        """Turn the pose stage on (PoseStage) or off (None) for the frames that follow: the native pipeline is made again."""
        self.pose = pose
        self._destroy_native()

    def _destroy_native(self):
        h, self._pipe = self._pipe, None
        if h is not None:
            check(lib().apds_pipeline_destroy(h))

    def close(self):
        """Destroy the native pipeline and the CU-masked match stream (if any)."""
        self._destroy_native()
        h, self._masked_stream_handle = self._masked_stream_handle, None
        if h is not None:
            lib().apds_stream_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001
            pass

    # ---- submit / poll (what bench.py's timed loop calls, through the bound C functions directly) -----------------------------------------
    def prepare(self, frame_shape, filter_strength=0.8, reproj_thr=3.0, max_iters=2000, confidence=0.995, timing=False):
        """Create (or keep) the native pipeline for frames of this shape and these parameters; returns its handle (void*)."""
        self._ensure(frame_shape, filter_strength, reproj_thr, max_iters, confidence, timing)
        return self._pipe

    @staticmethod
    def frame_args(f):
        """(pointer, row stride in bytes, on_device) of a [H, W(, C)] u8 tensor: a device tensor, or a host tensor (pinned: overlapped upload)."""
        return C.c_void_p(f.data_ptr()), int(f.stride(0)), 1 if f.is_cuda else 0

    @staticmethod
    def result_dict(r, pose=None):
        out = dict(n_keypoints=r.n_keypoints, n_matches=r.n_matches, n_inliers=r.n_inliers, status=r.status,
                   H=np.array(r.H, np.float64).reshape(3, 3) if r.homography_found else None)
        if pose is not None:
            out["pose"] = pose_dict_of(pose.status, pose.found, pose.n_correspondences, pose.n_inliers, list(pose.rvec), list(pose.tvec))
        return out

    def stats(self, reset=False):
        st = _lib.PipelineCounters()
        check(lib().apds_pipeline_stats(self._pipe, C.byref(st), 1 if reset else 0))
        return st

    @staticmethod
    def selection(mode, value, box=(0, 0, 0, 0)):
        """apds_db_selection: mode 0 image id, 1 level of detail, 2 level of detail + bounding box (x_start, y_start, x_end, y_end)"""
        return _lib.DbSelection(mode=int(mode), value=int(value), x_start=float(box[0]), y_start=float(box[1]), x_end=float(box[2]), y_end=float(box[3]))

    def submit_select(self, frame, sel):
        """Hand one frame and its train-set selection (selection(..)) to a per-frame-view pipeline (prepare() first); returns the frame number.
        The frame must stay alive until its result is polled."""
        ptr, stride, on_dev = self.frame_args(frame)
        fid = C.c_int64(0)
        check(lib().apds_pipeline_submit_select(self._pipe, ptr, stride, on_dev, C.byref(sel), C.byref(fid)))
        return fid.value

    def poll(self, wait=True):
        """The next result in submission order as a dict (None: wait=False and it is not finished, or nothing is in flight). A frame that
        failed is reported through its "status", not raised."""
        res = _lib.FrameResult()
        fp = _lib.FramePose() if self.pose is not None else None
        rc = lib().apds_pipeline_poll_pose(self._pipe, C.byref(res), C.byref(fp) if fp is not None else None, 1 if wait else 0)
        if rc < 0:
            check(rc)
        return self.result_dict(res, fp) if rc == 0 else None

    def run(self, frames, count, filter_strength=0.8, reproj_thr=3.0, max_iters=2000, confidence=0.995, timing=False, selections=None):
        """Push `count` frames (cycled from `frames`) through the pipeline. Returns (results in frame order, timers). selections (a
        per-frame-view pipeline): the frames' train-set selections, cycled like the frames."""
        L = lib()
        if (selections is not None) != (self.per_frame_table is not None):
            raise ValueError("selections go with a pipeline made by from_table(per_frame_view=True), and only with it")
        self._ensure(frames[0].shape, filter_strength, reproj_thr, max_iters, confidence, timing)
        if timing:
            self.stats(reset=True)
        args = [self.frame_args(f) for f in frames]
        res = _lib.FrameResult()
        fp = _lib.FramePose() if self.pose is not None else None
        fpp = C.byref(fp) if fp is not None else None
        results = []
        for i in range(count):
            ptr, stride, on_dev = args[i % len(args)]
            if selections is not None:
                check(L.apds_pipeline_submit_select(self._pipe, ptr, stride, on_dev, C.byref(selections[i % len(selections)]), None))
            else:
                check(L.apds_pipeline_submit(self._pipe, ptr, stride, on_dev, None))
            while True:       # take what is finished, so the result queue stays short on long runs
                rc = L.apds_pipeline_poll_pose(self._pipe, C.byref(res), fpp, 0)
                if rc != 0:
                    if rc < 0:
                        check(rc)
                    break
                results.append(self.result_dict(res, fp))
        while len(results) < count:
            check(L.apds_pipeline_poll_pose(self._pipe, C.byref(res), fpp, 1))
            results.append(self.result_dict(res, fp))
        for i, r in enumerate(results):
            if r["status"] != 0:
                raise _lib.ApdsError(r["status"], f"frame {i} failed in the pipeline")
        st = self.stats(reset=timing)
        timers = {}
        if timing:
            timers = {"hamming_topk": (st.hamming_topk_ms, st.hamming_topk_launches), "hamming_topk_sample": (st.hamming_topk_sample_ms, st.hamming_topk_sample_launches),
                      "akaze_extract": (st.akaze_extract_ms, st.akaze_extract_calls), "ransac_score": (st.ransac_score_ms, st.ransac_score_launches)}
        self.gap_log = [float(st.match_gaps_first_ms[i]) for i in range(min(16, st.match_gaps))]
        self.gap_mean = float(st.match_gap_mean_ms) if st.match_gaps else None
        if st.match_lds_cap_set_at_frame >= 0 and not self.cap_events:
            self.cap_events.append(dict(frame=int(st.match_lds_cap_set_at_frame), gaps_ms=[round(float(g), 2) for g in st.match_lds_cap_gaps_ms], previous=0))
            self.cap_bytes = int(st.match_lds_cap_bytes)
            self._key = self._key[:-1] + (int(self.cap_bytes),)     # the live native pipeline IS capped: no re-creation for that
        return results, timers
