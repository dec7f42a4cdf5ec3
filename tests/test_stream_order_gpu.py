"""GPU: WHEN the device entries run relative to the caller's stream (include/apds.h "device-resident API": asynchronous on `stream`), which
no value test sees - those hand over inputs that have been ready for a long time and synchronise right after.

Every call here goes to an explicit torch stream whose handle the ABI gets. In front of the real input the stream holds a DELAY
(torch.cuda._sleep, calibrated once to ~20 ms, at most 200 ms), and every ordering test asserts that the event behind the delay had not
completed when the host made the call - otherwise it proved nothing. Inputs: stream_order_cases.py (real and decoy sets, checked by
test_stream_order_inputs_cpu.py). References: the oracle / numpy where the entry is pinned to them bit for bit, else the same entry run
fully synchronised beforehand. All comparisons are exact.

 * late:        the buffers hold the decoy; on S: delay, real input copied in, the entry, the outputs cloned. Work done off S sees the decoy.
 * overwritten: the buffers hold the real input; on S: delay, the entry, the decoy copied over the input, the outputs cloned. A branch
                that was not joined back into S before the entry returned reads the decoy.
 * two streams: one thread, a long matcher call on A and four short ones on fresh streams that start with it: the thread's workspace
                (ThreadCtx, csrc/common.h) must not be handed to the second call while the first still uses it.
 * NULL:        the thread's own stream, then apds_dev_download(NULL)."""
import ctypes as C

import numpy as np
import pytest

import filter_border_cases as bc
import stream_order_cases as sc

pytestmark = pytest.mark.gpu

DELAY_MS, DELAY_CAP_MS = 20.0, 200.0


@pytest.fixture(scope="module")
def env(gpu_pkg):
    import torch
    return torch, torch.device("cuda:0"), gpu_pkg._lib.lib(), gpu_pkg._lib.check


@pytest.fixture(scope="module")
def delay_cycles(env):
    """cycles of torch.cuda._sleep for ~DELAY_MS, measured with events once per module"""
    torch = env[0]
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 2_000_000
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    per_ms = probe / max(a.elapsed_time(b), 1e-3)
    cycles = int(per_ms * DELAY_MS)
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    print(f"delay: {cycles} cycles = {ms:.1f} ms")
    assert DELAY_MS / 4 < ms < DELAY_CAP_MS
    return cycles


def _bytes(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()


def _sp(stream):
    return C.c_void_p(stream.cuda_stream)


class Entry:
    """One device entry at one shape. real / decoy: tuples of numpy arrays (the device inputs); run(ins, stream pointer) -> the tensors the
    entry wrote (only the part it defines), called under the torch stream whose handle it gets; blocking: the entry synchronises the stream
    (it returns a count or a model to the host); want: per output a numpy array (byte-compared with the synchronised run) or None (no
    independent reference: the synchronised run alone); prime: called, synchronised, in front of every ordered run (the view select: it
    leaves the decoy selection in the view's buffers)."""

    def __init__(self, name, real, decoy, run, blocking=False, want=None, prime=None):
        self.name, self.real, self.decoy, self.run, self.blocking, self.want, self.prime = name, real, decoy, run, blocking, want, prime


def _entries(gpu_pkg, oracle_mod, env, later):
    """later: callables that release what the entries keep for the module's life (scan states, the table and its view)"""
    torch, d, L, check = env
    synth, ptr = gpu_pkg.synth, gpu_pkg._lib.ptr
    E = []
    empty = lambda shape, dt: torch.empty(shape, dtype=dt, device=d)   # noqa: E731
    knn_keys = lambda q, t, k: bc.keys_from_knn(*oracle_mod.knn_hamming(q, t, k))   # noqa: E731

    (src, dec) = sc.pack_inputs()

    def run_pack(ins, sp):
        out = empty((sc.PACK_N, 64), torch.uint8)
        check(L.apds_dev_pack_descriptors(ins[0].data_ptr(), sc.PACK_N, sc.PACK_BYTES, sc.PACK_STRIDE, out.data_ptr(), sp))
        return [out]
    E.append(Entry("pack_descriptors", (src,), (dec,), run_pack, want=(sc.pack_reference(src),)))

    for nt in sc.TOPK_NT:
        (q, t), (dq, dt) = sc.topk_inputs(synth, nt)
        real, decoy = (sc.pad64(q), sc.pad64(t)), (sc.pad64(dq), sc.pad64(dt))
        for k in sc.TOPK_K:
            want = (knn_keys(q, t, k),)

            def run_topk(ins, sp, nt=nt, k=k, backend=None):
                out = empty((sc.TOPK_NQ, k), torch.int64)
                if backend is None:
                    check(L.apds_dev_hamming_topk(ins[0].data_ptr(), sc.TOPK_NQ, ins[1].data_ptr(), nt, 0, k, out.data_ptr(), sp))
                else:
                    check(L.apds_dev_hamming_topk_backend(ins[0].data_ptr(), sc.TOPK_NQ, ins[1].data_ptr(), nt, 0, k, out.data_ptr(), backend, sp))
                return [out]
            E.append(Entry(f"hamming_topk-nt{nt}-k{k}", real, decoy, run_topk, want=want))
            for backend in (sc.BACKEND_VECTOR, sc.mfma_backend(k)):
                E.append(Entry(f"hamming_topk_backend{backend}-nt{nt}-k{k}", real, decoy,
                               lambda ins, sp, f=run_topk, b=backend: f(ins, sp, backend=b), want=want))
        if nt == sc.TOPK_NT[0]:
            for k in (1, 2):
                # one state for the module's life: creating, growing and destroying a state synchronise the device, which would sit out the
                # delay; the synchronised runs in front of every ordered one have grown it, so the three steps return with everything queued
                st = C.c_void_p()
                check(L.apds_dev_topk_state_create(C.byref(st)))
                later.append(lambda st=st: check(L.apds_dev_topk_state_destroy(st)))

                def run_split(ins, sp, nt=nt, k=k, st=st):
                    out = empty((sc.TOPK_NQ, k), torch.int64)
                    check(L.apds_dev_topk_prepass(st, ins[0].data_ptr(), sc.TOPK_NQ, ins[1].data_ptr(), nt, 0, k, sp))
                    check(L.apds_dev_topk_scan(st, ins[0].data_ptr(), ins[1].data_ptr(), sp))
                    check(L.apds_dev_topk_merge(st, 0, out.data_ptr(), sp))
                    return [out]
                E.append(Entry(f"topk_prepass_scan_merge-k{k}", real, decoy, run_split, want=(knn_keys(q, t, k),)))

    mk, mdec = sc.merge_inputs()

    def run_merge(ins, sp):
        out = empty((sc.MERGE_NQ, sc.MERGE_K), torch.int64)
        check(L.apds_dev_merge_topk(ins[0].data_ptr(), sc.MERGE_PARTS, sc.MERGE_NQ, sc.MERGE_K, out.data_ptr(), sp))
        return [out]
    E.append(Entry("merge_topk", (mk,), (mdec,), run_merge, want=(sc.merge_reference(mk),)))

    (fq, ft), (fdq, fdt) = sc.filter_descriptors(synth)
    k2, dk2 = knn_keys(fq, ft, 2), knn_keys(fdq, fdt, 2)
    tb, dtb = knn_keys(ft, fq, 1).ravel(), knn_keys(fdt, fdq, 1).ravel()

    def run_ratio(ins, sp):
        out, n = empty((sc.FILTER_NQ, 4), torch.int32), C.c_int(-1)
        check(L.apds_dev_ratio_filter(ins[0].data_ptr(), sc.FILTER_NQ, 2, float(sc.FILTER_FS), out.data_ptr(), C.byref(n), sp))
        return [out[: n.value]]
    E.append(Entry("ratio_filter", (k2,), (dk2,), run_ratio, blocking=True, want=(bc.ratio_reference(k2, 2, sc.FILTER_FS),)))

    def run_cross(ins, sp):
        out, n = empty((sc.FILTER_NQ, 4), torch.int32), C.c_int(-1)
        check(L.apds_dev_cross_check(ins[0].data_ptr(), sc.FILTER_NT, sc.FILTER_NQ, out.data_ptr(), C.byref(n), sp))
        return [out[: n.value]]
    E.append(Entry("cross_check", (tb,), (dtb,), run_cross, blocking=True, want=(bc.cross_check_reference(tb, sc.FILTER_NQ),)))

    def run_ccmatch(ins, sp):
        out, n = empty((sc.FILTER_NQ, 4), torch.int32), C.c_int(-1)
        check(L.apds_dev_crosscheck_match(ins[0].data_ptr(), sc.FILTER_NQ, ins[1].data_ptr(), sc.FILTER_NT, 0, out.data_ptr(), C.byref(n), sp))
        return [out[: n.value]]
    E.append(Entry("crosscheck_match", (sc.pad64(fq), sc.pad64(ft)), (sc.pad64(fdq), sc.pad64(fdt)), run_ccmatch, blocking=True,
                   want=(oracle_mod.get_bruteforce_matches(fq, ft),)))

    for dim in sc.L2_DIMS:
        lr, ld = sc.l2_inputs(dim)

        def run_l2(ins, sp, dim=dim):
            out = empty((sc.L2_NQ, 2), torch.int64)
            check(L.apds_dev_l2_topk(ins[0].data_ptr(), sc.L2_NQ, ins[1].data_ptr(), sc.L2_NT, dim, 0, 2, out.data_ptr(), sp))
            return [out]
        E.append(Entry(f"l2_topk-dim{dim}", lr, ld, run_l2))

    br, bd = sc.band_inputs()
    for bgra in (0, 1):
        def run_band(ins, sp, bgra=bgra):
            out = empty((sc.BAND_N, 4), torch.uint8)
            check(L.apds_dev_band_merger(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), sc.BAND_N, ptr(sc.BAND_MINMAX), bgra, out.data_ptr(), sp))
            return [out]
        rgba = np.asarray(oracle_mod.band_merger(*br, sc.BAND_MINMAX)).reshape(-1, 4)
        E.append(Entry(f"band_merger-bgra{bgra}", br, bd, run_band, want=(np.ascontiguousarray(rgba[:, [2, 1, 0, 3]]) if bgra else rgba,)))

    sr, sd = sc.sat_inputs()

    def run_sat(ins, sp):
        out = empty((sc.SAT_ROWS + 1, sc.SAT_COLS + 1), torch.int32)
        check(L.apds_dev_mask_zero_sat(ins[0].data_ptr(), sc.SAT_ROWS, sc.SAT_COLS, sc.SAT_COLS, 1, out.data_ptr(), sp))
        return [out]
    E.append(Entry("mask_zero_sat", (sr,), (sd,), run_sat, want=(sc.sat_reference(sr),)))

    pr, pd = sc.point_inputs()

    def run_points(ins, sp):
        p1, p2 = empty((sc.POINTS_NM, 2), torch.float32), empty((sc.POINTS_NM, 2), torch.float32)
        check(L.apds_dev_points_from_matches(ins[0].data_ptr(), sc.POINTS_N1, ins[1].data_ptr(), sc.POINTS_N2, ins[2].data_ptr(), sc.POINTS_NM, 0,
                                             p1.data_ptr(), p2.data_ptr(), sp))
        return [p1, p2]
    E.append(Entry("points_from_matches", pr[:3], pd[:3], run_points, blocking=True, want=sc.points_reference(*pr[:3])))

    def run_corr(ins, sp):
        img, obj = empty((sc.POINTS_NM, 2), torch.float32), empty((sc.POINTS_NM, 3), torch.float32)
        check(L.apds_dev_pnp_correspondences(ins[0].data_ptr(), sc.POINTS_N1, ins[1].data_ptr(), sc.POINTS_N2, ptr(sc.PNP_ORIGIN), ins[2].data_ptr(),
                                             sc.POINTS_NM, img.data_ptr(), obj.data_ptr(), sp))
        return [img, obj]
    E.append(Entry("pnp_correspondences", (pr[0], pr[3], pr[2]), (pd[0], pd[3], pd[2]), run_corr, blocking=True,
                   want=sc.correspondences_reference(pr[0], pr[3], pr[2])))

    hr, hd = sc.homography_inputs(synth)
    for method in sc.HOMOGRAPHY_METHODS:
        def run_h(ins, sp, method=method):
            H, mask = np.zeros(9, np.float64), empty((sc.HOMOGRAPHY_N,), torch.uint8)
            check(L.apds_dev_find_homography(ins[0].data_ptr(), ins[1].data_ptr(), sc.HOMOGRAPHY_N, method, 3.0, 2000, 0.995, ptr(H), mask.data_ptr(), sp))
            return [torch.from_numpy(H.view(np.uint8).copy()).to(d, non_blocking=False), mask]
        # (the model is pinned to the oracle within a tolerance elsewhere, so it has no exact reference here; RANSAC's inlier mask has)
        omask = np.asarray(oracle_mod.find_homography(*hr, method, 3.0)[2], np.uint8).ravel() if method else None
        E.append(Entry(f"find_homography-method{method}", hr, hd, run_h, blocking=True, want=(None, omask)))

    ar, ad = sc.akaze_single_inputs(synth)
    rows, cols, ch = sc.AKAZE_SINGLE
    cap = sc.AKAZE_CAP

    def run_akaze(ins, sp):
        kps, desc, n = empty((cap, 7), torch.float32), empty((cap, 64), torch.uint8), C.c_int(-1)
        check(L.apds_dev_akaze_extract(ins[0].data_ptr(), rows, cols, ch, cols * ch, cap, kps.data_ptr(), desc.data_ptr(), cap, C.byref(n), sp))
        return [kps[: n.value], desc[: n.value, :61]]
    ref = oracle_mod.akaze(ar)
    E.append(Entry("akaze_extract", (ar,), (ad,), run_akaze, blocking=True, want=(ref.keypoints.copy(), ref.descriptors.copy())))

    abr, abd = sc.akaze_batch_inputs(synth)
    B, brows, bcols, bch = sc.AKAZE_BATCH

    def run_akaze_batch(ins, sp):
        kps, desc, counts = empty((B, cap, 7), torch.float32), empty((B, cap, 64), torch.uint8), (C.c_int * B)()
        check(L.apds_dev_akaze_extract_batch(ins[0].data_ptr(), B, brows * bcols * bch, brows, bcols, bch, bcols * bch, cap, kps.data_ptr(), desc.data_ptr(),
                                             cap, counts, sp))
        out = [torch.tensor(list(counts), dtype=torch.int32)]
        for i in range(B):
            out += [kps[i, : counts[i]], desc[i, : counts[i], :61]]
        return out
    refs = [oracle_mod.akaze(abr[i]) for i in range(B)]
    want = [np.array([len(r.keypoints) for r in refs], np.int32)]
    for r in refs:
        want += [r.keypoints.copy(), r.descriptors.copy()]
    E.append(Entry("akaze_extract_batch", (abr,), (abd,), run_akaze_batch, blocking=True, want=tuple(want)))

    # ---- the keypoint table: the device inserts into a fresh table, read back through apds_db_table; a view's select
    def download(ptr_dev, nbytes, sp):
        host = np.empty(max(nbytes, 1), np.uint8)
        check(L.apds_dev_download(host.ctypes.data, ptr_dev, nbytes, sp))    # on the caller's stream, which it synchronises
        return torch.from_numpy(host[:nbytes])

    def table_columns(db, sp):
        rows64, tk, n = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        check(L.apds_db_table(db, C.byref(rows64), C.byref(tk), None, C.byref(n)))
        return [torch.tensor([n.value], dtype=torch.int64), download(tk, n.value * 28, sp), download(rows64, n.value * 64, sp)]

    def fresh_table(insert):
        db = C.c_void_p()
        check(L.apds_db_create(C.byref(db), sc.INSERT_TABLE_ROWS))
        try:
            insert(db)
            return table_columns(db, insert.sp)
        finally:
            check(L.apds_db_destroy(db))

    ir, idec = sc.insert_inputs()

    def run_insert(ins, sp):
        def insert(db):
            check(L.apds_db_insert_dev(db, ins[0].data_ptr(), ins[1].data_ptr(), sc.INSERT_N, *sc.INSERT_ARGS, sp))
        insert.sp = sp
        return fresh_table(insert)
    # (the lifted keypoints are pinned elsewhere: here the synchronised run; the descriptor column is the rows as they came)
    E.append(Entry("db_insert_dev", ir, idec, run_insert, blocking=True, want=(np.array([sc.INSERT_N], np.int64), None, ir[1])))

    ibr, ibd = sc.insert_batch_inputs()
    counts = (C.c_int32 * sc.INSERT_BATCH_TILES)(*sc.INSERT_BATCH_COUNTS)

    def run_insert_batch(ins, sp):
        def insert(db):
            image_id, lod, _, _, tw, th = sc.INSERT_ARGS
            check(L.apds_db_insert_batch_dev(db, ins[0].data_ptr(), ins[1].data_ptr(), sc.INSERT_BATCH_TILES, sc.INSERT_BATCH_CAP, counts, image_id, lod,
                                             ptr(sc.INSERT_BATCH_COLUMNS_ROWS), tw, th, sp))
        insert.sp = sp
        return fresh_table(insert)
    E.append(Entry("db_insert_batch_dev", ibr, ibd, run_insert_batch, blocking=True,
                   want=(np.array([sum(sc.INSERT_BATCH_COUNTS)], np.int64), None, sc.insert_batch_rows(ibr[1]))))

    db, view = C.c_void_p(), C.c_void_p()
    check(L.apds_db_create(C.byref(db), sc.VIEW_TABLE_ROWS))
    later.append(lambda: check(L.apds_db_destroy(db)))
    for image_id, lod, kp, d61 in sc.view_table():
        check(L.apds_db_insert_image(db, ptr(kp), ptr(d61), len(kp), image_id, lod, 0, 0, *sc.VIEW_TILE))
    check(L.apds_db_view_create(db, 0, C.byref(view)))
    later.append(lambda: check(L.apds_db_view_destroy(view)))     # (appended last, released first: the view borrows the table)

    def select(selection, sp):
        n = C.c_int(-1)
        check(L.apds_db_view_select(view, selection[0], selection[1], 0.0, 0.0, 0.0, 0.0, 0, sp, C.byref(n)))
        return n.value

    def run_view(ins, sp):
        n = select(sc.VIEW_REAL, sp)
        rows64, vk, ids, img, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(-1)
        check(L.apds_db_view_pointers(view, C.byref(rows64), C.byref(vk), C.byref(ids), C.byref(img), None, C.byref(cnt)))
        assert cnt.value == n
        return [download(ids, n * 4, sp), download(img, n * 4, sp), download(vk, n * 28, sp), download(rows64, n * 64, sp)]

    def prime_view():
        assert select(sc.VIEW_DECOY, None) == len(sc.view_reference(sc.VIEW_DECOY)[0])
        check(L.apds_stream_synchronize(None))
    vrows, vimg = sc.view_reference(sc.VIEW_REAL)
    E.append(Entry("db_view_select", (), (), run_view, blocking=True, want=(vrows, vimg, None, None), prime=prime_view))
    return E


@pytest.fixture(scope="module")
def entries(gpu_pkg, oracle_mod, env):
    """The entries, each with the result of a fully synchronised run on the real input (a warm-up too: module loads, workspace growth and
    LDS opt-ins happen here, not under a delay), compared with its oracle / numpy reference where it has one."""
    torch, d = env[0], env[1]
    later = []
    E = _entries(gpu_pkg, oracle_mod, env, later)
    S = torch.cuda.Stream(d)
    for e in E:
        ins = [torch.from_numpy(_bytes(a)).to(d) for a in e.real]
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            outs = e.run(ins, _sp(S))
        torch.cuda.synchronize()
        e.sync = [_bytes(o.cpu().numpy()) for o in outs]
        if e.want is not None:
            assert len(e.want) == len(e.sync), e.name
            for i, (w, g) in enumerate(zip(e.want, e.sync)):
                assert w is None or np.array_equal(_bytes(w), g), f"{e.name}: output {i} of the synchronised run differs from its reference"
    yield {e.name: e for e in E}
    torch.cuda.synchronize()
    for release in reversed(later):
        release()


def _names():
    n = ["pack_descriptors"]
    for nt in sc.TOPK_NT:
        for k in sc.TOPK_K:
            n += [f"hamming_topk-nt{nt}-k{k}", f"hamming_topk_backend{sc.BACKEND_VECTOR}-nt{nt}-k{k}", f"hamming_topk_backend{sc.mfma_backend(k)}-nt{nt}-k{k}"]
    n += ["topk_prepass_scan_merge-k1", "topk_prepass_scan_merge-k2", "merge_topk", "ratio_filter", "cross_check", "crosscheck_match"]
    n += [f"l2_topk-dim{dim}" for dim in sc.L2_DIMS] + ["band_merger-bgra0", "band_merger-bgra1", "mask_zero_sat", "points_from_matches", "pnp_correspondences"]
    n += [f"find_homography-method{m}" for m in sc.HOMOGRAPHY_METHODS] + ["akaze_extract", "akaze_extract_batch"]
    n += ["db_insert_dev", "db_insert_batch_dev", "db_view_select"]
    return n


NAMES = _names()


def test_every_entry_has_a_case(entries):
    assert sorted(entries) == sorted(NAMES)


def _ordered_run(env, cycles, e, first, then):
    """On a fresh stream: delay, `first` copied into the input buffers (None: they hold it already), the entry, `then` copied over the
    inputs (None: nothing), the outputs cloned. -> (output bytes, delay pending at the call, delay pending after the enqueue)"""
    torch, d = env[0], env[1]
    S = torch.cuda.Stream(d)
    bufs = [torch.from_numpy(_bytes(a)).to(d) for a in (e.decoy if first is not None else e.real)]
    first = [torch.from_numpy(_bytes(a)).to(d) for a in first] if first is not None else None
    then = [torch.from_numpy(_bytes(a)).to(d) for a in then] if then is not None else None
    torch.cuda.synchronize()
    # settle the thread's workspace for this shape: a call that outgrows it opens a second slab, and the NEXT call replaces both by one with
    # a device-wide synchronisation (ThreadCtx::ws_reset) - which would sit out the delay. Two synchronised calls leave one slab that fits.
    warm = first if first is not None else bufs
    for _ in range(2):
        with torch.cuda.stream(S):
            e.run(warm, _sp(S))
        torch.cuda.synchronize()
    if e.prime is not None:
        e.prime()
        torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        ev.record(S)
        if first is not None:
            for b, r in zip(bufs, first):
                b.copy_(r, non_blocking=True)
        pending_at_call = not ev.query()
        outs = e.run(bufs, _sp(S))
        if then is not None:
            for b, r in zip(bufs, then):
                b.copy_(r, non_blocking=True)
        outs = [o.clone() for o in outs]
        pending_after = not ev.query()
    S.synchronize()
    got = [_bytes(o.cpu().numpy()) for o in outs]
    torch.cuda.synchronize()
    return got, pending_at_call, pending_after


def _check(e, got, pending_at_call, pending_after):
    print(f"{e.name}: delay pending at the call {pending_at_call}, after the enqueue {pending_after}")
    assert pending_at_call, "the delay had run out before the call was made: the run shows nothing"
    assert e.blocking or pending_after, "the delay had run out before the outputs' clone was queued: the run shows nothing"
    assert len(got) == len(e.sync)
    for i, (g, w) in enumerate(zip(got, e.sync)):
        assert g.shape == w.shape and np.array_equal(g, w), f"{e.name}: output {i} differs from the synchronised run"


@pytest.mark.parametrize("name", NAMES)
def test_input_that_is_ready_late(env, delay_cycles, entries, name):
    e = entries[name]
    _check(e, *_ordered_run(env, delay_cycles, e, first=e.real, then=None))


@pytest.mark.parametrize("name", NAMES)
def test_input_overwritten_right_after_the_call(env, delay_cycles, entries, name):
    e = entries[name]
    _check(e, *_ordered_run(env, delay_cycles, e, first=None, then=e.decoy))


# ---- two streams, one thread ------------------------------------------------------------------------------------------------------------
# Only matcher calls: their scratch in the thread's workspace holds expanded rows, popcounts, norms, thresholds and key lists (hm_topk_expanded,
# hamming_mfma_topk_device, topk_device_k, l2_topk_device) - values, nothing that addresses memory - so two calls sharing it give wrong keys,
# not a fault. AKAZE keeps tables of offsets there and stays out on purpose.

def _hamming_call(env, q, nq, t, nt, out, sp):
    L, check = env[2], env[3]
    check(L.apds_dev_hamming_topk(q.data_ptr(), nq, t.data_ptr(), nt, 0, 2, out.data_ptr(), sp))


def _l2_call(env, q, nq, t, nt, out, sp):
    L, check = env[2], env[3]
    check(L.apds_dev_l2_topk(q.data_ptr(), nq, t.data_ptr(), nt, sc.PAIR_L2_DIM, 0, 2, out.data_ptr(), sp))


def _pair_data(env, gpu_pkg, kind, nq, nt, seed, self_queries):
    torch, d = env[0], env[1]
    if kind == "hamming":
        t = sc.pad64(gpu_pkg.synth.make_descriptor_db(nt, seed=seed))
        q = t[:nq].copy() if self_queries else sc.pad64(gpu_pkg.synth.make_queries(t[:, :61], nq, seed=seed + 1)[0])
    else:
        rng = np.random.default_rng(seed)
        t = rng.standard_normal((nt, sc.PAIR_L2_DIM)).astype(np.float32)
        q = t[:nq].copy() if self_queries else (t[rng.integers(0, nt, nq)] + 0.05 * rng.standard_normal((nq, sc.PAIR_L2_DIM))).astype(np.float32)
    return torch.from_numpy(q).to(d), torch.from_numpy(t).to(d)


@pytest.mark.parametrize("x_kind,y_kind", [("hamming", "hamming"), ("hamming", "l2"), ("l2", "hamming")])
def test_two_streams_one_thread_do_not_share_scratch(env, gpu_pkg, delay_cycles, x_kind, y_kind):
    torch, d = env[0], env[1]
    call = {"hamming": _hamming_call, "l2": _l2_call}
    (xq_n, xt_n), (yq_n, yt_n) = sc.PAIR_X, sc.PAIR_Y
    xq, xt = _pair_data(env, gpu_pkg, x_kind, xq_n, xt_n, 301, False)
    yq, yt = _pair_data(env, gpu_pkg, y_kind, yq_n, yt_n, 303, True)
    new = lambda n: torch.empty((n, 2), dtype=torch.int64, device=d)   # noqa: E731
    A = torch.cuda.Stream(d)
    # the synchronised results (and the warm-up of both shapes)
    x_want, y_want = new(xq_n), new(yq_n)
    for _ in range(2):                            # (twice: the second round runs in a workspace that has settled, see _ordered_run)
        torch.cuda.synchronize()
        call[x_kind](env, xq, xq_n, xt, xt_n, x_want, _sp(A))
        torch.cuda.synchronize()
        call[y_kind](env, yq, yq_n, yt, yt_n, y_want, _sp(A))
    torch.cuda.synchronize()
    x_want, y_want = x_want.cpu().numpy().view(np.uint64), y_want.cpu().numpy().view(np.uint64)
    # a query that is a copy of train row i: row i at the lowest distance (exactly 0 for Hamming)
    assert np.array_equal(y_want[:, 0] & np.uint64(0xFFFFFFFF), np.arange(yq_n, dtype=np.uint64))
    if y_kind == "hamming":
        assert not (y_want[:, 0] >> np.uint64(32)).any()

    Bs = [torch.cuda.Stream(d) for _ in range(sc.PAIR_STREAMS)]   # fresh streams, consecutive creations: at most one shares A's hardware queue
    x_got, y_got = new(xq_n), [new(yq_n) for _ in Bs]
    torch.cuda.synchronize()
    e0 = torch.cuda.Event()
    with torch.cuda.stream(A):
        torch.cuda._sleep(delay_cycles)
        e0.record(A)
        call[x_kind](env, xq, xq_n, xt, xt_n, x_got, _sp(A))
    for B, out in zip(Bs, y_got):
        B.wait_event(e0)
        call[y_kind](env, yq, yq_n, yt, yt_n, out, _sp(B))
    pending = not e0.query()
    torch.cuda.synchronize()
    print(f"two streams {x_kind}/{y_kind}: delay pending after the enqueue {pending}")
    assert pending, "the delay had run out before every call was queued: X and the Ys did not start together"
    for i, out in enumerate(y_got):
        g = out.cpu().numpy().view(np.uint64)
        if y_kind == "hamming":
            assert not (g[:, 0] >> np.uint64(32)).any(), f"Y{i}: a query that equals a train row has a non-zero best distance"
        assert np.array_equal(g, y_want), f"Y{i} differs from its synchronised result"
    assert np.array_equal(x_got.cpu().numpy().view(np.uint64), x_want), "X differs from its synchronised result"


# ---- NULL: the thread's own stream ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"hamming_topk-nt{sc.TOPK_NT[0]}-k2", "mask_zero_sat"])
def test_null_is_the_threads_own_stream(env, entries, name):
    torch, d, L, check = env
    e = entries[name]
    ins = [torch.from_numpy(_bytes(a)).to(d) for a in e.real]
    torch.cuda.synchronize()                      # the producer (torch's stream) is done: NULL orders itself against nothing else
    outs = e.run(ins, None)
    assert len(outs) == 1
    host = np.empty(outs[0].numel() * outs[0].element_size(), np.uint8)
    check(L.apds_dev_download(host.ctypes.data, outs[0].data_ptr(), host.nbytes, None))
    assert np.array_equal(host, _bytes(e.want[0]))
