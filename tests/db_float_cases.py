"""What the float keypoint table's GPU tests share: synthetic rows, a numpy model of the table that is written from the definitions (the
predicate of keypointdb.rs:50-90, ORDER BY response DESC with ties by row, a delete = the rows without the victims) and never reads
anything back from the library, and the few device helpers the tests need. No test in here."""
import ctypes as C
from importlib import import_module

import numpy as np

LIMIT = 2 ** 18 - 1    # keypointdb.rs:12
EXACT, SCREEN = 0, 1


class Ex:
    def __init__(self, kp, d):
        self.keypoints, self.descriptors = kp, d


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def keypoints(pkg, n, seed, levels=64):
    rng = np.random.default_rng(seed)
    kp = np.zeros(n, pkg._lib.KEYPOINT_DTYPE)
    kp["x"], kp["y"] = rng.integers(0, 400, n), rng.integers(0, 400, n)
    kp["size"], kp["angle"] = rng.random(n, np.float32) * 9, rng.random(n, np.float32) * 360
    kp["response"] = np.round(rng.random(n, np.float32) * levels) / levels          # few levels: ties everywhere
    kp["octave"], kp["class_id"] = rng.integers(0, 4, n), rng.integers(0, 3, n)
    return kp


def unit_rows(n, seed, norm=1.0):
    """[n, 64] float32 rows of (about) the given norm"""
    r = np.random.default_rng(seed).standard_normal((n, 64))
    r *= norm / np.linalg.norm(r, axis=1, keepdims=True)
    return np.ascontiguousarray(r, np.float32)


def byte_rows(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 61), dtype=np.uint8)


class Model:
    """the numpy table: one entry per row, in insertion order. image_of / lod_of: per-row arrays (rows of one image need not be adjacent:
    the table is filled by one insert per run of equal (image, lod))"""

    def __init__(self, kp, img, lod, desc_f, desc_b):
        self.kp = kp.copy()
        self.kp["x"], self.kp["y"] = kp["x"] * np.exp2(lod).astype(np.float32), kp["y"] * np.exp2(lod).astype(np.float32)
        self.src_kp, self.img, self.lod, self.desc_f, self.desc_b = kp, img.astype(np.int32), lod.astype(np.int32), desc_f, desc_b
        self.ids = np.arange(1, len(kp) + 1, dtype=np.int32)
        self.next_id = len(kp) + 1

    def __len__(self):
        return len(self.ids)

    def runs(self):
        """[(start, end)] of the maximal runs of equal (image, lod)"""
        n = len(self)
        if not n:
            return []
        cut = np.flatnonzero((np.diff(self.img) != 0) | (np.diff(self.lod) != 0)) + 1
        edges = [0] + cut.tolist() + [n]
        return list(zip(edges[:-1], edges[1:]))

    def fill(self, table, is_float):
        for a, b in self.runs():
            table.create_keypoints(Ex(self.src_kp[a:b], (self.desc_f if is_float else self.desc_b)[a:b]), int(self.img[a]), int(self.lod[a]))

    def mask(self, mode, value, box=None):
        if mode == 0:
            return self.img == value
        m = self.lod == value
        if mode == 2:
            x0, y0, x1, y1 = np.floor(np.float32(box[0])), np.floor(np.float32(box[1])), np.ceil(np.float32(box[2])), np.ceil(np.float32(box[3]))
            m = m & (self.kp["x"] >= x0) & (self.kp["x"] <= x1) & (self.kp["y"] >= y0) & (self.kp["y"] <= y1)
        return m

    def select(self, mode, value, box=None, limit=LIMIT):
        """table rows of the selection: the predicate, ORDER BY response DESC (-0.0 == +0.0), ties by row, LIMIT"""
        rows = np.flatnonzero(self.mask(mode, value, box))
        r = self.kp["response"][rows].astype(np.float64)
        r[r == 0] = 0.0
        return rows[np.lexsort((rows, -r))][:limit]

    def delete(self, victims):
        """victims: a boolean mask over the rows"""
        keep = ~victims
        for name in ("kp", "src_kp", "img", "lod", "desc_f", "desc_b", "ids"):
            setattr(self, name, getattr(self, name)[keep])
        return int(victims.sum())


def make_tables(pkg, model, capacity=None):
    """(float table, byte table) holding the model's rows"""
    fd = pkg.feature_database
    cap = max(capacity or len(model), 1)
    tf, tb = fd.KeypointTable(cap, descriptor="kaze"), fd.KeypointTable(cap)
    model.fill(tf, True)
    model.fill(tb, False)
    assert len(tf) == len(tb) == len(model)
    return tf, tb


def select(view, mode, value, box=None, **kw):
    if mode == 0:
        return view.read_keypoints_from_image_id(value, **kw)
    if mode == 1:
        return view.read_keypoints_from_lod(value, **kw)
    return view.read_keypoints_from_coordinates(box[0], box[1], box[2], box[3], value, **kw)


def download_view(pkg, view, row_bytes, stream=None):
    """(row ids, keypoints, descriptor rows as bytes [n, row_bytes], image ids) of the view's last selection, ordered on `stream`"""
    r, k, i, g, _, n = view.device_pointers()
    out = [np.zeros(n, np.int32), np.zeros(n, pkg._lib.KEYPOINT_DTYPE), np.zeros((n, row_bytes), np.uint8), np.zeros(n, np.int32)]
    for a, addr in zip(out, (i, k, r, g)):
        if a.nbytes:
            pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(a), addr, a.nbytes, stream))
    return out


def check_views(pkg, model, vf, vb, nf, nb, want, stream=None):
    """the float view and the byte view of the same selection against the model and against each other"""
    rows_f, kp_f, d_f, img_f = download_view(pkg, vf, 256, stream)
    rows_b, kp_b, d_b, img_b = download_view(pkg, vb, 64, stream)
    assert nf == nb == len(want) == len(rows_f) == len(rows_b)
    assert np.array_equal(rows_f, want) and np.array_equal(rows_b, want)
    assert np.array_equal(bits(kp_f), bits(model.kp[want])) and np.array_equal(bits(kp_b), bits(kp_f))
    assert np.array_equal(img_f, model.img[want]) and np.array_equal(img_b, img_f)
    assert np.array_equal(d_f, bits(model.desc_f[want]).reshape(len(want), 256))          # every bit of every float row
    assert np.array_equal(d_b[:, :61], model.desc_b[want]) and not d_b[:, 61:].any()


class Dev:
    """device tensors and the L2 calls on an explicit torch stream (the C ABI reads torch's default stream, handle 0, as "the thread's own")"""

    def __init__(self, pkg):
        import torch
        self.torch, self.pkg = torch, pkg
        self.pl = import_module(pkg.__name__ + ".pipeline")
        self.L, self.check = pkg.lib(), pkg._lib.check
        self.stream = torch.cuda.Stream()

    def handle(self):
        return C.c_void_p(self.stream.cuda_stream)

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.torch.cuda.synchronize()
        return t

    def view_rows(self, view):
        """the view's float rows as a [n, 64] float32 tensor over the view's own memory"""
        r, _, _, _, _, n = view.device_pointers()
        return self.pl._table_tensor(r, max(n, 1) * 256, "cuda:0", self.torch.float32, (max(n, 1), 64))[:n]

    def topk(self, dq, dt):
        out = self.torch.empty((dq.shape[0], 2), dtype=self.torch.int64, device="cuda:0")
        with self.torch.cuda.stream(self.stream):
            self.check(self.L.apds_dev_l2_topk(dq.data_ptr(), dq.shape[0], dt.data_ptr() if dt.shape[0] else None, dt.shape[0], 64, 0, 2, out.data_ptr(),
                                               self.pl.torch_stream()))
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def top2(self, ts, dq, mode):
        with self.torch.cuda.stream(self.stream):
            out = ts.top2(dq, mode)
        self.torch.cuda.synchronize()
        return out.cpu().numpy(), ts.mode_used, ts.candidates_per_query


def download(pkg, addr, shape, dtype, stream=None):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        pkg._lib.check(pkg.lib().apds_dev_download(pkg._lib.ptr(out), addr, out.nbytes, stream))
    return out


class Snapshot:
    """host copy of a table of either kind, by row: descriptor rows as bytes, keypoints, world points and ids through apds_db_table and
    apds_db_ids; image id and level of detail rebuilt from the row ids of one apds_db_select per value (no pointer exposes them)"""

    def __init__(self, pkg, table, image_ids, lods):
        rows, kps, xyz, n = table.device_table()
        assert n == len(table)
        self.n = n
        self.desc = download(pkg, rows, (n, 256 if table.is_float else 64), np.uint8)
        self.kps = download(pkg, kps, n, pkg._lib.KEYPOINT_DTYPE)
        self.xyz = download(pkg, xyz, (n, 3), np.float64) if xyz else None
        self.ids = table.ids()
        self.image_id = self._column(pkg, table, 0, image_ids)
        self.lod = self._column(pkg, table, 1, lods)

    def _column(self, pkg, table, mode, values):
        col = np.full(self.n, -1, np.int32)
        for v in values:
            m = C.c_int(0)
            pkg._lib.check(pkg.lib().apds_db_select(table._h, mode, int(v), 0.0, 0.0, 0.0, 0.0, C.byref(m)))
            assert m.value < LIMIT
            _, _, rows, _, m2 = table.view_device_pointers()
            assert m2 == m.value
            r = download(pkg, rows, m2, np.int32)
            assert (col[r] == -1).all()
            col[r] = v
        return col

    def columns(self):
        """every non-descriptor column"""
        return dict(kps=self.kps, ids=self.ids, image_id=self.image_id, lod=self.lod)


def assert_model(pkg, model, tf, tb, what=""):
    """both tables against the model, every column by row, and the non-descriptor columns of the two kinds against each other"""
    images, lods = sorted(set(model.img.tolist())), sorted(set(model.lod.tolist()))
    sf, sb = Snapshot(pkg, tf, images, lods), Snapshot(pkg, tb, images, lods)
    assert sf.n == sb.n == len(model), (what, sf.n, sb.n, len(model))
    for s in (sf, sb):
        assert s.kps.tobytes() == model.kp.tobytes(), what
        assert np.array_equal(s.ids, model.ids) and np.array_equal(s.image_id, model.img) and np.array_equal(s.lod, model.lod), what
    assert np.array_equal(sf.desc, bits(model.desc_f).reshape(len(model), 256)), what
    assert np.array_equal(sb.desc[:, :61], model.desc_b) and not sb.desc[:, 61:].any(), what
    return sf, sb
