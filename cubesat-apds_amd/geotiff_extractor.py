"""Host-side mirror of the pixel math of the reference crate `geotiff_extractor`
(/root/reference/geotiff_extractor/src/image_extractor/mod.rs) — the step right before the hot path.
GDAL I/O itself is out of scope; these functions take the f32 bands GDAL would deliver."""
import ctypes as C
import struct

import numpy as np

from . import _lib
from ._lib import check, lib, ptr

GAMMA_VALUE = np.float32(1.0) / np.float32(2.2)   # mod.rs:14
U8_MAX = np.float32(255)                           # mod.rs:15


class BandsMinMax:
    """mod.rs `BandsMinMax` (f64 fields)."""

    def __init__(self, red_min, red_max, green_min, green_max, blue_min, blue_max):
        self.red_min, self.red_max, self.green_min, self.green_max, self.blue_min, self.blue_max = (
            float(red_min), float(red_max), float(green_min), float(green_max), float(blue_min), float(blue_max))

    def as_array(self):
        return np.array([self.red_min, self.red_max, self.green_min, self.green_max, self.blue_min, self.blue_max], np.float64)


def band_merger(bands, min_max, bgra=False):
    """mod.rs:346-378 — bands = [red, green, blue] f32 arrays of equal length -> n x 4 u8 (RGBA8; BGRA when bgra=True,
    i.e. fused with homographier::raster_to_mat)."""
    r, g, b = (np.ascontiguousarray(x, np.float32).ravel() for x in bands)
    if not (len(r) == len(g) == len(b)):
        raise _lib.ApdsError(_lib.ERR_ASSERT, "bands differ in length")
    out = np.zeros((len(r), 4), np.uint8)
    mm = min_max.as_array()
    check(lib().apds_band_merger(ptr(r), ptr(g), ptr(b), len(r), ptr(mm), int(bgra), ptr(out)))
    return out


def f32_to_u8(input_value, mn, mx):
    """mod.rs:410-422 — returns the u8 or None where the reference returns Err (NaN, gamma out of range)."""
    v = np.float32(input_value)
    if np.isnan(v):
        return None
    with np.errstate(all="ignore"):
        f = (v - np.float32(mn)) / (np.float32(mx) - np.float32(mn))
    if not (0.0 <= f <= 1.0):
        return None
    out = band_merger([[v], [np.nan], [np.nan]], BandsMinMax(mn, mx, 0, 1, 0, 1))
    return int(out[0, 0])


# ---- minimal TIFF I/O for synthetic mosaics (SURVEY §8f-2 "optional minimal TIFF reader/writer") ---------------------------
# Baseline TIFF, little endian, uncompressed, 32-bit IEEE float samples, strips; chunky or planar. Enough to put a synthetic
# three-band mosaic on disk and read it back the way `MosaicedDataset::to_rgb` consumes a GDAL dataset. Compressed / tiled /
# BigTIFF files (what GDAL's COG driver writes, mod.rs:140-160) are not read: GDAL I/O stays out of scope.
def write_tiff_f32(path, bands):
    """bands: array [n_bands, H, W] (or a list of HxW arrays) of float32 -> one-strip chunky TIFF."""
    b = np.ascontiguousarray(np.stack([np.asarray(x, np.float32) for x in bands]), np.float32)
    nb, h, w = b.shape
    data = np.ascontiguousarray(np.moveaxis(b, 0, 2)).tobytes()          # chunky: H x W x bands
    if len(data) >= 2 ** 32 - 1024:
        raise ValueError("classic TIFF is limited to 4 GiB")
    entries = []

    def tag(code, typ, values):
        entries.append((code, typ, list(values)))

    tag(256, 4, [w]); tag(257, 4, [h]); tag(258, 3, [32] * nb); tag(259, 3, [1])
    tag(262, 3, [2 if nb >= 3 else 1]); tag(273, 4, [0]); tag(277, 3, [nb]); tag(278, 4, [h])
    tag(279, 4, [len(data)]); tag(284, 3, [1]); tag(339, 3, [3] * nb)
    if nb > 3:
        tag(338, 3, [0] * (nb - 3))                                       # ExtraSamples: unspecified
    entries.sort()
    ifd_off = 8
    ifd_size = 2 + 12 * len(entries) + 4
    extra_off = ifd_off + ifd_size
    extra = b""
    body = b""
    fixups = {}
    for code, typ, vals in entries:
        fmt = "<" + {3: "H", 4: "I"}[typ] * len(vals)
        raw = struct.pack(fmt, *vals)
        if len(raw) <= 4:
            field = raw.ljust(4, b"\0")
        else:
            field = struct.pack("<I", extra_off + len(extra))
            extra += raw + (b"\0" if len(raw) % 2 else b"")
        fixups[code] = len(body) + 8
        body += struct.pack("<HHI", code, typ, len(vals)) + field
    data_off = extra_off + len(extra)
    body = bytearray(body)
    body[fixups[273]:fixups[273] + 4] = struct.pack("<I", data_off)       # StripOffsets
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, ifd_off))
        f.write(struct.pack("<H", len(entries)) + bytes(body) + struct.pack("<I", 0))
        f.write(extra)
        f.write(data)


def read_tiff_f32(path):
    """-> float32 array [n_bands, H, W]. Raises ValueError for anything but uncompressed float32 strips."""
    raw = np.fromfile(path, np.uint8)
    view = memoryview(raw)

    def rd(fmt, off):
        return struct.unpack_from(fmt, view, off)

    if bytes(view[0:2]) != b"II" or rd("<H", 2)[0] != 42:
        raise ValueError("not a little-endian classic TIFF")
    ifd = rd("<I", 4)[0]
    tags = {}
    for i in range(rd("<H", ifd)[0]):
        code, typ, cnt = rd("<HHI", ifd + 2 + 12 * i)
        size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 11: 4, 12: 8}.get(typ)
        if size is None:
            continue
        off = ifd + 2 + 12 * i + 8
        if size * cnt > 4:
            off = rd("<I", off)[0]
        if typ in (3, 4):
            tags[code] = list(rd("<" + ("H" if typ == 3 else "I") * cnt, off))
    w, h = tags[256][0], tags[257][0]
    nb = tags.get(277, [1])[0]
    if tags.get(259, [1])[0] != 1 or set(tags.get(258, [0])) != {32} or set(tags.get(339, [1])) != {3} or 322 in tags:
        raise ValueError("only uncompressed 32-bit float strip TIFFs are read (GDAL I/O is out of scope)")
    offs, cnts = tags[273], tags[279]
    blob = np.concatenate([raw[o:o + c] for o, c in zip(offs, cnts)]).view(np.float32)
    if tags.get(284, [1])[0] == 2:
        return np.ascontiguousarray(blob.reshape(nb, h, w))
    return np.ascontiguousarray(np.moveaxis(blob.reshape(h, w, nb), 2, 0))


class MosaicedDataset:
    """mod.rs `MosaicedDataset` + the `Datasets` methods the preprocessor uses (mod.rs:200-269, 279-288), over an in-memory
    [3, H, W] float32 raster instead of a GDAL handle."""

    def __init__(self, bands):
        self.bands = np.ascontiguousarray(bands, np.float32)
        if self.bands.ndim != 3 or self.bands.shape[0] < 3:
            raise ValueError("bands: [>=3, H, W] float32")
        self.min_max = None
        self._device = None

    def to_device(self, overviews=False, min_size=512):
        """The same raster resident in HBM (DeviceMosaic): windows are resampled and extracted there. overviews=True also builds the
        pyramid a COG carries (DeviceMosaic.build_overviews), which window reads are then served from; this host class itself models the
        read of a dataset without overviews."""
        dm = DeviceMosaic(self.bands)
        if overviews:
            dm.build_overviews(min_size)
        return dm

    @classmethod
    def import_mosaic_dataset(cls, path):
        """mod.rs:279-288"""
        return cls(read_tiff_f32(path))

    def raster_size(self):
        """(width, height), as gdal's Dataset::raster_size (preprocessor/src/main.rs:207)"""
        return self.bands.shape[2], self.bands.shape[1]

    def datasets_min_max(self):
        """mod.rs:200-229 — per-band minimum and maximum (NaN ignored), cached."""
        if self.min_max is None:
            with np.errstate(all="ignore"):
                mm = [(float(np.nanmin(self.bands[i])), float(np.nanmax(self.bands[i]))) for i in range(3)]
            self.min_max = BandsMinMax(mm[0][0], mm[0][1], mm[1][0], mm[1][1], mm[2][0], mm[2][1])
        return self.min_max

    def to_rgb(self, window, window_size, size, resample="nearest"):
        """mod.rs:241-269 — window (x, y) and window_size (w, h) in raster pixels, resampled to size (w, h), then band_merger.
        Returns size[0]*size[1] RGBA8 pixels. Equal sizes are copied; otherwise resample="nearest" (the default) decimates by nearest
        neighbour ((i + 0.5) * window / size, floored) on the host, resample="lanczos" is the reference's read (GDAL's Lanczos, mod.rs:339,
        as DESIGN.md section 2 restates it) on a device copy of the raster."""
        x0, y0 = int(window[0]), int(window[1])
        ww, wh = int(window_size[0]), int(window_size[1])
        ow, oh = int(size[0]), int(size[1])
        W, H = self.raster_size()
        if x0 < 0 or y0 < 0 or ww <= 0 or wh <= 0 or x0 + ww > W or y0 + wh > H or ow <= 0 or oh <= 0:
            raise _lib.ApdsError(_lib.ERR_OUT_OF_RANGE, "window outside the raster")
        win = self.window(window, window_size, size, resample)
        return band_merger([np.ascontiguousarray(win[i]).ravel() for i in range(3)], self.datasets_min_max())

    def window(self, window, window_size, size, resample="nearest"):
        """The three f32 band windows `to_rgb` merges ([3, size_h, size_w]; a strided view of the mosaic when no resampling is needed)."""
        if _lib.resample_mode(resample) == _lib.RESAMPLE_LANCZOS:
            if self._device is None:
                self._device = self.to_device()       # created on first use, lives as long as the dataset
            return self._device.window(window, window_size, size, resample)
        x0, y0 = int(window[0]), int(window[1])
        ww, wh = int(window_size[0]), int(window_size[1])
        ow, oh = int(size[0]), int(size[1])
        W, H = self.raster_size()
        if x0 < 0 or y0 < 0 or ww <= 0 or wh <= 0 or x0 + ww > W or y0 + wh > H or ow <= 0 or oh <= 0:
            raise _lib.ApdsError(_lib.ERR_OUT_OF_RANGE, "window outside the raster")
        win = self.bands[:3, y0:y0 + wh, x0:x0 + ww]
        if (ow, oh) != (ww, wh):
            ys = np.minimum(((np.arange(oh) + 0.5) * (wh / oh)).astype(np.int64), wh - 1)
            xs = np.minimum(((np.arange(ow) + 0.5) * (ww / ow)).astype(np.int64), ww - 1)
            win = win[:, ys][:, :, xs]
        return win


class DeviceMosaic:
    """The `MosaicedDataset` methods the preprocessor uses, on a [3, H, W] float32 raster resident in HBM (apds_mosaic_*): min/max is a
    device reduction, windows are resampled on the device (resample="nearest": the host mirror's rule bit for bit; "lanczos": the
    reference's read_as(.., Lanczos), mod.rs:332-343), and the preprocessor extracts tiles from it without the bands crossing PCIe.
    After build_overviews() the handle also holds the overview pyramid of the reference's COG (cubic, factor 2 per level), and every
    window read is served from the level GDAL would pick."""

    def __init__(self, bands):
        b = np.asarray(bands)
        if b.ndim != 3 or b.shape[0] < 3 or b.dtype != np.float32 or b.strides[2] != 4 or b.strides[1] % 4:
            b = np.ascontiguousarray(bands, np.float32)
            if b.ndim != 3 or b.shape[0] < 3:
                raise ValueError("bands: [>=3, H, W] float32")
        self._shape = (b.shape[1], b.shape[2])
        self._handle = C.c_void_p()
        check(lib().apds_mosaic_create(C.byref(self._handle), b[0].ctypes.data, b[1].ctypes.data, b[2].ctypes.data, b.shape[1], b.shape[2],
                                       b.strides[1] // 4, 0))
        self.min_max = None

    @property
    def handle(self):
        if not self._handle:
            raise _lib.ApdsError(_lib.ERR_BAD_ARG, "the device mosaic has been closed")
        return self._handle

    def close(self):
        if getattr(self, "_handle", None):
            lib().apds_mosaic_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 (interpreter shutdown)
            pass

    def raster_size(self):
        """(width, height)"""
        return self._shape[1], self._shape[0]

    def datasets_min_max(self):
        """mod.rs:200-229 — per-band minimum and maximum (NaN ignored), reduced on the device and cached in the handle."""
        if self.min_max is None:
            mm = np.zeros(6, np.float64)
            check(lib().apds_mosaic_min_max(self.handle, ptr(mm)))
            self.min_max = BandsMinMax(*mm)
        return self.min_max

    def build_overviews(self, min_size=512):
        """Builds the overview levels (factor 2, 4, ... while the level below exceeds min_size on either axis) and returns how many there
        are. Once per handle, before it is shared between threads; a repeat with the same min_size is a no-op."""
        n = C.c_int(0)
        check(lib().apds_mosaic_build_overviews(self.handle, int(min_size), C.byref(n)))
        return n.value

    def level_size(self, level):
        """(width, height) of overview `level` (0: the raster itself)"""
        rows, cols = C.c_int(0), C.c_int(0)
        check(lib().apds_mosaic_level_info(self.handle, int(level), C.byref(rows), C.byref(cols)))
        return cols.value, rows.value

    def best_level(self, window_size, size):
        """The level a read of window_size -> size is served from (0 without overviews)"""
        level = C.c_int(0)
        check(lib().apds_mosaic_best_level(self.handle, int(window_size[0]), int(window_size[1]), int(size[0]), int(size[1]), C.byref(level)))
        return level.value

    def window_level(self, level, window, window_size, size, resample="nearest"):
        """`window` on the raster of overview `level`, in that level's own pixel coordinates: [3, size_h, size_w]"""
        out = np.zeros((3, max(int(size[1]), 0), max(int(size[0]), 0)), np.float32)
        check(lib().apds_mosaic_window_level(self.handle, int(level), int(window[0]), int(window[1]), int(window_size[0]), int(window_size[1]), int(size[0]),
                                             int(size[1]), _lib.resample_mode(resample), ptr(out)))
        return out

    def window(self, window, window_size, size, resample="nearest"):
        """The three f32 band windows `to_rgb` merges, [3, size_h, size_w], resampled on the device (on a handle with overviews: from the
        level best_level gives)."""
        out = np.zeros((3, max(int(size[1]), 0), max(int(size[0]), 0)), np.float32)
        check(lib().apds_mosaic_window(self.handle, int(window[0]), int(window[1]), int(window_size[0]), int(window_size[1]), int(size[0]), int(size[1]),
                                       _lib.resample_mode(resample), ptr(out)))
        return out

    def to_rgb(self, window, window_size, size, resample="nearest"):
        """mod.rs:241-269 — the resampled window through band_merger: size[0]*size[1] RGBA8 pixels."""
        win = self.window(window, window_size, size, resample)
        return band_merger([win[i].ravel() for i in range(3)], self.datasets_min_max())
