"""Tables, shapes and a NumPy restatement of the device images of a table (tests/test_gpu_tables.py);
nothing here needs a GPU.  The formats are restated from the comments of mulut_kernels.h, mulut_interval.h and mulut_core.h, never
from the builders of mulut_capi.hip; the quantiser is the fine-tune driver's export line (sr/3_finetune_lut.py:168)."""
import numpy as np

from mulut_amd.lut_io import lut_rows

KINDS = ("random", "min", "max", "ramp")
# (interval, u, pattern): every row size at interval 4 with a band pattern (s) and a wide one (e: full image only), intervals 5 and 6
SHAPES = [(4, u, m) for u in (1, 2, 3, 4) for m in "se"] + [(iv, u, "s") for iv in (5, 6) for u in (1, 2, 3, 4)] + [(5, 4, "e"), (6, 1, "e")]


def table(kind, iv, u, seed=0):
    rows, v = lut_rows(iv), u * u
    if kind == "random":
        return np.random.default_rng(1000 * iv + 10 * u + seed).integers(-128, 128, (rows, v), dtype=np.int8)
    if kind == "min":
        return np.full((rows, v), -128, np.int8)
    if kind == "max":
        return np.full((rows, v), 127, np.int8)
    return ((np.arange(rows * v, dtype=np.int64) * 7 + seed) % 256 - 128).astype(np.int8).reshape(rows, v)      # ramp: every value, row by row


def np_export(w):
    """sr/3_finetune_lut.py:168 on float32 values, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        r = np.round(np.clip(np.asarray(w, np.float32), -1, 1) * 127)
    assert r.dtype == np.float32
    return np.where(np.isnan(r), np.float32(0), r).astype(np.int8)


def full_image(iv, u, t):
    """the full-table image mulut_set_lut uploads for int8 rows t [L^4, u * u]"""
    rows, v = t.shape
    if iv != 4:
        rb = 1 if u == 1 else (v + 3) // 4 * 4
        img = np.zeros((rows * rb + 15) // 16 * 16, np.uint8)
        img[:rows * rb].reshape(rows, rb)[:, :v] = t.view(np.uint8)
        return img
    if u == 1:
        img = np.zeros((rows + 15) // 16 * 16, np.uint8)
        img[:rows] = t.view(np.uint8)[:, 0]
        return img
    rb = (v + 3) // 4 * 4
    img = np.full((rows, rb), 128, np.uint8)
    img[:, :v] = (t.astype(np.int16) + 128).astype(np.uint8)
    return img.reshape(-1)


def tube_image(u, t):
    """the tube band mulut_set_lut uploads for an interval-4 table of an s / d / y pattern (mulut_core.h): the rows whose four keys
    span at most two MSB steps at slot 27 A + 18 B + 12 C + 8 D, values as 16-bit fields, value + 128 for u > 1"""
    k = np.stack(np.meshgrid(*[np.arange(17)] * 4, indexing="ij"), -1).reshape(-1, 4)
    rows = np.flatnonzero(k.max(1) - k.min(1) <= 2)
    slots = k[rows] @ np.array([27, 18, 12, 8])
    assert rows.size == 991 and np.unique(slots).size == 991 and slots.max() == 1040
    n = 1041
    if u == 1:
        band = np.zeros((4176 // 4, 2), np.uint16)
        band[slots] = t[rows, 0].astype(np.int16).view(np.uint16)[:, None]
        return band.view(np.uint8).reshape(-1)
    e = (t[rows].astype(np.int16) + 128).astype(np.uint16)
    if u == 2:
        band = np.full((8336 // 8, 4), 128, np.uint16)
        band[slots] = e
    elif u == 3:        # ten fields e0 e1 e2 e3 e4 e4 e5 e6 e7 e8 in 24 bytes
        band = np.full((24992 // 2,), 128, np.uint16)
        slot_fields = band[:n * 12].reshape(n, 12)
        slot_fields[slots, :10] = e[:, [0, 1, 2, 3, 4, 4, 5, 6, 7, 8]]
    else:               # two planes of 16 bytes per slot: LO dword k = e(4k) | e(4k+2) << 16, HI dword k = e(4k+1) | e(4k+3) << 16
        band = np.full((2, n, 8), 128, np.uint16)
        band[0][slots] = e[:, [0, 2, 4, 6, 8, 10, 12, 14]]
        band[1][slots] = e[:, [1, 3, 5, 7, 9, 11, 13, 15]]
    return np.ascontiguousarray(band).view(np.uint8).reshape(-1)


def slab_image(t):
    """the 16 anchor slab pairs of an interval-4 table with 16-value rows: pair A = rows (A, bcd) and (A + 1, bcd) interleaved,
    value + 128, and a 1 KiB tail of 128"""
    img = (t.astype(np.int16) + 128).astype(np.uint8).reshape(17, 4913, 16)
    pairs = np.stack([img[:16], img[1:]], axis=2)          # [A][bcd][f][16]
    return np.concatenate([pairs.reshape(-1), np.full(1024, 128, np.uint8)])


def images(iv, u, mode, t):
    """[full, tube band, slab pairs] as bytes; b"" where a table of this shape has no such image"""
    band = iv == 4 and mode in "sdy"
    return [full_image(iv, u, t).tobytes(), tube_image(u, t).tobytes() if band else b"", slab_image(t).tobytes() if band and u == 4 else b""]
