"""The JPEG export contract (include/imagestitch.h, section 'export: baseline JPEG') in numpy: the only oracle of the encoder.

RGBA8 + quality + layout -> a jpeg_writer Frame (integer colour conversion, edge padding, 2x2 chroma means, the integer matrix
FDCT, libjpeg's quality rule on the Annex K tables, rounding quantisation) -> the file, by write_jpeg(..., restart = MCUs per MCU
row).  Every step is signed integer arithmetic: '>>' is an arithmetic shift, '//' floor division of non-negative numbers.  The
library's file must equal encode()'s byte for byte.
"""
import numpy as np

from tests.jpeg_writer import Q_CHROMA, Q_LUMA, ZIGZAG, _new_frame, write_jpeg

_COS = (4017, 3784, 3406, 2896, 2276, 1567, 799)        # round(4096 cos(k pi / 16)), k = 1 .. 7


def fdct_matrix():
    """T[u][x]: the rounded value of 8192 a(u) cos((2x+1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2, built by the folding rule"""
    T = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            if u == 0:
                T[u, x] = 2896
                continue
            k, sign = ((2 * x + 1) * u) % 32, 1
            if k > 16:
                k = 32 - k
            if k > 8:
                k, sign = 16 - k, -1
            T[u, x] = sign * _COS[k - 1]
    return T


T = fdct_matrix()


def quant_tables(quality):
    """(luma, chroma), natural order, libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)"""
    if not 1 <= quality <= 100:
        raise ValueError("quality must be 1..100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def planes(rgba):
    a = np.asarray(rgba).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16
    return y, cb, cr


def fdct_quant(plane, q):
    """plane (multiple of 8 on both sides, 0..255) -> blocks_y x blocks_x x 64 quantised coefficients, natural order"""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    s = (plane - 128).reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)                 # [by, bx, y, x]
    r = (np.einsum("ux,abyx->abyu", T, s) + 512) >> 10                            # rows
    c = (np.einsum("vy,abyu->abvu", T, r) + 4096) >> 13                           # columns: 8 x the orthonormal coefficient
    c = c.reshape(by, bx, 64)
    k = np.sign(c) * ((np.abs(c) + 4 * q) // (8 * q))
    k[..., 1:] = np.clip(k[..., 1:], -1023, 1023)
    return k


def frame(rgba, quality=90, layout="420"):
    """the jpeg_writer Frame of an H x W x 4 uint8 canvas (alpha is not read)"""
    rgba = np.asarray(rgba)
    H, W = rgba.shape[:2]
    ql, qc = quant_tables(quality)
    m = 16 if layout == "420" else 8
    ph, pw = -(-H // m) * m, -(-W // m) * m
    full = [np.pad(p, ((0, ph - H), (0, pw - W)), mode="edge") for p in planes(rgba)]
    if layout == "420":
        for i in (1, 2):
            p = full[i]
            full[i] = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    f = _new_frame(W, H, layout, [ql, qc, qc])
    for c, p, q in zip(f.comps, full, (ql, qc, qc)):
        assert c["coef"].shape[:2] == (p.shape[0] // 8, p.shape[1] // 8)
        c["coef"] = fdct_quant(p, q)
    return f


def mcus_per_row(width, layout):
    return -(-width // (16 if layout == "420" else 8))


def encode(rgba, quality=90, layout="420"):
    f = frame(rgba, quality, layout)
    return write_jpeg(f, sof=0, marker="jfif", huff="std", restart=mcus_per_row(f.width, layout))


def max_zero_run(f):
    """the longest run of zeros in front of a non-zero AC coefficient, over the frame (>= 16: the file holds a ZRL)"""
    best = 0
    for c in f.comps:
        z = c["coef"].reshape(-1, 64)[:, ZIGZAG]
        for row in z[np.any(z[:, 1:] != 0, axis=1)]:
            nz = np.nonzero(row[1:])[0] + 1
            best = max(best, int(np.max(np.diff(np.concatenate([[0], nz])) - 1)))
    return best
