"""The preview reduce (ist_preview.hip) restated for the tests: numpy, float64, no GPU.  Test infrastructure.

Three things live here.

  the contract   A preview pixel (X, Y) of a w x h image at pw x ph is the overlap-weighted mean of the source under the box
                 [kx X, kx (X + 1)) x [ky Y, ky (Y + 1)), kx = w / pw, ky = h / ph - of the colour bytes under the opaque hint, of
                 the premultiplied bytes c * a and of a otherwise - rounded once and read back with straight alpha.  weights() is one
                 axis of that, unrounded() the mean in fp64: independent of the kernel (no groups, passes or chunks) and of the oracle
                 (no raster, no op list).
  the geometry   geometry() restates preview_geometry (ist_preview_host.cpp): how many output pixels share a 256-column footprint, how
                 many lanes fold a box, how many passes and row chunks a box takes.  CASES are the smallest shapes on either side of
                 every boundary of that rule; each carries the regime it claims, and tests/test_preview_reference.py holds the claims
                 against ist_debug_preview_geometry.
  the rules      exact: integer odd kx and ky make every weight 1.0 and every partial sum an integer below 2^24, so the bytes are
                 known; exact_ok(n) replays the kernel's fp32 finish for every possible sum and says whether it is the integer rule.
                 consistent(): everything else must be a correct rounding of the fp64 reference to within EPS.

EPS = 0.01 LSB is derived, not measured: fp32 unit roundoff 2^-24; the longest chain of roundings in any case of the list is at most
150 (at most 33 row adds per lane, the wave tree, the column loop, 6 shuffles, the passes, at most 64 chunks); relative error at most
150 * 2^-24 = 9e-6, which is 2.3e-3 LSB at 255; EPS is four times that."""
import functools
import math
from collections import namedtuple

import numpy as np

EPS = 0.01
ROUNDOFF_BOUND = 2.3e-3          # the derived bound itself; a measured margin above it is a finding


# ---- the contract ---------------------------------------------------------------------------------------------------------------

def weights(n_out, n_in):
    """(n_out, n_in) fp64: the overlap of source pixel [i, i + 1) with the box [k X, k (X + 1)), k = n_in / n_out, clipped to the
    source.  The edges are X * n_in / n_out with the product exact and one rounding in the division; the last one is n_in itself, so
    there is no sliver beyond the source to drop."""
    edges = np.arange(n_out + 1, dtype=np.float64) * float(n_in) / float(n_out)
    edges = np.clip(edges, 0.0, float(n_in))
    i = np.arange(n_in, dtype=np.float64)
    lo, hi = edges[:-1, None], edges[1:, None]
    return np.maximum(np.minimum(i + 1.0, hi) - np.maximum(i, lo), 0.0)


def planes(img, opaque):
    """what is averaged: the colour planes (opaque form), or the premultiplied planes c * a and a itself"""
    p = img.astype(np.float64)
    if opaque:
        return p[..., :3]
    return np.concatenate([p[..., :3] * p[..., 3:4], p[..., 3:4]], axis=-1)


def reduce_with(p, wy, wx, area):
    """Wy . P . Wx^T / area per plane, fp64"""
    h, w, c = p.shape
    rows = (wy @ p.reshape(h, w * c)).reshape(wy.shape[0], w, c)
    return np.einsum("yjc,xj->yxc", rows, wx) / area


def unrounded(img, pw, ph, opaque):
    """(ph, pw, 3) mean colours under the opaque hint; otherwise (ph, pw, 4): the premultiplied means of c * a, then the mean alpha"""
    h, w = img.shape[:2]
    return reduce_with(planes(img, opaque), weights(ph, h), weights(pw, w), (w * h) / float(pw * ph))


def _round(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.int64)


def readback(r, a):
    """preview_finish's other branch after its one rounding: (colour byte, alpha byte) of a premultiplied colour r under alpha a"""
    r, a = np.asarray(r, np.int64), np.asarray(a, np.int64)
    straight = np.minimum(255, (r * 255 + a // 2) // np.maximum(a, 1))
    return np.where(a == 255, r, np.where(a == 0, 0, straight))


def finish(v, opaque):
    """the bytes of an unrounded result rounded half up: what a kernel that computed v exactly would store"""
    out = np.empty(v.shape[:2] + (4,), np.uint8)
    if opaque:
        out[..., :3] = _round(v[..., :3])
        out[..., 3] = 255
        return out
    a = _round(v[..., 3])
    out[..., :3] = readback(_round(v[..., :3] / 255.0), a[..., None])
    out[..., 3] = a
    return out


def tie_distance(v):
    """how far a value is from the nearest rounding tie x.5"""
    return np.abs(v - np.floor(v) - 0.5)


def rounded_values(v, opaque):
    """the values of an unrounded result that get rounded: colours (opaque form), or premultiplied colours / 255 and alpha"""
    return v[..., :3] if opaque else np.concatenate([v[..., :3] / 255.0, v[..., 3:4]], axis=-1)


def consistent(got, v, eps, opaque):
    """(ph, pw) bool: the pixel's bytes are a correct rounding of the reference v when the kernel's sums are within eps of it.
    Opaque form: |got - v| <= 0.5 + eps per colour byte, alpha 255.  Other form: some a in {floor(alpha -+ eps + 0.5)} and, per
    channel, some r in {floor(rho -+ eps + 0.5)} reads back (readback()) as the pixel's four bytes."""
    g = got.astype(np.int64)
    if opaque:
        return (np.abs(g[..., :3] - v[..., :3]) <= 0.5 + eps).all(axis=-1) & (g[..., 3] == 255)
    rho, alpha = v[..., :3] / 255.0, v[..., 3]
    ok = np.zeros(got.shape[:2], bool)
    for ea in (-eps, eps):
        a = np.clip(np.floor(alpha + ea + 0.5), 0, 255).astype(np.int64)
        this = g[..., 3] == a
        for c in range(3):
            ch = np.zeros(got.shape[:2], bool)
            for er in (-eps, eps):
                r = np.clip(np.floor(rho[..., c] + er + 0.5), 0, 255).astype(np.int64)
                ch |= g[..., c] == readback(r, a)
            this &= ch
        ok |= this
    return ok


def margin(got, v):
    """the largest |got - v| - 0.5 over the colour bytes of an opaque-form result: how far beyond a perfect rounding the worst byte is"""
    return float((np.abs(got[..., :3].astype(np.float64) - v[..., :3]) - 0.5).max())


# ---- the exact rule -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_mismatches(n):
    """the opaque finish of preview_finish replayed in float32 for every integer sum s of n bytes: how many s in [0, 255 n] the
    kernel's trunc(min(float32(s) * float32(1 / n), 255) + 0.5f) takes elsewhere than the integer rule (2 s + n) // (2 n)"""
    assert 255 * n < 1 << 24, n
    s = np.arange(0, 255 * n + 1, dtype=np.int64)
    normf = np.float32(1.0 / float(n))
    k = np.minimum(s.astype(np.float32) * normf, np.float32(255.0)) + np.float32(0.5)
    assert k.dtype == np.float32
    return int((np.trunc(k).astype(np.int64) != (2 * s + n) // (2 * n)).sum())


def exact_ok(n):
    return exact_mismatches(n) == 0


@functools.lru_cache(maxsize=None)
def exact_mismatches_translucent(n):
    """the other finish replayed in float64 for every integer sum of n pixels: the mean alpha over s in [0, 255 n] against
    (2 s + n) // (2 n), the premultiplied mean / 255 over s in [0, 255 * 255 n] against (2 s + 255 n) // (2 * 255 n)"""
    assert 255 * 255 * n < 1 << 24, n
    norm = 1.0 / float(n)
    bad = 0
    for top, div, den in ((255 * n, 1.0, n), (255 * 255 * n, 255.0, 255 * n)):
        for at in range(0, top + 1, 1 << 21):
            s = np.arange(at, min(at + (1 << 21), top + 1), dtype=np.int64)
            k = np.clip(np.floor(s.astype(np.float32).astype(np.float64) * norm / div + 0.5), 0.0, 255.0)
            bad += int((k.astype(np.int64) != (2 * s + den) // (2 * den)).sum())
    return bad


def _block_sums(p, pw, ph):
    h, w, c = p.shape
    assert h % ph == 0 and w % pw == 0
    return p.reshape(ph, h // ph, pw, w // pw, c).sum(axis=(1, 3))


def exact_bytes(img, pw, ph):
    """integer kx, ky, opaque pixels: every colour byte is (2 s + n) // (2 n) of its box's sum s, alpha 255"""
    h, w = img.shape[:2]
    n = (h // ph) * (w // pw)
    out = np.empty((ph, pw, 4), np.uint8)
    out[..., :3] = (2 * _block_sums(img[..., :3].astype(np.int64), pw, ph) + n) // (2 * n)
    out[..., 3] = 255
    return out


def exact_bytes_translucent(img, pw, ph):
    """integer kx, ky, any alpha, in integers: one rounding of the premultiplied mean and of the mean alpha, then the straight-alpha
    readback (preview_finish without the hint)"""
    h, w = img.shape[:2]
    n = (h // ph) * (w // pw)
    p = img.astype(np.int64)
    sa = _block_sums(p[..., 3:4], pw, ph)
    sca = _block_sums(p[..., :3] * p[..., 3:4], pw, ph)
    a = (2 * sa + n) // (2 * n)
    r = (2 * sca + 255 * n) // (2 * 255 * n)
    out = np.empty((ph, pw, 4), np.uint8)
    out[..., :3] = readback(r, a)
    out[..., 3] = a[..., 0]
    return out


# ---- the geometry ---------------------------------------------------------------------------------------------------------------

Geometry = namedtuple("Geometry", "per_group groups passes sub chunk_rows chunks")


def geometry(w, h, pw, ph):
    """preview_geometry restated: None for a shape the reduce does not take (the job path)"""
    if pw < 1 or ph < 1 or w <= pw or h <= ph or w > 1 << 30 or h > 1 << 30:
        return None
    kx, ky = w / pw, h / ph
    per_group = int(max(1.0, math.floor(253.0 / kx)))
    groups = (pw + per_group - 1) // per_group
    passes = 1 if per_group > 1 else (math.ceil(kx) + 3 + 255) // 256
    box_cols = min(64, math.ceil(kx) + 1)
    sub = 1
    while sub < box_cols:
        sub <<= 1
    box_rows = math.ceil(ky) + 2
    chunk_rows = max(64, ((box_rows + 63) // 64 + 3) & ~3)
    chunks = (box_rows + chunk_rows - 1) // chunk_rows
    return Geometry(per_group, groups, passes, sub, chunk_rows, chunks)


def rounds(g, pw):
    """column rounds of a full group: 256 / sub output pixels are folded at a time"""
    return -(-min(g.per_group, pw) // (256 // g.sub))


# (w, h, pw, ph), the regime the case claims - per_group, sub, column rounds, passes, chunks, chunk_rows - and the rule it is held to
# under the opaque hint: 'exact' (byte equality; tests/test_preview_reference.py replays exact_ok for each) or 'consistent'
Case = namedtuple("Case", "w h pw ph per_group sub rounds passes chunks chunk_rows rule", defaults=("exact",))


def case_id(c):
    return "%dx%d-%dx%d" % (c.w, c.h, c.pw, c.ph)


# integer odd kx and ky.  The kx sweep at ky = 3: two full groups and a ragged third, or three one-pixel groups.
KX_SWEEP = [
    Case(507, 15, 169, 5, 84, 4, 2, 1, 1, 64),       # 3
    Case(510, 15, 170, 5, 84, 4, 2, 1, 1, 64),       # 3, an even width (odd kx times odd pw is odd): w mod 4 = 2
    Case(516, 15, 172, 5, 84, 4, 2, 1, 1, 64),       # 3, w mod 4 = 0
    Case(505, 15, 101, 5, 50, 8, 2, 1, 1, 64),       # 5
    Case(511, 15, 73, 5, 36, 8, 2, 1, 1, 64),        # 7
    Case(513, 15, 57, 5, 28, 16, 2, 1, 1, 64),       # 9
    Case(495, 15, 33, 5, 16, 16, 1, 1, 1, 64),       # 15
    Case(493, 15, 29, 5, 14, 32, 2, 1, 1, 64),       # 17
    Case(527, 15, 17, 5, 8, 32, 1, 1, 1, 64),        # 31
    Case(495, 15, 15, 5, 7, 64, 2, 1, 1, 64),        # 33
    Case(567, 15, 9, 5, 4, 64, 1, 1, 1, 64),         # 63
    Case(455, 15, 7, 5, 3, 64, 1, 1, 1, 64),         # 65: a box wider than sub, the strided column loop
    Case(625, 15, 5, 5, 2, 64, 1, 1, 1, 64),         # 125
    Case(381, 15, 3, 5, 1, 64, 1, 1, 1, 64),         # 127: per_group 1
    Case(759, 15, 3, 5, 1, 64, 1, 1, 1, 64),         # 253: the widest box of one pass
    Case(765, 15, 3, 5, 1, 64, 1, 2, 1, 64),         # 255: two passes (the second one finds no column left)
    Case(1527, 15, 3, 5, 1, 64, 1, 2, 1, 64),        # 509: two passes, both with columns
    Case(1533, 15, 3, 5, 1, 64, 1, 3, 1, 64),        # 511: three passes (the third one finds no column left)
    Case(1539, 15, 3, 5, 1, 64, 1, 3, 1, 64),        # 513: three passes, all with columns
]
# the ky sweep at kx = 3: on either side of one row per wave slot (ky 13, 15, 17), of 1 -> 2 -> 3 chunks, and many chunks
KY_SWEEP = [Case(21, h, 7, 3, 84, 4, 1, 1, chunks, 64)
            for h, chunks in [(39, 1), (45, 1), (51, 1), (183, 1), (189, 2), (195, 2), (381, 3), (387, 3), (4095, 22)]]
# boxes around 4096 rows: 64 chunks of 64 rows, then taller chunks
TALL = [
    Case(15, 8186, 5, 2, 84, 4, 1, 1, 64, 64),       # ky 4093
    Case(15, 8190, 5, 2, 84, 4, 1, 1, 61, 68),       # ky 4095
    Case(15, 16382, 5, 2, 84, 4, 1, 1, 63, 132),     # ky 8191
]
INTEGER_CASES = KX_SWEEP + KY_SWEEP + TALL
# fractional kx and ky: held to consistent(), both forms
FRACTIONAL_CASES = [
    Case(632, 7, 5, 2, 2, 64, 1, 1, 1, 64, "consistent"),          # kx 126.4: per_group 2, a ragged third group
    Case(633, 7, 5, 2, 1, 64, 1, 1, 1, 64, "consistent"),          # kx 126.6: per_group 1
    Case(506, 7, 4, 2, 2, 64, 1, 1, 1, 64, "consistent"),          # kx 126.5: on the boundary itself
    Case(2529, 7, 10, 2, 1, 64, 1, 1, 1, 64, "consistent"),        # kx 252.9: one pass
    Case(2531, 7, 10, 2, 1, 64, 1, 2, 1, 64, "consistent"),        # kx 253.1: two passes
    Case(258, 38, 257, 37, 252, 4, 4, 1, 1, 64, "consistent"),     # kx 1.004: four column rounds, boxes barely wider than a pixel
    Case(523, 37, 400, 28, 193, 4, 4, 1, 1, 64, "consistent"),     # kx 1.31: three groups, four rounds
    Case(21, 191, 7, 3, 84, 4, 1, 1, 2, 64, "consistent"),         # ky 63.67: the middle box touches 65 rows, the last alone in chunk 1
    Case(601, 97, 273, 44, 114, 4, 2, 1, 1, 64, "consistent"),
    Case(1001, 333, 77, 41, 19, 16, 2, 1, 1, 64, "consistent"),
]
CASES = INTEGER_CASES + FRACTIONAL_CASES

# the batch twin: square noise of side 5 k into a 5 x 5 cell (mode 'fit'): kx = ky = k
BATCH_KS = (3, 15, 17, 63, 65, 127, 253, 255)
# k -> the regime claimed for 5 k x 5 k -> 5 x 5: per_group, sub, passes, chunks
BATCH_REGIMES = {3: (84, 4, 1, 1), 15: (16, 16, 1, 1), 17: (14, 32, 1, 1), 63: (4, 64, 1, 2), 65: (3, 64, 1, 2), 127: (1, 64, 1, 3),
                 253: (1, 64, 1, 4), 255: (1, 64, 2, 5)}
BATCH_EXACT = (3, 15, 17, 63, 65, 127, 255)          # exact_ok(k * k) holds; 253 * 253 fails the replay and goes under consistent()


def integer_n(c):
    """kx * ky of a case with integer ratios, else None"""
    if c.w % c.pw or c.h % c.ph:
        return None
    return (c.w // c.pw) * (c.h // c.ph)


# Seeds are chosen, not measured: with the hint off and n > 257 the premultiplied sums pass 2^24 and are no longer integers in fp32, so
# byte equality holds only where no mean lies within EPS of a tie (consistent() then admits one value per byte).  Every case takes
# seed 1 unless that fails the condition, then the first seed that meets it; tests/test_preview_reference.py checks the condition.
SEEDS = {"625x15-5x5": 3, "765x15-3x5": 6, "1527x15-3x5": 7, "1533x15-3x5": 4, "1539x15-3x5": 2, "21x381-7x3": 2, "21x387-7x3": 3,
         "21x4095-7x3": 7, "15x8186-5x2": 2, "15x16382-5x2": 3}


def seed_of(c):
    return SEEDS.get(case_id(c), 1)


def noise(seed, h, w, opaque=True):
    """per-pixel noise confined to 0..127, so that a pixel read from a surround of 255 raises a sum"""
    a = (np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8) >> 1).astype(np.uint8)
    if opaque:
        a[..., 3] = 255
    return a


def case_image(c, opaque=True):
    """the case's source: opaque noise, or (seed + 1000) translucent noise"""
    return noise(seed_of(c) + (0 if opaque else 1000), c.h, c.w, opaque)
