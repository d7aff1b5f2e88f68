"""The colour contract of include/imagestitch.h ("colour profiles"), restated in numpy: an ICC profile -> kind + integer tables,
and RGBA8 pixels through those tables to sRGB.  All integer; the curve functions are evaluated per entry with math.pow, which is
the C library's pow - the same call the library makes.  The GPU agrees with convert() byte for byte."""
import math
import struct

import numpy as np

NONE, IDENTITY, CONVERT, UNSUPPORTED = 0, 1, 2, 3

INV = ((52584397, -27133356, -8233164), (-16421465, 32147857, 561266), (1207600, -3841813, 23584544))      # sRGB colorants (D50) inverted, Q24
SRGB_COLORANTS = ((28576, 25239, 9375), (14581, 46983, 3972), (912, 6361, 46787))                          # s15.16; rows X, Y, Z

# T[c] = ceil(65535 s((c - 0.5) / 255)), c = 1 .. 255 (T[0] is a placeholder): the literal the library carries (csrc/ist_icc.h)
T = (
      0,    10,    30,    50,    70,    90,   110,   130,   150,   170,   189,   209,   230,   253,   276,   301,
    327,   354,   382,   412,   443,   475,   509,   544,   580,   618,   657,   698,   740,   783,   828,   875,
    923,   972,  1023,  1075,  1129,  1185,  1242,  1300,  1360,  1422,  1486,  1551,  1617,  1685,  1755,  1827,
   1900,  1975,  2052,  2130,  2210,  2292,  2376,  2461,  2548,  2637,  2727,  2820,  2914,  3010,  3108,  3208,
   3309,  3412,  3518,  3625,  3734,  3844,  3957,  4072,  4188,  4307,  4427,  4550,  4674,  4800,  4928,  5059,
   5191,  5325,  5461,  5599,  5740,  5882,  6026,  6173,  6321,  6471,  6624,  6778,  6935,  7094,  7255,  7418,
   7583,  7750,  7919,  8091,  8265,  8440,  8618,  8798,  8981,  9165,  9352,  9541,  9732,  9925, 10121, 10318,
  10518, 10720, 10925, 11132, 11341, 11552, 11765, 11981, 12199, 12420, 12643, 12868, 13095, 13325, 13557, 13791,
  14028, 14267, 14508, 14752, 14998, 15247, 15498, 15751, 16007, 16265, 16525, 16788, 17054, 17321, 17592, 17864,
  18139, 18417, 18697, 18980, 19264, 19552, 19842, 20134, 20429, 20727, 21027, 21329, 21634, 21942, 22252, 22564,
  22880, 23197, 23518, 23840, 24166, 24494, 24824, 25158, 25493, 25832, 26173, 26516, 26862, 27211, 27563, 27917,
  28273, 28633, 28995, 29359, 29727, 30097, 30469, 30845, 31223, 31603, 31987, 32373, 32762, 33153, 33547, 33944,
  34344, 34747, 35152, 35560, 35970, 36384, 36800, 37219, 37640, 38065, 38492, 38922, 39355, 39790, 40229, 40670,
  41114, 41561, 42011, 42463, 42918, 43377, 43838, 44301, 44768, 45238, 45710, 46185, 46663, 47144, 47628, 48115,
  48605, 49097, 49593, 50091, 50592, 51096, 51604, 52114, 52627, 53142, 53661, 54183, 54708, 55235, 55766, 56300,
  56836, 57376, 57918, 58464, 59012, 59564, 60118, 60675, 61236, 61799, 62366, 62935, 63508, 64083, 64662, 65244,
)


def srgb_to_linear(x):
    return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)


def thresholds_by_formula():
    return (0,) + tuple(int(math.ceil(65535.0 * srgb_to_linear((c - 0.5) / 255.0))) for c in range(1, 256))


def encode(o):
    """the output code of linear values o (any integer array in 0 .. 65535): the number of c in 1 .. 255 with T[c] <= o"""
    return np.searchsorted(np.asarray(T[1:], np.int64), np.asarray(o, np.int64), side="right").astype(np.uint8)


def _quantise(y):
    q = math.floor(65535.0 * y + 0.5)
    return 0 if not q > 0 else 65535 if q >= 65535 else int(q)


def _curve(tag):
    """one TRC tag -> 256 uint16, or None"""
    if len(tag) < 12:
        return None
    if tag[:4] == b"curv":
        n = struct.unpack(">I", tag[8:12])[0]
        if n > (len(tag) - 12) // 2:
            return None
        if n == 0:
            return [257 * v for v in range(256)]
        if n == 1:
            g8 = struct.unpack(">H", tag[12:14])[0]
            if g8 == 0:
                return None
            return [_quantise(math.pow(v / 255.0, g8 / 256.0)) for v in range(256)]
        t = struct.unpack(">%dH" % n, tag[12:12 + 2 * n])
        out = []
        for v in range(256):
            p = v * (n - 1)
            i, r = p // 255, p % 255
            out.append((t[i] * (255 - r) + t[min(i + 1, n - 1)] * r + 127) // 255)
        return out
    if tag[:4] == b"para":
        ftype = struct.unpack(">H", tag[8:10])[0]
        if ftype > 4:
            return None
        np_ = (1, 3, 4, 5, 7)[ftype]
        if len(tag) < 12 + 4 * np_:
            return None
        q = [v / 65536.0 for v in struct.unpack(">%di" % np_, tag[12:12 + 4 * np_])] + [0.0] * (7 - np_)
        g, a, b, c, d, e, f = q
        if not g > 0.0 or (ftype in (1, 2) and a == 0.0):
            return None
        out = []
        for v in range(256):
            x = v / 255.0
            base = a * x + b if a * x + b > 0.0 else 0.0
            if ftype == 0:
                y = math.pow(x, g)
            elif ftype == 1:
                y = math.pow(base, g) if x >= -b / a else 0.0
            elif ftype == 2:
                y = math.pow(base, g) + c if x >= -b / a else c
            elif ftype == 3:
                y = math.pow(base, g) if x >= d else c * x
            else:
                y = math.pow(base, g) + e if x >= d else c * x + f
            out.append(_quantise(y))
        return out
    return None


def tables(icc):
    """an ICC profile -> {'kind', 'dec' (3x256 uint16), 'mq' (3x3 int64)}; dec and mq are None for UNSUPPORTED"""
    bad = {"kind": UNSUPPORTED, "dec": None, "mq": None}
    icc = bytes(icc)
    if len(icc) < 132:
        return bad
    size = struct.unpack(">I", icc[:4])[0]
    if size < 132 or size > len(icc) or icc[36:40] != b"acsp" or icc[16:20] != b"RGB " or icc[20:24] != b"XYZ ":
        return bad
    n = struct.unpack(">I", icc[128:132])[0]
    if n > (size - 132) // 12:
        return bad
    tags = {}
    for k in range(n):
        sig, off, ln = struct.unpack(">4sII", icc[132 + 12 * k:144 + 12 * k])
        tags.setdefault(sig, (off, ln))                     # the first tag of a signature is the one that counts
    body = {}
    for sig in (b"rXYZ", b"gXYZ", b"bXYZ", b"rTRC", b"gTRC", b"bTRC"):
        if sig not in tags:
            return bad
        off, ln = tags[sig]
        if off > size or ln > size - off:
            return bad
        body[sig] = icc[off:off + ln]
    C = [[0] * 3 for _ in range(3)]
    for j, sig in enumerate((b"rXYZ", b"gXYZ", b"bXYZ")):
        t = body[sig]
        if len(t) < 20 or t[:4] != b"XYZ ":
            return bad
        for k, v in enumerate(struct.unpack(">3i", t[8:20])):
            C[k][j] = v
    mq = [[(sum(INV[i][k] * C[k][j] for k in range(3)) + (1 << 23)) >> 24 for j in range(3)] for i in range(3)]
    if any(not -2 ** 31 <= v < 2 ** 31 for row in mq for v in row):
        return bad
    dec = [_curve(body[sig]) for sig in (b"rTRC", b"gTRC", b"bTRC")]
    if any(d is None for d in dec):
        return bad
    dec = np.asarray(dec, np.uint16)
    mq = np.asarray(mq, np.int64)
    same = np.array_equal(mq, 65536 * np.eye(3, dtype=np.int64)) and all(np.array_equal(encode(dec[c]), np.arange(256)) for c in range(3))
    return {"kind": IDENTITY if same else CONVERT, "dec": dec, "mq": mq}


def convert(tab, rgba):
    """RGBA8 pixels (any shape x 4) through the tables of a CONVERT / IDENTITY profile; alpha is copied"""
    rgba = np.asarray(rgba, np.uint8)
    lin = np.stack([tab["dec"][j][rgba[..., j]].astype(np.int64) for j in range(3)], -1)
    out = rgba.copy()
    for i in range(3):
        o = (tab["mq"][i][0] * lin[..., 0] + tab["mq"][i][1] * lin[..., 1] + tab["mq"][i][2] * lin[..., 2] + (1 << 15)) >> 16
        out[..., i] = encode(np.clip(o, 0, 65535))
    return out
