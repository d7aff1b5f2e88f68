"""The reduced-size JPEG decode contract (include/imagestitch.h, "reduced-size JPEG decode") restated in numpy: a jpeg_writer.Frame
decoded at 1 / d of its natural size, d in {1, 2, 4, 8} - libjpeg-turbo's decode-to-scale, integer for integer.  Test infrastructure
only; tests/test_jpeg_scaled_reference.py pins it against Pillow's Image.draft byte for byte, tests/test_gpu_jpeg_scaled.py pins the
GPU decode against it.

With N = 8 / d: every component gets an S x S inverse DCT (S from idct_size), its plane is cropped to its true size, doubled along
one axis where it is still coarser than the output (triangle filter, or replication at d = 8 and for planes at most 2 samples wide),
cropped to the output size ceil(W N / 8) x ceil(H N / 8) and colour-converted with the full-size 16-bit fixed-point constants."""
import numpy as np


def F(x):
    return int(round(x * 8192))


def _i32(x):
    """the arithmetic is 32-bit: wrap like an int32 register"""
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def descale(x, n):
    return _i32(_i32(x) + (1 << (n - 1))) >> n


def scaled_size(w, h, d):
    n = 8 // d
    return -(-w * n // 8), -(-h * n // 8)


def idct_size(n, h, v, hmax, vmax):
    s = n
    while s < 8 and (hmax * n) % (h * s * 2) == 0 and (vmax * n) % (v * s * 2) == 0:
        s *= 2
    return s


def _pass8(v, sh):
    """one 1-D pass of the full-size (slow integer) IDCT"""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * F(0.541196100)
    t2 = z1 - z3 * F(1.847759065)
    t3 = z1 + z2 * F(0.765366865)
    t0, t1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * F(1.175875602)
    a0, a1, a2, a3 = a0 * F(0.298631336), a1 * F(2.053119869), a2 * F(3.072711026), a3 * F(1.501321110)
    z1, z2 = -z1 * F(0.899976223), -z2 * F(2.562915447)
    z3, z4 = -z3 * F(1.961570560) + z5, -z4 * F(0.390180644) + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return [descale(t10 + a3, sh), descale(t11 + a2, sh), descale(t12 + a1, sh), descale(t13 + a0, sh),
            descale(t13 - a0, sh), descale(t12 - a1, sh), descale(t11 - a2, sh), descale(t10 - a3, sh)]


def _pass4(v, sh):
    t0 = v[0] << 14
    t2 = v[2] * F(1.847759065) - v[6] * F(0.765366865)
    t10, t12 = t0 + t2, t0 - t2
    o0 = -v[7] * F(0.211164243) + v[5] * F(1.451774981) - v[3] * F(2.172734803) + v[1] * F(1.061594337)
    o2 = -v[7] * F(0.509795579) - v[5] * F(0.601344887) + v[3] * F(0.899976223) + v[1] * F(2.562915447)
    return [descale(t10 + o2, sh), descale(t12 + o0, sh), descale(t12 - o0, sh), descale(t10 - o2, sh)]


def _pass2(v, sh):
    t10 = v[0] << 15
    t0 = -v[7] * F(0.720959822) + v[5] * F(0.850430095) - v[3] * F(1.272758580) + v[1] * F(3.624509785)
    return [descale(t10 + t0, sh), descale(t10 - t0, sh)]


_PASSES = {8: (_pass8, 11, 18), 4: (_pass4, 12, 19), 2: (_pass2, 13, 20)}


def idct(co, s):
    """dequantised coefficients [..., v, u] (int64) -> [..., s, s] samples before the level shift.  Pass 1 runs down the columns, pass
    2 along the rows; the reduced passes never read the indices the contract leaves out (their results for unused columns are
    computed and ignored, which changes nothing)."""
    if s == 1:
        return descale(co[..., 0:1, 0:1], 3)
    fn, sh1, sh2 = _PASSES[s]
    ws = np.stack(fn([co[..., r, :] for r in range(8)], sh1), -2)          # [..., s, 8]
    return np.stack(fn([ws[..., :, c] for c in range(8)], sh2), -1)        # [..., s, s]


def _h2v1(p, fancy):
    if not fancy:
        return np.repeat(p, 2, 1)
    n = p.shape[1]
    i = np.arange(n)
    prev, nxt = p[:, np.maximum(i - 1, 0)], p[:, np.minimum(i + 1, n - 1)]
    ev, od = (3 * p + prev + 1) >> 2, (3 * p + nxt + 2) >> 2
    ev[:, 0], od[:, -1] = p[:, 0], p[:, -1]
    return np.stack([ev, od], 2).reshape(p.shape[0], 2 * n)


def _h1v2(p, fancy):
    if not fancy:
        return np.repeat(p, 2, 0)
    n = p.shape[0]
    j = np.arange(n)
    prev, nxt = p[np.maximum(j - 1, 0)], p[np.minimum(j + 1, n - 1)]
    return np.stack([(3 * p + prev + 1) >> 2, (3 * p + nxt + 2) >> 2], 1).reshape(2 * n, p.shape[1])


def geometry(f, d):
    """per component (S, cw, ch, ux, uy)"""
    n = 8 // d
    out = []
    for c in f.comps:
        h, v = f.eff(c)
        s = idct_size(n, h, v, f.hmax, f.vmax)
        out.append((s, -(-f.width * h * s // (f.hmax * 8)), -(-f.height * v * s // (f.vmax * 8)), f.hmax * n // (h * s), f.vmax * n // (v * s)))
    return out


def decode(f, d):
    """Frame -> sh x sw (grey) or sh x sw x 3 (RGB) int64 in 0..255, at 1 / d.  d = 1 is the full-size decode."""
    n = 8 // d
    sw, sh = scaled_size(f.width, f.height, d)
    planes = []
    for c, (s, cw, ch, ux, uy) in zip(f.comps, geometry(f, d)):
        co = (c["coef"].astype(np.int64) * np.asarray(c["q"], np.int64))
        by, bx = co.shape[:2]
        smp = idct(co.reshape(by, bx, 8, 8), s)
        p = np.clip(smp + 128, 0, 255).transpose(0, 2, 1, 3).reshape(by * s, bx * s)[:ch, :cw]
        if (ux, uy) == (2, 1):
            p = _h2v1(p, n > 1 and cw > 2)
        elif (ux, uy) == (1, 2):
            p = _h1v2(p, n > 1)
        elif (ux, uy) == (2, 2):                       # full size only: vertical 3:1 first (unscaled), then horizontal, one shift by 4
            assert d == 1
            if cw > 2:
                j = np.arange(ch)
                rows = np.stack([3 * p + p[np.maximum(j - 1, 0)], 3 * p + p[np.minimum(j + 1, ch - 1)]], 1).reshape(2 * ch, cw)
                i = np.arange(cw)
                l, r = rows[:, np.maximum(i - 1, 0)], rows[:, np.minimum(i + 1, cw - 1)]
                p = np.stack([(3 * rows + l + 8) >> 4, (3 * rows + r + 7) >> 4], 2).reshape(2 * ch, 2 * cw)
            else:
                p = np.repeat(np.repeat(p, 2, 0), 2, 1)
        else:
            assert (ux, uy) == (1, 1), (ux, uy)
        planes.append(p[:sh, :sw])
    if len(planes) == 1:
        return planes[0]
    if f.colour == "rgb":
        return np.stack(planes, -1)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255)


def decode_rgba(f, d):
    """what the library stores: sh x sw x 4 uint8, grey replicated, alpha 255"""
    a = decode(f, d)
    if a.ndim == 2:
        a = np.repeat(a[..., None], 3, 2)
    return np.concatenate([a, np.full(a.shape[:2] + (1,), 255, np.int64)], -1).astype(np.uint8)
