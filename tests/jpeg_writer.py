"""A baseline / extended-sequential JPEG writer and a float64 reference decoder (test infrastructure only).

Written from ITU-T T.81 so that the suite can decode streams no PIL-made file contains: any component IDs and sampling
factors, one scan per component in any order, tables in any slot and redefined between scans, deep Huffman codes,
restart intervals that wrap RSTn, fill bytes and foreign segments between scans, 16-bit quantisation tables, and
coefficients chosen directly (DC category 11, AC category 10, ZRL chains).

A Frame holds the quantised coefficients (natural order) of every component; write_jpeg() entropy-codes it;
reference_decode() turns the same coefficients back into RGB in float64 (T.81 A.3.3 IDCT, libjpeg's upsampling rules,
exact JFIF colour constants), so a file can be checked against what it was meant to hold, independently of any codec.
Everything is deterministic in its seeds; the bit packing is vectorised (a 1 MP file takes a fraction of a second).
"""
import heapq

import numpy as np

# T.81 figure A.6: zig-zag position k -> natural index (row * 8 + column)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,
                   6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38,
                   31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K.1 tables K.1 / K.2 (natural order)
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# T.81 Annex K.3 tables K.3 - K.6: (BITS[1..16], HUFFVAL)
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14,
    0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09,
    0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a,
    0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65,
    0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88,
    0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9,
    0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea,
    0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32,
    0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16,
    0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39,
    0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86,
    0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8,
    0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9,
    0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

# sampling layouts: (colour model, ((h, v) per component))
LAYOUTS = {
    "grey": ("grey", ((1, 1),)),
    "grey22": ("grey", ((2, 2),)),          # a single component whose frame header says 2x2 (it decodes as 1x1)
    "444": ("ycc", ((1, 1), (1, 1), (1, 1))),
    "422": ("ycc", ((2, 1), (1, 1), (1, 1))),
    "420": ("ycc", ((2, 2), (1, 1), (1, 1))),
    "440": ("ycc", ((1, 2), (1, 1), (1, 1))),
    "rgb": ("rgb", ((1, 1), (1, 1), (1, 1))),
    "rgb420": ("rgb", ((2, 2), (1, 1), (1, 1))),
}

_DCT = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for u in range(8)]
                 for x in range(8)])          # M[x, u]: samples = M @ S @ M.T (T.81 A.3.3), S = M.T @ samples @ M


class Frame:
    """width x height, colour 'grey' | 'ycc' | 'rgb'; comps: dicts with id, h, v, q (natural-order table, the one in
    force when the component's first scan starts), tq (slot) and coef (blocks_y x blocks_x x 64 int, natural order,
    padded to whole MCUs)."""

    def __init__(self, width, height, colour, comps):
        self.width, self.height, self.colour, self.comps = width, height, colour, comps

    @property
    def hmax(self):
        return max(c["h"] for c in self.comps) if len(self.comps) > 1 else 1

    @property
    def vmax(self):
        return max(c["v"] for c in self.comps) if len(self.comps) > 1 else 1

    def eff(self, c):
        """sampling factors as the decoder uses them (a lone component is 1x1 whatever its header says)"""
        return (1, 1) if len(self.comps) == 1 else (c["h"], c["v"])


def _new_frame(width, height, layout, qtabs, ids=None, tq=None):
    colour, samp = LAYOUTS[layout] if isinstance(layout, str) else layout
    n = len(samp)
    ids = ids or ((82, 71, 66) if colour == "rgb" and n == 3 else (1, 2, 3))[:n]
    tq = tq or (0, 1, 1)[:n]
    comps = [{"id": ids[i], "h": samp[i][0], "v": samp[i][1], "tq": tq[i], "q": np.asarray(qtabs[i], np.int64)} for i in range(n)]
    f = Frame(width, height, colour, comps)
    mx, my = -(-width // (8 * f.hmax)), -(-height // (8 * f.vmax))
    for c in comps:
        h, v = f.eff(c)
        c["coef"] = np.zeros((my * v, mx * h, 64), np.int64)
    return f


def quant_table(kind, scale):
    base = Q_LUMA if kind == 0 else Q_CHROMA
    return np.clip(np.round(base * scale), 1, 65535).astype(np.int64)


def frame_from_pixels(px, layout, scale=1.0, qtabs=None, ids=None, tq=None):
    """RGB (H x W x 3) or grey (H x W) uint8 -> a Frame: colour conversion, box down-sampling, forward DCT, quantisation."""
    px = np.asarray(px, np.float64)
    H, W = px.shape[:2]
    colour, samp = LAYOUTS[layout] if isinstance(layout, str) else layout
    if colour == "grey":
        planes = [px if px.ndim == 2 else px[..., 0]]
    elif colour == "rgb":
        planes = [px[..., 0], px[..., 1], px[..., 2]]
    else:
        r, g, b = px[..., 0], px[..., 1], px[..., 2]
        planes = [0.299 * r + 0.587 * g + 0.114 * b, -0.168735892 * r - 0.331264108 * g + 0.5 * b + 128,
                  0.5 * r - 0.418687589 * g - 0.081312411 * b + 128]
    if qtabs is None:
        qtabs = [quant_table(0 if i == 0 else 1, scale) for i in range(len(planes))]
    f = _new_frame(W, H, layout, qtabs, ids, tq)
    for c, p in zip(f.comps, planes):
        h, v = f.eff(c)
        sx, sy = f.hmax // h, f.vmax // v
        cw, ch = -(-W // sx), -(-H // sy)
        pp = np.pad(p, ((0, ch * sy - H), (0, cw * sx - W)), mode="edge")
        pp = pp.reshape(ch, sy, cw, sx).mean(axis=(1, 3))
        by, bx = c["coef"].shape[:2]
        pp = np.pad(pp, ((0, by * 8 - ch), (0, bx * 8 - cw)), mode="edge") - 128.0
        blocks = pp.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3)
        S = np.einsum("xu,abxy,yv->abuv", _DCT, blocks, _DCT).reshape(by, bx, 64)      # [vertical, horizontal frequency]
        c["coef"] = np.round(S / c["q"]).astype(np.int64)
    return f


def frame_edges(layout, width, height, seed):
    """Coefficients chosen directly (quantisation tables all 1): DC differences of category 11, AC values of category
    10, ZRL chains ending at zig-zag index 63, all-zero blocks - with every IDCT output kept inside [-512, 511]."""
    rng = np.random.default_rng(seed)
    ones = np.ones(64, np.int64)
    f = _new_frame(width, height, layout, [ones] * 3)
    for ci, c in enumerate(f.comps):
        co = c["coef"]
        by, bx = co.shape[:2]
        kinds = rng.integers(0, 5, (by, bx))
        kinds.flat[:2] = 1
        sign = 1
        for (y, x), k in np.ndenumerate(kinds):
            b = np.zeros(64, np.int64)
            if k == 1:                      # DC +-1016 alternating: differences of 2032 (category 11); AC of category 10
                b[0] = 1016 * sign
                sign = -sign
                b[ZIGZAG[int(rng.integers(1, 3))]] = int(rng.choice([-1, 1]) * rng.integers(512, 640))
            elif k == 2:                    # a chain of ZRLs to the last coefficient
                b[0] = int(rng.integers(-300, 300))
                b[ZIGZAG[63]] = int(rng.choice([-1, 1]) * rng.integers(1, 60))
                if rng.integers(0, 2):
                    b[ZIGZAG[17]] = int(rng.integers(-20, 21))      # a run of exactly 16 zeros first (one ZRL, then r = 0)
            elif k == 3:                    # sparse, mid-size values everywhere
                for z in rng.choice(np.arange(1, 64), int(rng.integers(1, 8)), replace=False):
                    b[ZIGZAG[z]] = int(rng.integers(-40, 41))
                b[0] = int(rng.integers(-600, 600))
            co[y, x] = b                    # k == 0 (and 4: DC 0 after a non-zero DC): an all-zero block
        if ci == 0:
            co.reshape(-1, 64)[:2, 0] = (1016, -1016)
    return f


# ---- Huffman tables ----------------------------------------------------------------------------------------------------
def _codes(bits, vals):
    """(code, length) per symbol (T.81 C.2 canonical codes)."""
    code_of, len_of = np.zeros(256, np.int64), np.zeros(256, np.int64)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code_of[vals[k]], len_of[vals[k]] = code, l
            code += 1
            k += 1
        code <<= 1
    return code_of, len_of


def optimal_table(freq):
    """BITS / HUFFVAL from symbol counts (T.81 K.2: a reserved code point so no code is all ones, lengths limited to 16)."""
    syms = [s for s in range(256) if freq[s] > 0] + [256]
    f = list(freq[:256]) + [1]
    heap = [(int(f[s]), s, [s]) for s in syms]
    heapq.heapify(heap)
    size = {s: 0 for s in syms}
    if len(heap) == 1:
        size[syms[0]] = 1
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            size[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    bits = [0] * 40
    for s in syms:
        bits[size[s]] += 1
    i = 39
    while i > 16:                            # T.81 figure K.3 (Adjust_BITS)
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                             # the reserved code point
    order = sorted((s for s in syms if s != 256), key=lambda s: (size[s], s))
    return bits[1:17], order


def deep_table(freq):
    """A valid table that gives the most frequent symbols codes of 12-16 bits and the rare ones 2-11 bits."""
    syms = sorted((s for s in range(256) if freq[s] > 0), key=lambda s: (-freq[s], s))
    if not syms:
        syms = [0]
    n_rare = min(len(syms) - 1, 10)
    frequent, rare = syms[:len(syms) - n_rare], syms[len(syms) - n_rare:]
    length = {s: 2 + i for i, s in enumerate(rare)}
    for i, s in enumerate(frequent):
        length[s] = 16 - i % 5
    bits = [0] * 16
    for s in syms:
        bits[length[s] - 1] += 1
    return bits, sorted(syms, key=lambda s: (length[s], s))


# ---- entropy coding ----------------------------------------------------------------------------------------------------
def _scan_blocks(f, cs):
    """(component, block row, block column, MCU index) of every block of a scan, in coding order."""
    if len(cs) == 1:
        c = f.comps[cs[0]]
        h, v = f.eff(c)
        bw = -(-(-(-f.width * h // f.hmax)) // 8)
        bh = -(-(-(-f.height * v // f.vmax)) // 8)
        yy, xx = np.divmod(np.arange(bw * bh), bw)
        return np.full(bw * bh, cs[0]), yy, xx, np.arange(bw * bh)
    mx, my = -(-f.width // (8 * f.hmax)), -(-f.height // (8 * f.vmax))
    parts = []
    for ci in cs:
        h, v = f.eff(f.comps[ci])
        for k in range(h * v):
            parts.append((ci, k // h, k % h, h, v))
    n = len(parts)
    mcu = np.repeat(np.arange(mx * my), n)
    slot = np.tile(np.arange(n), mx * my)
    P = np.array(parts)
    comp, oy, ox, h, v = (P[slot, i] for i in range(5))
    return comp, (mcu // mx) * v + oy, (mcu % mx) * h + ox, mcu


def _symbols(f, cs, restart):
    """The scan as events in coding order: (table class 0 DC / 1 AC, component, symbol) for Huffman codes, component -1
    for raw magnitude bits (value, size); plus the restart interval each event belongs to."""
    ev, _, iv, n_iv = _events(f, cs, restart)
    return ev, iv, n_iv


def _events(f, cs, restart):
    """_symbols, and the block (its index in coding order) that each event belongs to"""
    comp, by, bx, mcu = _scan_blocks(f, cs)
    nb = len(comp)
    Z = np.zeros((nb, 64), np.int64)
    for ci in set(comp.tolist()):
        m = comp == ci
        Z[m] = f.comps[ci]["coef"][by[m], bx[m]][:, ZIGZAG]
    interval = mcu // restart if restart else np.zeros(nb, np.int64)
    diff = Z[:, 0].copy()
    for ci in set(comp.tolist()):
        idx = np.nonzero(comp == ci)[0]
        d = Z[idx, 0]
        prev = np.concatenate([[0], d[:-1]])
        first = np.concatenate([[True], interval[idx][1:] != interval[idx][:-1]])
        diff[idx] = np.where(first, d, d - prev)

    def size_of(v):
        a = np.abs(v)
        s = np.zeros_like(a)
        while np.any(a >> s):
            s += (a >> s) > 0
        return s

    def magnitude(v, s):
        return np.where(v >= 0, v, v + (1 << s) - 1)

    keys, cls, ecomp, sym, raw, nbits = [], [], [], [], [], []

    def add(key, c_, comp_, sym_, raw_, nb_):
        keys.append(key); cls.append(c_); ecomp.append(comp_); sym.append(sym_); raw.append(raw_); nbits.append(nb_)

    b = np.arange(nb)
    ds = size_of(diff)
    add(b * 1024 + 0, np.zeros(nb, np.int64), comp, ds, np.zeros(nb, np.int64), np.zeros(nb, np.int64))
    add(b * 1024 + 1, np.zeros(nb, np.int64), np.full(nb, -1), np.zeros(nb, np.int64), magnitude(diff, ds), ds)
    A = Z[:, 1:]
    nzb, nzk = np.nonzero(A)
    nzk = nzk + 1
    same = np.concatenate([[False], nzb[1:] == nzb[:-1]])
    prevk = np.where(same, np.concatenate([[0], nzk[:-1]]), 0)
    run = nzk - prevk - 1
    val = Z[nzb, nzk]
    for j in range(3):                       # ZRL: 16 zeros
        m = run // 16 > j
        add((nzb[m] * 1024 + nzk[m] * 16 + j), np.ones(m.sum(), np.int64), comp[nzb[m]], np.full(m.sum(), 0xF0), np.zeros(m.sum(), np.int64), np.zeros(m.sum(), np.int64))
    s = size_of(val)
    add(nzb * 1024 + nzk * 16 + 4, np.ones(len(nzb), np.int64), comp[nzb], (run % 16) * 16 + s, np.zeros(len(nzb), np.int64), np.zeros(len(nzb), np.int64))
    add(nzb * 1024 + nzk * 16 + 5, np.ones(len(nzb), np.int64), np.full(len(nzb), -1), np.zeros(len(nzb), np.int64), magnitude(val, s), s)
    last = np.zeros(nb, np.int64)
    last[nzb] = nzk                          # (nonzero() is in order: the last write per block is its last coefficient)
    m = last < 63
    add(b[m] * 1024 + 1023, np.ones(m.sum(), np.int64), comp[m], np.zeros(m.sum(), np.int64), np.zeros(m.sum(), np.int64), np.zeros(m.sum(), np.int64))
    key = np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    ev = [np.concatenate(x)[order] for x in (cls, ecomp, sym, raw, nbits)]
    blk = key[order] // 1024
    return ev, blk, interval[blk], int(interval.max()) + 1 if nb else 0


def _pack(codes, lens):
    """bit strings -> bytes, padded with 1 bits, 0xFF stuffed with 0x00."""
    data = _pack_bits(codes, lens)
    ff = np.nonzero(data == 0xFF)[0]
    return np.insert(data, ff + 1, 0).tobytes()


def _pack_bits(codes, lens):
    """bit strings -> a uint8 array, padded with 1 bits, before any stuffing."""
    lens = np.asarray(lens, np.int64)
    codes = np.asarray(codes, np.int64)
    keep = lens > 0
    codes, lens = codes[keep], lens[keep]
    total = int(lens.sum())
    pad = (-total) % 8
    if pad:
        codes = np.append(codes, (1 << pad) - 1)
        lens = np.append(lens, pad)
        total += pad
    if total == 0:
        return np.zeros(0, np.uint8)
    starts = np.cumsum(lens) - lens
    rep = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(total) - starts[rep]
    bits = (codes[rep] >> (lens[rep] - 1 - within)) & 1
    return np.packbits(bits.astype(np.uint8))


def _seg(marker, payload, fill):
    return b"\xff" * fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload if payload is not None else b"\xff" * fill + bytes([0xFF, marker])


def write_jpeg(f, *, sof=0, marker="jfif", scans=None, huff="std", dc_slots=None, ac_slots=None, restart=0, fill=0,
               noise=False, tables="front", seed=0, trace=None):
    """Entropy-code a Frame.

    sof: 0 (baseline) or 1 (extended sequential: 16-bit quantisation tables where a value exceeds 255).
    marker: 'jfif', 'adobe0', 'adobe1' or None.
    scans: list of component-index lists (default: one interleaved scan).
    huff: 'std' (Annex K: luma tables for component 0, chroma for the rest), 'optimal' or 'deep'.
    dc_slots / ac_slots: table slot per component (default 0 for component 0, 1 for the others).
    restart: DRI in MCUs (blocks of a single-component scan); RSTn wrap past RST7.
    fill: number of 0xFF fill bytes in front of every marker after SOI (RSTn included).
    noise: COM and APPn segments between scans, bytes behind EOI.
    tables: 'front' (every DQT / DHT before the frame) or 'scan' (each scan's tables just in front of it: quantisation
    tables appear right before a component's first scan, Huffman slots are redefined per scan when their content changes).
    trace: a list that receives, per scan, what was coded (tests/jpeg_sync_model.py works from it): the _symbols events, the
    length in bits of every event (code or magnitude bits), the event index where each restart interval starts, and the slots;
    also every event's value ("codes": the Huffman code or the magnitude bits) and the block it belongs to ("block": the index in
    the scan's coding order), from which tests/jpeg_encode_cases.py restates the encoder's batch loop.
    """
    n = len(f.comps)
    scans = scans or [list(range(n))]
    dc_slots = dc_slots or (0, 1, 1)[:n]
    ac_slots = ac_slots or (0, 1, 1)[:n]
    rng = np.random.default_rng(seed)
    out = bytearray(b"\xff\xd8")
    if marker == "jfif":
        out += _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", fill)
    elif marker in ("adobe0", "adobe1"):
        out += _seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([int(marker[-1])]), fill)

    def dqt(slot, q):
        wide = int(q.max()) > 255
        assert not wide or sof == 1, "16-bit quantisation tables need SOF1"
        body = bytes([(16 if wide else 0) | slot]) + b"".join(int(v).to_bytes(2 if wide else 1, "big") for v in q[ZIGZAG])
        return _seg(0xDB, body, fill)

    def dht(tc, slot, bits, vals):
        return _seg(0xC4, bytes([tc * 16 + slot]) + bytes(bits) + bytes(vals), fill)

    scan_all = [_events(f, cs, restart) for cs in scans]
    scan_ev = [(ev, iv, n_iv) for ev, _, iv, n_iv in scan_all]
    slots = (dc_slots, ac_slots)

    def table_for(tc, slot, evs):
        """the table a slot holds for the given scans' events"""
        if huff == "std":
            first = min(ci for ci in range(n) if slots[tc][ci] == slot)
            return ((STD_DC_LUMA, STD_AC_LUMA) if first == 0 else (STD_DC_CHROMA, STD_AC_CHROMA))[tc]
        freq = np.zeros(257, np.int64)
        for (cls, comp, sym, _, _), _, _ in evs:
            m = (cls == tc) & (comp >= 0)
            m &= np.isin(comp, [ci for ci in range(n) if slots[tc][ci] == slot])
            np.add.at(freq, sym[m], 1)
        return optimal_table(freq) if huff == "optimal" else deep_table(freq)

    qcur, hcur = {}, {}
    if tables == "front":
        for c in f.comps:
            if c["tq"] in qcur:
                assert np.array_equal(qcur[c["tq"]], c["q"]), "two components need different tables in one slot"
                continue
            qcur[c["tq"]] = c["q"]
            out += dqt(c["tq"], c["q"])
        for tc in (0, 1):
            for slot in sorted(set(slots[tc])):
                hcur[(tc, slot)] = table_for(tc, slot, scan_ev)
                out += dht(tc, slot, *hcur[(tc, slot)])
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, "big"), fill)
    body = bytes([8]) + f.height.to_bytes(2, "big") + f.width.to_bytes(2, "big") + bytes([n])
    for c in f.comps:
        body += bytes([c["id"], c["h"] * 16 + c["v"], c["tq"]])
    out += _seg(0xC0 + sof, body, fill)
    latched = set()
    for si, (cs, (ev, blk, iv, n_iv)) in enumerate(zip(scans, scan_all)):
        if noise and si > 0:
            out += _seg(0xFE, b"between scans %d" % si, fill)
            out += _seg(0xE9, bytes(rng.integers(0, 256, 20, dtype=np.uint8)), fill)
        if tables == "scan":
            for ci in cs:
                c = f.comps[ci]
                if ci in latched:
                    continue
                latched.add(ci)
                if c["tq"] not in qcur or not np.array_equal(qcur[c["tq"]], c["q"]):
                    qcur[c["tq"]] = c["q"]
                    out += dqt(c["tq"], c["q"])
            for tc in (0, 1):
                for slot in sorted({slots[tc][ci] for ci in cs}):
                    t = table_for(tc, slot, [(ev, iv, n_iv)])
                    if hcur.get((tc, slot)) != t:
                        hcur[(tc, slot)] = t
                        out += dht(tc, slot, *t)
        sos = bytes([len(cs)]) + b"".join(bytes([f.comps[ci]["id"], dc_slots[ci] * 16 + ac_slots[ci]]) for ci in cs) + b"\x00\x3f\x00"
        out += _seg(0xDA, sos, fill)
        cls, comp, sym, raw, nbits = ev
        code_tab = {}
        for ci in cs:
            for tc in (0, 1):
                code_tab[(tc, ci)] = _codes(*hcur[(tc, slots[tc][ci])])
        codes, lens = raw.copy(), nbits.copy()
        for (tc, ci), (cd, ln) in code_tab.items():
            m = (cls == tc) & (comp == ci)
            assert np.all(ln[sym[m]] > 0), "symbol without a code"
            codes[m], lens[m] = cd[sym[m]], ln[sym[m]]
        bounds = np.searchsorted(iv, np.arange(n_iv + 1))
        if trace is not None:
            trace.append({"comps": list(cs), "cls": cls, "comp": comp, "sym": sym, "lens": lens.copy(), "bounds": bounds,
                          "dc_slots": tuple(dc_slots), "ac_slots": tuple(ac_slots), "codes": codes.copy(), "block": blk})
        for k in range(n_iv):
            if k:
                out += b"\xff" * fill + bytes([0xFF, 0xD0 + (k - 1) % 8])
            out += _pack(codes[bounds[k]:bounds[k + 1]], lens[bounds[k]:bounds[k + 1]])
    out += b"\xff" * fill + b"\xff\xd9"
    if noise:
        out += b"\x00trailing bytes\xff\xd9"
    return bytes(out)


# ---- float64 reference decoder -----------------------------------------------------------------------------------------
def component_planes(f):
    """dequantise, T.81 A.3.3 IDCT, level shift, round, clamp: one uint8-valued float plane per component (its true size)."""
    planes = []
    for c in f.comps:
        co = c["coef"].astype(np.float64) * c["q"]
        by, bx = co.shape[:2]
        S = co.reshape(by, bx, 8, 8)                     # [v, u]
        s = np.einsum("yv,abvu,xu->abyx", _DCT, S, _DCT)
        p = np.clip(np.round(s + 128.0), 0, 255).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
        h, v = f.eff(c)
        cw, ch = -(-f.width * h // f.hmax), -(-f.height * v // f.vmax)
        planes.append(p[:ch, :cw])
    return planes


def _fancy(p, axis):
    """triangle (3/4, 1/4) doubling along one axis, edges replicated"""
    n = p.shape[axis]
    idx = np.arange(n)
    prev = np.take(p, np.maximum(idx - 1, 0), axis)
    nxt = np.take(p, np.minimum(idx + 1, n - 1), axis)
    even, odd = 0.75 * p + 0.25 * prev, 0.75 * p + 0.25 * nxt
    return np.stack([even, odd], axis + 1).reshape(p.shape[:axis] + (2 * n,) + p.shape[axis + 1:])


def upsample(p, sx, sy, width, height):
    """libjpeg-turbo's rules: h2v1 and h2v2 blend only when the plane is more than 2 samples wide, else replicate;
    h1v2 always blends."""
    if sx == 2 and p.shape[1] <= 2:
        p = np.repeat(p, 2, 1)
        if sy == 2:
            p = np.repeat(p, 2, 0)
    else:
        if sx == 2:
            p = _fancy(p, 1)
        if sy == 2:
            p = _fancy(p, 0)
    return p[:height, :width]


def reference_decode(f):
    """H x W x 3 float64 RGB (unrounded after the colour stage)."""
    planes = component_planes(f)
    if len(planes) == 1:
        return np.repeat(planes[0][..., None], 3, 2)
    full = []
    for c, p in zip(f.comps, planes):
        h, v = f.eff(c)
        full.append(upsample(p, f.hmax // h, f.vmax // v, f.width, f.height))
    if f.colour == "rgb":
        return np.stack(full, -1)
    y, cb, cr = full[0], full[1] - 128.0, full[2] - 128.0
    return np.stack([y + 1.402 * cr, y - 0.344136286 * cb - 0.714136286 * cr, y + 1.772 * cb], -1)


def reference_rgb(f):
    return np.clip(np.round(reference_decode(f)), 0, 255)


# ---- the conformance matrix (tests/test_jpeg_writer.py checks the files, tests/test_gpu_jpeg_conformance.py decodes them) --
WIDTHS = range(1, 18)
HEIGHTS = (1, 2, 3, 7, 8, 9, 15, 16, 17)


def photo(seed, h, w, noise=24):
    """smooth colour + noise: chroma that varies from sample to sample, so every upsampling rule shows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.empty((h, w, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.5, 3.0, 3)
        a[..., c] = 127.5 + 100 * np.sin(fx * xx / max(w, 4) * 6.28 + fy * yy / max(h, 4) * 6.28 + ph * 2)
    a += rng.integers(-noise, noise + 1, a.shape)
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


def gpu_eligible(f, opts):
    """what the GPU Huffman decoder takes (ist_jpeg.cpp): one scan over all components, at most two DC and two AC table
    slots, at most 10 blocks per MCU, at most 2048 restart intervals"""
    n = len(f.comps)
    scans = opts.get("scans") or [list(range(n))]
    if len(scans) != 1 or len(scans[0]) != n:
        return False
    if len(set(opts.get("dc_slots") or (0, 1, 1)[:n])) > 2 or len(set(opts.get("ac_slots") or (0, 1, 1)[:n])) > 2:
        return False
    if sum(f.eff(c)[0] * f.eff(c)[1] for c in f.comps) > 10:
        return False
    ri = opts.get("restart", 0)
    mcus = -(-f.width // (8 * f.hmax)) * -(-f.height // (8 * f.vmax))
    return not ri or -(-mcus // ri) <= 2048


def _case(name, f, **opts):
    marker = opts.pop("marker", "jfif" if f.colour != "rgb" else "adobe0")
    return {"name": name, "data": write_jpeg(f, marker=marker, **opts), "frame": f, "gpu": gpu_eligible(f, opts),
            "width": f.width, "height": f.height}


def size_cases(layout):
    """every width 1-17 x heights {1, 2, 3, 7, 8, 9, 15, 16, 17}; 'rgbids' = RGB named by its component IDs, no marker"""
    out = []
    for w in WIDTHS:
        for h in HEIGHTS:
            seed = 1000 * w + h
            if layout == "rgbids":
                f = frame_from_pixels(photo(seed, h, w), "rgb", 0.6)
                out.append(_case("rgbids_%dx%d" % (w, h), f, marker=None))
            else:
                f = frame_from_pixels(photo(seed, h, w), layout, 0.6)
                out.append(_case("%s_%dx%d" % (layout, w, h), f))
    return out


SIZE_LAYOUTS = ("grey", "grey22", "444", "422", "420", "440", "rgb", "rgbids", "rgb420")
VARIANT_LAYOUTS = ("420", "440", "grey")


def variant_cases(layout):
    """every scan, table, restart, marker-noise and coefficient variant of the writer on one layout"""
    rng_seed = {"420": 1, "440": 2, "grey": 3}[layout]
    W, H = 61, 45
    f = frame_from_pixels(photo(rng_seed, H, W), layout, 0.5)
    n = len(f.comps)
    out = []
    add = lambda name, fr, **o: out.append(_case("%s_%s" % (layout, name), fr, **o))
    add("std", f)
    add("optimal", f, huff="optimal")
    add("deep", f, huff="deep")
    add("deep_restart3", f, huff="deep", restart=3)
    add("slots23", f, huff="optimal", dc_slots=(2, 3, 3)[:n], ac_slots=(3, 2, 2)[:n])
    for ri in (1, 2, 3, 7, 65535):
        add("restart%d" % ri, f, restart=ri)
    add("fill_noise", f, fill=3, noise=True, restart=2)
    add("fill_noise_deep", f, fill=1, noise=True, huff="deep")
    if n == 3:
        add("three_tables", f, huff="optimal", dc_slots=(0, 1, 2), ac_slots=(0, 1, 2))
        add("scans_cr_cb_y", f, scans=[[2], [1], [0]])
        add("scans_y_then_cbcr", f, scans=[[0], [1, 2]], tables="scan", huff="optimal")
        add("scans_restart", f, scans=[[1], [0], [2]], restart=5, fill=1)
        add("scans_restart_mixed", f, scans=[[0], [2, 1]], restart=2, huff="deep", tables="scan")
        add("scans_noise_redefined", f, scans=[[0], [1], [2]], tables="scan", huff="optimal", dc_slots=(0, 0, 0),
            ac_slots=(0, 0, 0), noise=True, fill=2)
        # one quantisation slot for all three components, redefined in front of the chroma scans
        g = frame_from_pixels(photo(rng_seed + 10, H, W), layout, 0.5, tq=(0, 0, 0),
                              qtabs=[quant_table(0, 0.5), quant_table(1, 0.9), quant_table(1, 0.3)])
        add("dqt_redefined", g, scans=[[0], [1], [2]], tables="scan")
        add("dqt_late", frame_from_pixels(photo(rng_seed + 11, H, W), layout, 0.7), scans=[[0], [2, 1]], tables="scan")
    else:
        add("scan_tables", f, tables="scan", huff="optimal", restart=4)
    wide = frame_from_pixels(photo(rng_seed + 20, H, W), layout, qtabs=[quant_table(0, 6.0), quant_table(1, 4.0), quant_table(1, 5.0)][:n],
                             tq=(0, 1, 2)[:n])            # 16-bit tables (values up to 726), a third slot
    add("sof1_q16", wide, sof=1, huff="optimal")
    e = frame_edges(layout, W, H, rng_seed)
    add("edges", e)
    add("edges_deep_restart", e, huff="deep", restart=7)
    add("edges_optimal", frame_edges(layout, 40, 24, rng_seed + 1), huff="optimal")
    if n == 3:
        add("edges_scans", e, scans=[[2], [0], [1]], huff="deep", tables="scan")
    return out


def large_cases():
    out = []
    for (w, h), layout, seed in (((1000, 700), "420", 7), ((4000, 64), "420", 8), ((1000, 700), "440", 9), ((4000, 64), "grey", 10)):
        out.append(_case("%s_%dx%d" % (layout, w, h), frame_from_pixels(photo(seed, h, w, 8), layout, 0.5), huff="optimal"))
    return out


# layouts the decoder refuses (IST_E_UNSUPPORTED): all components 2x2, chroma larger than 1x1, 4:1:1
REFUSED = {
    "all_2x2": ("ycc", ((2, 2), (2, 2), (2, 2))),
    "cb_2x1": ("ycc", ((2, 2), (2, 1), (1, 1))),
    "411": ("ycc", ((4, 1), (1, 1), (1, 1))),
}


def refused_cases():
    return [_case(name, frame_from_pixels(photo(50 + k, 20, 36), layout, 0.5))
            for k, (name, layout) in enumerate(REFUSED.items())]


def pillow_keep_rgb_cases():
    """RGB files as Pillow writes them (keep_rgb=True: an Adobe marker with transform 0)"""
    import io
    from PIL import Image
    out = []
    for k, (w, h) in enumerate(((1, 1), (3, 9), (17, 16), (64, 40), (33, 7))):
        b = io.BytesIO()
        Image.fromarray(photo(70 + k, h, w)).save(b, "JPEG", quality=85, keep_rgb=True, subsampling=0)
        out.append({"name": "pillow_rgb_%dx%d" % (w, h), "data": b.getvalue(), "frame": None, "gpu": True, "width": w, "height": h})
    return out
