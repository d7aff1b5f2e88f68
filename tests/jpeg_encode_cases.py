"""The inputs of the JPEG entropy coder's seam tests (tests/test_jpeg_encode_cases.py judges them on the CPU,
tests/test_gpu_jpeg_encode_regimes.py encodes them on the GPU): cases(layout), named (name, H x W x 4 uint8 canvas, quality) triples,
and regimes(a, quality, layout, tables), the set of things that the encoder's loops meet on the contract's stream of a canvas.

Every canvas is ONE MCU row high (8 rows for 4:4:4, 16 for 4:2:0): an MCU row is a restart interval, the entropy kernel codes the
intervals independently of each other, and so does the histogram.  What matters is the number of blocks in the interval and what the
bits do where the kernel's loops have an edge.

regimes() restates the batch loop of jpeg_entropy (ist_jpeg_encode.hip) in integers, once:
    an interval is coded in batches of 256 blocks in coding order; a batch starts with the `carry` bits (0..7) that the batches
    before it left of their last byte; total = carry + the bits of its blocks; only the last batch is padded to a byte with 1 bits;
    nb = (total + pad) >> 3 whole bytes are stuffed and written, thread t owning bytes [t span, t span + span) of them,
    span = (((nb + 255) >> 8) + 3) & ~3; carry = (total + pad) & 7
and the part loop of jpeg_histogram: parts of 128 blocks, a wave taking 8 blocks per step.  The bits of every block and the bytes
before stuffing come from tests/jpeg_writer.py (write_jpeg's trace and _pack_bits): no code is derived here.

Three things that the kernels guard against cannot be reached from a canvas and are no regimes:
  - a batch without a whole byte: a block is at least 2 bits of DC and 2 of EOB, so 256 blocks are at least 512 bits;
  - the AC clamp min(|k|, 1023): samples are -128 .. 127, the largest orthonormal AC coefficient of such a block is below
    8 x 128 x (0.5 x 2.563)^2 / 1.0 ~ 928 at a quantiser of 1 (2.563 = the sum of |cos| of the odd frequencies' basis row), under 1023;
  - the DC clamp +-2047: a DC coefficient is within 8 x (-128 .. 127) = -1024 .. 1016, quantised by 1 at the least, so two of them
    differ by 2040 at the most.
A last batch of ONE block and a single batch of 255 blocks exist in 4:4:4 only: an interval of m MCUs has 3 m blocks there and 6 m in
4:2:0, and 6 m is even, so it is never 1 or 255 modulo 256; for the same reason it is never 1 modulo 128, and the histogram's part of
one block is a 4:4:4 regime too (ONLY_444).
"""
import functools
import hashlib

import numpy as np

from tests import jpeg_encode_reference as R
from tests import jpeg_writer as JW
from tests.test_gpu_jpeg_encode import checker, noise, photo

BATCH, PART, STEP = 256, 128, 8          # kBatch, kHistBlocks, kHistStep of ist_jpeg_encode.hip

ENTROPY_REGIMES = (
    "several batches", "partial byte carried", "batch ends on a byte", "0xFF completed from carried bits",
    "0xFF last whole byte of a batch", "padded last byte is 0xFF", "unpadded last byte is 0xFF", "interval ends without padding",
    "full last batch", "two-block last batch", "one-block last batch", "single batch of 255 blocks", "span 4", "span 8",
    "span above 8", "idle threads in the stuffing", "0xFF at the start of a thread's span", "0xFF at the end of a thread's span")
HISTOGRAM_REGIMES = (
    "part of exactly 128 blocks", "part of one block", "part whose last wave step is partial",
    "DC predictor read across a part edge", "run of 16..31", "run of 32..47", "run of 48..62", "coefficient 63 set (no EOB)",
    "block of zeros only", "DC size 11")
ALL_REGIMES = frozenset(ENTROPY_REGIMES + HISTOGRAM_REGIMES)
ONLY_444 = frozenset(("one-block last batch", "single batch of 255 blocks", "part of one block"))

_coded = {}


def coded(a, quality, layout, tables):
    """(the contract's file of a canvas, the trace of its scan); tables: 'std' (tests/jpeg_encode_reference.py encode) or 'optimal'
    (the file of optimize=True).  Computed once per process."""
    key = (a.shape, hashlib.sha1(np.ascontiguousarray(a)).digest(), quality, layout, tables)
    if key not in _coded:
        trace = []
        data = JW.write_jpeg(R.frame(a, quality, layout), sof=0, marker="jfif", huff=tables, restart=R.mcus_per_row(a.shape[1], layout),
                             trace=trace)
        _coded[key] = (data, trace[0])
    return _coded[key]


def reference(a, quality, layout, tables):
    return coded(a, quality, layout, tables)[0]


def counts(a, quality, layout):
    """the 544 symbol counts of a canvas as jpeg_histogram leaves them: per table slot (luma, then chroma) 16 DC sizes, then 256 AC symbols"""
    tr = coded(a, quality, layout, "optimal")[1]
    m = tr["comp"] >= 0
    at = (tr["comp"][m] > 0) * (16 + 256) + tr["cls"][m] * 16 + tr["sym"][m]
    return np.bincount(at, minlength=2 * (16 + 256)).astype(np.int64)


def regimes(a, quality, layout, tables):
    """the names out of ALL_REGIMES that the stream of a one-interval canvas reaches"""
    assert a.shape[0] <= (16 if layout == "420" else 8), "one MCU row: one interval"
    tr = coded(a, quality, layout, tables)[1]
    bpm = 6 if layout == "420" else 3
    blocks = R.mcus_per_row(a.shape[1], layout) * bpm
    block, lens, cls, comp, sym = tr["block"], tr["lens"], tr["cls"], tr["comp"], tr["sym"]
    bits = np.bincount(block, weights=lens, minlength=blocks).astype(np.int64)
    assert len(bits) == blocks
    stream = JW._pack_bits(tr["codes"], lens)                # the interval before stuffing, padded
    out = set()
    hit = lambda name, cond: out.add(name) if cond else None

    # ---- jpeg_entropy: the batch loop ----
    carry, done = 0, 0                                         # bits carried into the batch; whole bytes written by the batches before
    for base in range(0, blocks, BATCH):
        last = base + BATCH >= blocks
        total = carry + int(bits[base:base + BATCH].sum())
        pad = (-total) % 8 if last else 0
        nb = (total + pad) >> 3
        span = (((nb + 255) >> 8) + 3) & ~3
        b = stream[done:done + nb]
        assert len(b) == nb and nb >= 1
        ff = np.nonzero(b == 0xFF)[0]
        hit("several batches", base > 0)
        hit("partial byte carried", not last and total & 7)
        hit("batch ends on a byte", not last and not total & 7)
        hit("0xFF completed from carried bits", carry and b[0] == 0xFF)
        hit("0xFF last whole byte of a batch", not last and b[-1] == 0xFF)
        hit("padded last byte is 0xFF", last and pad and b[-1] == 0xFF)
        hit("unpadded last byte is 0xFF", last and not pad and b[-1] == 0xFF)
        hit("interval ends without padding", last and not pad)
        hit("full last batch", last and blocks - base == BATCH)
        hit("two-block last batch", last and blocks - base == 2)
        hit("one-block last batch", last and blocks - base == 1)
        hit("single batch of 255 blocks", blocks == 255)
        hit("span 4", span == 4)
        hit("span 8", span == 8)
        hit("span above 8", span > 8)
        hit("idle threads in the stuffing", (BATCH - 1) * span >= nb)
        # a thread other than the first starts on a 0xFF; a thread that another follows ends on one (the next one's place counts the 0x00)
        hit("0xFF at the start of a thread's span", np.any((ff % span == 0) & (ff > 0)))
        hit("0xFF at the end of a thread's span", np.any((ff % span == span - 1) & (ff < nb - 1)))
        carry, done = (total + pad) & 7, done + nb
    assert carry == 0 and done == len(stream)

    # ---- jpeg_histogram: parts, and what count_block meets ----
    back = np.full(blocks, 3)
    if bpm == 6:
        pos = np.arange(blocks) % 6
        back = np.where(pos == 0, 3, np.where(pos < 4, 1, 6))
    j = np.arange(blocks)
    for p0 in range(0, blocks, PART):
        n = min(PART, blocks - p0)
        hit("part of exactly 128 blocks", n == PART)
        hit("part of one block", n == 1)
        hit("part whose last wave step is partial", n % STEP)
    hit("DC predictor read across a part edge", np.any((j >= back) & ((j - back) // PART != j // PART)))
    ac = (cls == 1) & (comp >= 0)
    zrl = ac & (sym == 0xF0)
    before = np.cumsum(zrl)
    ends = np.nonzero(ac & ~zrl & (sym != 0))[0]              # the symbol of a non-zero coefficient: its run is 16 per ZRL in front of it
    zrls = np.diff(np.concatenate([[0], before[ends]]))
    run = 16 * zrls + (sym[ends] >> 4)
    hit("run of 16..31", np.any((run >= 16) & (run < 32)))
    hit("run of 32..47", np.any((run >= 32) & (run < 48)))
    hit("run of 48..62", np.any(run >= 48))
    assert run.max(initial=0) <= 62
    eob = np.bincount(block[ac & (sym == 0)], minlength=blocks)
    hit("coefficient 63 set (no EOB)", np.any(eob == 0))
    dc_size = sym[(cls == 0) & (comp >= 0)]
    assert len(dc_size) == blocks
    hit("block of zeros only", np.any((dc_size == 0) & (np.bincount(block[ac], minlength=blocks) == 1) & (eob == 1)))
    hit("DC size 11", np.any(dc_size == 11))
    assert out <= ALL_REGIMES
    return frozenset(out)


# ---- contents -----------------------------------------------------------------------------------------------------------------
def _corner():
    """8 x 8 of +-1: the sign of the basis function of the last coefficient (zig-zag 63, vertical and horizontal frequency 7)"""
    s = np.sign(R.T[7])
    return np.outer(s, s)


def directed(base, layout, kind, amp, seed):
    """`base` with its last MCU replaced by 128 + amp x the corner pattern + noise of +-3 (seed).  At quality 100 an amplitude of 39
    quantises coefficient 63 to 255: eight 1 bits of magnitude, and no EOB behind them.
    kind 'seam': a grey pattern in the luma block in front of the first batch seam (block 255 of a 688 wide canvas: Y of MCU 85 in
    4:4:4, Y3 of MCU 42 in 4:2:0); kind 'end': R against G and B, which is a pattern of Cr, the interval's last block (constant over
    2 x 2 pixels in 4:2:0, so that it survives the chroma mean).  The noise is re-drawn until the bits in front align the eight ones
    with a byte: the seeds below were found by tools/search_jpeg_encode_cases.py."""
    a = base.copy()
    rng = np.random.default_rng(seed)
    s = _corner()
    if kind == "end" and layout == "420":
        s = np.kron(s, np.ones((2, 2), np.int64))
    m = s.shape[0]
    px = np.empty((m, m, 3), np.int64)
    px[...] = 128 + amp * s[..., None]
    if kind == "end":
        px[..., 1:] = 128 - amp * s[..., None]
    px += rng.integers(-3, 4, px.shape)
    a[a.shape[0] - m:, a.shape[1] - m:, :3] = px
    return a


def constant(w, h, v=200):
    return np.full((h, w, 4), v, np.uint8)


def sparse(w, h, seed):
    """grey blocks of one to three basis functions each, at random zig-zag positions and 1.3 times the quality 50 quantiser, so that
    they quantise to +-1 there with nothing between them: runs of every length up to 62 in the luma blocks, and all-zero chroma"""
    rng = np.random.default_rng(seed)
    q = R.quant_tables(50)[0]
    v = np.full((h, w), 128.0)
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            S = np.zeros(64)
            for z in rng.choice(np.arange(1, 64), int(rng.integers(1, 4)), replace=False):
                S[JW.ZIGZAG[z]] = 1.3 * q[JW.ZIGZAG[z]] * rng.choice((-1, 1))
            v[y:y + 8, x:x + 8] += (JW._DCT @ S.reshape(8, 8) @ JW._DCT.T)[:h - y, :w - x]
    v = np.clip(np.round(v), 0, 255).astype(np.uint8)
    return np.stack([v, v, v, np.full_like(v, 255)], -1)


# (layout, tables the search was made for, kind, amplitude, seed of the +-3 noise): tools/search_jpeg_encode_cases.py
DIRECTED = (
    ("444", "std", "seam", 39, 57),          # input 58 of the search
    ("444", "optimal", "seam", 39, 34),      # input 35
    ("444", "std", "end", 39, 29),           # input 30
    ("444", "optimal", "end", 39, 2),        # input 3
    ("420", "std", "seam", 39, 65),          # input 66
    ("420", "optimal", "seam", 39, 14),      # input 15
    ("420", "std", "end", 39, 7),            # input 8
    ("420", "optimal", "end", 39, 34),       # input 35
)

# seeds of 688 wide noise rows at quality 100 which between them reach 'batch ends on a byte', '0xFF completed from carried bits' and
# 'padded last byte is 0xFF' with either kind of table (the same search: the first rows that add one of the six)
NOISE_688 = {"444": (0, 1, 5, 10, 14), "420": (0, 1, 66, 225)}


@functools.lru_cache(maxsize=None)
def cases(layout):
    """(name, canvas, quality) of every case of a layout, rebuilt from seeds (once per process: nobody writes to a canvas)"""
    h = 16 if layout == "420" else 8
    out = [("noise 2048", noise(2048, h, seed=11), 100)]
    out += [("noise 688 seed %d" % s, noise(688, h, seed=s), 100) for s in NOISE_688[layout]]
    if layout == "444":
        out += [("noise 1365", noise(1365, h, seed=12), 100), ("noise 677", noise(677, h, seed=13), 100), ("photo 341", photo(341, h), 50)]
    out += [("photo 2048 quality 1", photo(2048, h), 1), ("photo 2048 quality 50", photo(2048, h), 50), ("photo 688 quality 50", photo(688, h), 50),
            ("constant 688", constant(688, h), 90), ("checker 688", checker(688, h), 100), ("sparse 688", sparse(688, h, 31), 50)]
    base = noise(688, h, seed=21)
    out += [("directed %s for %s tables" % (kind, tables), directed(base, layout, kind, amp, seed), 100)
            for lay, tables, kind, amp, seed in DIRECTED if lay == layout]
    return out
