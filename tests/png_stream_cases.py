"""The inputs of tests/test_gpu_png_stream.py, built without the GPU so that tests/test_png_deflate_reference.py can judge them
first: every group is a list of (name, HxWx4 uint8 canvas), and report(name, a) is the CPU reference's encode of it, computed
once per process."""
import functools

import numpy as np

from tests import png_deflate_reference as R

_reports = {}


def report(name, a):
    if name not in _reports:
        _reports[name] = R.encode(a)
    return _reports[name]


def row_image(res, fill=None):
    """a one-row canvas whose filtered stream is the filter byte and `res` (h = 1: Paeth = Sub); res is padded to whole pixels
    with `fill` (default: its first byte)"""
    res = np.asarray(res).astype(np.uint8)
    res = np.concatenate([res, np.full((-len(res)) % 4, res[0] if fill is None else fill, np.uint8)])
    return np.ascontiguousarray(np.cumsum(res.reshape(-1, 4).astype(np.int64), axis=0).astype(np.uint8)[None, :, :]).copy()


def below_zero_rows(res, rows):
    """the same residual row as the LAST row of a canvas whose other rows are zero, `rows` rows in all: with zeros above, Paeth
    predicts from the left, so the last row filters to `res` again"""
    one = row_image(res)
    a = np.zeros((rows, one.shape[1], 4), np.uint8)
    a[-1] = one[0]
    return a


def photo_like(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 90 * np.sin(xx / 37.0 + yy / 91.0), 128 + 80 * np.cos(xx / 53.0 - yy / 29.0), 100 + 0.03 * xx + 0.05 * yy, np.full((h, w), 255.0)], -1)
    base[..., :3] += rng.normal(0, 2.0, (h, w, 3))
    return base.clip(0, 255).astype(np.uint8)


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def flat_with_lines(seed, h, w):
    rng = np.random.default_rng(seed)
    a = np.full((h, w, 4), 255, np.uint8)
    for _ in range(max(2, h // 6)):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, max(1, w - 40)))
        a[y:y + 2, x:x + int(rng.integers(5, 40)), :3] = rng.integers(0, 80, 3, dtype=np.uint8)
    return a


# ---- grid: the smallest shapes that reach each form of the chunk grid ----------------------------------------------------------
GRID_SHAPES = ((1, 1), (3, 5), (64, 33), (257, 19), (2047, 3), (2048, 3), (4095, 2), (4096, 2), (4097, 2), (8191, 2))      # (w, h)


@functools.lru_cache(None)
def grid_cases():
    out = [("grid photo %dx%d" % (w, h), photo_like(1000 + w, h, w)) for w, h in GRID_SHAPES]
    out += [("grid noise %dx%d" % (w, h), noise(1100 + w, h, w)) for w, h in ((64, 33), (4097, 2))]
    out += [("grid flat %dx%d" % (w, h), flat_with_lines(1200 + w, h, w)) for w, h in ((257, 19), (2048, 3), (4096, 2), (8191, 2))]
    return out


# ---- runs: chosen residuals in one row -----------------------------------------------------------------------------------------
FILL = (17, 34, 51)             # filler that never repeats; run bytes are none of these


class Row:
    """residual bytes behind the filter byte, addressed by their index in the CHUNK (the filter byte is index 0)"""

    def __init__(self):
        self.b = [4]

    def fill_to(self, at):
        """non-repeating filler up to chunk index `at` (at least one byte, so that two runs never touch)"""
        assert at > len(self.b)
        while len(self.b) < at:
            self.b.append(FILL[len(self.b) % 3])
        return self

    def run(self, value, n):
        assert value not in FILL and self.b[-1] != value
        self.b += [value] * n
        return self

    def image(self):
        if (len(self.b) - 1) % 4:
            self.fill_to(len(self.b) + (-(len(self.b) - 1)) % 4)
        return row_image(self.b[1:])


def _runs_at_offset(o):
    """every run length 1..70, each starting at a chunk index that is o modulo 8"""
    r = Row()
    for n in range(1, 71):
        at = len(r.b) + 1
        at += (o - at) % 8
        r.fill_to(at).run(200 if n % 2 else 90, n)
    return r.fill_to(len(r.b) + 1).image()


def _runs_through_boundaries():
    """runs that start d bytes before a span boundary and go e bytes beyond it: both parts restart"""
    r, span = Row(), 1
    for d in (1, 2, 3, 4, 5, 9):
        for e in (1, 2, 3, 4, 5, 70):
            r.fill_to(64 * span - d).run(200, d + e)
            span += 1 + (e + 63) // 64
    return r.fill_to(len(r.b) + 1).image()


def _threes_and_fours():
    r = Row()
    for k in range(40):
        r.fill_to(len(r.b) + 1 + k % 3).run(200, 3 + k % 2)
    return r.fill_to(len(r.b) + 2).image()


def _ragged_end(tail, value=9, through=False):
    """three full spans of zeros, then a ragged span of `tail` bytes that is one run to the chunk's last byte (through: the run
    starts 5 bytes before the boundary)"""
    assert (191 + tail) % 4 == 0
    res = [0] * (191 - (5 if through else 0)) + [value] * (tail + (5 if through else 0))
    return row_image(res)


def _back_to_back():
    r = Row()
    for a, b in ((10, 10), (4, 4), (3, 5), (5, 3), (4, 63), (30, 2)):
        r.fill_to(64 * ((len(r.b) + 63) // 64) + 3).run(200, a).run(90, b)
    return r.fill_to(len(r.b) + 1).image()


def _every_match_length():
    """span m - 2 starts with a run of m + 1 bytes, m = 3 .. 63: every match length, so every length symbol (257 .. 276) and every
    extra-bit value the encoder can send"""
    r = Row()
    for m in range(3, 64):
        r.fill_to(64 * (m - 2)).run(200 if m % 2 else 90, m + 1)
    return r.fill_to(len(r.b) + 3).image()


@functools.lru_cache(None)
def runs_cases():
    out = [("runs 1..70 at offset %d" % o, _runs_at_offset(o)) for o in range(8)]
    out.append(("runs through span boundaries", _runs_through_boundaries()))
    out.append(("all-zero 64 px row", np.zeros((1, 64, 4), np.uint8)))
    out.append(("runs of 3 and of 4", _threes_and_fours()))
    out += [("run to the last byte, ragged span of %d" % t, _ragged_end(t)) for t in (1, 5, 9, 33, 61)]
    out.append(("run through the last boundary to the last byte", _ragged_end(9, through=True)))
    out.append(("two runs back to back", _back_to_back()))
    out.append(("every match length", _every_match_length()))
    return out


# ---- the stored / Huffman boundary ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def boundary_rows(draws=3300, seed=20):
    """(residual rows whose Huffman form is exactly as long as the stored one, rows whose Huffman form is one byte shorter), found
    by a seeded search with the reference: one-row images of 40..110 pixels, residuals drawn from 3..32 values"""
    rng = np.random.default_rng(seed)
    ties, wins = [], []
    for _ in range(draws):
        px, nv = int(rng.integers(40, 111)), int(rng.integers(3, 33))
        res = rng.choice(rng.permutation(256)[:nv], 4 * px).astype(np.uint8)
        _, length, _, hsize, ssize = R.chunk_form(np.concatenate([[4], res]).astype(np.uint8))
        if length is None:
            continue
        if hsize == ssize:
            ties.append(res)
        elif hsize == ssize - 1:
            wins.append(res)
    return ties, wins


@functools.lru_cache(None)
def boundary_cases():
    ties, wins = boundary_rows()
    out = []
    for kind, rows in (("tie", ties), ("one byte smaller", wins)):
        for k, res in enumerate(rows[:10]):
            out.append(("boundary %s %d, chunk 0" % (kind, k), row_image(res)))
            rpc = R.CH // (len(res) + 1)
            out.append(("boundary %s %d, chunk 1" % (kind, k), below_zero_rows(res, rpc + 1)))
    return out


# ---- pads: what the other groups leave out of 0..15 ----------------------------------------------------------------------------
@functools.lru_cache(None)
def pad_cases():
    """one-row canvases of a few residual values, the first found for every pad count (seeded)"""
    rng = np.random.default_rng(31)
    found = {}
    for _ in range(400):
        if len(found) == 16:
            break
        px = int(rng.integers(100, 200))
        a = row_image(rng.choice(np.array([0, 0, 0, 1, 255, 7], np.uint8), 4 * px))
        pads = R.encode(a).chunks[0].pads
        found.setdefault(pads, a)
    return [("pads %d" % p, a) for p, a in sorted(found.items())]


# ---- the code rule -------------------------------------------------------------------------------------------------------------
def adversarial_residuals():
    """the histograms of test_compressed_png_codes_complete_on_adversarial_histograms (tests/test_gpu_png.py), same seed and order"""
    rng = np.random.default_rng(77)
    cases = []
    cases.append(np.where(np.arange(16000) == 7777, 9, 200))                                   # 15999 : 1
    cases.append(np.repeat(np.arange(14) * 3 + 1, 2 ** np.arange(14))[:16000])                 # counts 1, 2, 4, ... 8192
    cases.append(np.concatenate([np.full(15000, 33), np.arange(250)]))                         # one dominant + 250 singletons
    cases.append(np.arange(256).repeat(2))                                                     # every literal twice
    cases.append(rng.choice(np.array([5, 6, 7], np.uint8), 12000))                             # three values, equal
    cases.append(np.concatenate([np.full(3, 1), np.full(3, 2), np.full(16000, 3)]))           # two rare, one common
    for k in range(6):                                                                          # random power-law shapes
        ns = int(rng.integers(2, 256))
        c = np.maximum(1, (2.0 ** rng.uniform(0, 12, ns)).astype(int))
        c = (c * min(1.0, 15000 / c.sum())).astype(int).clip(1)
        cases.append(np.repeat(rng.permutation(256)[:ns], c))
    out = []
    for res in cases:
        res = np.asarray(res).copy()
        rng.shuffle(res)
        out.append(res)
    return out


def fibonacci_residuals():
    """test_compressed_png_code_longer_than_15_bits_is_limited (tests/test_gpu_png.py)"""
    fib = [1, 1]
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    res = np.repeat(np.arange(19) * 7 + 20, fib).astype(np.uint8)
    np.random.default_rng(11).shuffle(res)
    return res


def equal_counts_residuals():
    """40 values 100 times each: one length class of 40 symbols of which the first round shortens some - which ones is the
    order inside a class"""
    res = np.repeat(np.arange(40) * 5 + 3, 100).astype(np.uint8)
    np.random.default_rng(12).shuffle(res)
    return res


@functools.lru_cache(None)
def most_rounds_residuals(trials=1500, seed=5):
    """the row, of a short seeded search, on whose chunk the rule takes the most rounds.  Rounds come with few symbols of very
    unequal counts (many symbols leave little slack: one round), so the rows are segments of a few values in a few lengths -
    literals and matches, like flat content."""
    rng = np.random.default_rng(seed)
    best, best_rounds = None, -1
    for _ in range(trials):
        nv = int(rng.integers(2, 8))
        vals = rng.permutation(256)[:nv]
        lens = rng.choice(np.array([1, 2, 3, 5, 9, 17, 40, 64, 150, 700]), int(rng.integers(1, 5)))
        p = 2.0 ** rng.uniform(0, 10, nv)
        segs = int(rng.integers(5, 300))
        res = np.repeat(rng.choice(vals, segs, p=p / p.sum()), rng.choice(lens, segs))[:16000]
        res = np.concatenate([res, np.full(-len(res) % 4, res[-1])]).astype(np.uint8)
        _, length, rounds, hsize, ssize = R.chunk_form(np.concatenate([[4], res]).astype(np.uint8))
        if length is not None and hsize < ssize and rounds > best_rounds:
            best, best_rounds = res, rounds
    return best


@functools.lru_cache(None)
def code_cases():
    out = [("adversarial histogram %d" % k, row_image(res)) for k, res in enumerate(adversarial_residuals())]
    out.append(("fibonacci counts", row_image(fibonacci_residuals(), fill=20)))
    out.append(("many equal counts", row_image(equal_counts_residuals())))
    out.append(("most rounds", row_image(most_rounds_residuals())))
    return out


# ---- several slabs on the host path --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def slab_case():
    """4096 x 400: two pieces per row, 800 chunks - slabs of 768 and 32 on the host path; flat with lines and a band of noise rows"""
    h, w = 400, 4096
    a = np.full((h, w, 4), 255, np.uint8)
    a[::37, 100:900, :3] = 30
    a[5::53, 3000:, :3] = (40, 120, 200)
    a[380:383] = noise(7, 3, w)                                     # (chunks 760..765 in the first slab ...)
    a[390:392] = noise(8, 2, w)                                     # (... and 780..783 in the second)
    return "slabs 4096x400", a


@functools.lru_cache(None)
def limit_case():
    """17 chunks of about 7 KB each: more than 65536 bytes of stream, every chunk larger than the smallest IDAT limit (4096)"""
    return "photo 640x100", photo_like(9, 100, 640)


def all_cases():
    return grid_cases() + runs_cases() + boundary_cases() + pad_cases() + code_cases() + [slab_case(), limit_case()]


# ---- the regimes the inputs were built for, asserted on the reference's report -------------------------------------------------
GRID_CHUNK_BYTES = {(1, 1): [5], (3, 5): [65], (64, 33): [33 * 257], (257, 19): [15 * 1029, 4 * 1029], (2047, 3): [2 * 8189, 8189],
                    (2048, 3): [8193] * 3, (4095, 2): [16381] * 2, (4096, 2): [16381, 4] * 2, (4097, 2): [16381, 8] * 2,
                    (8191, 2): [16381, 16380, 4] * 2}


def check_grid_regimes():
    for name, a in grid_cases():
        h, w = a.shape[:2]
        assert [len(c.data) for c in report(name, a).chunks] == GRID_CHUNK_BYTES[(w, h)], name
    forms = {c.form for name, a in grid_cases() for c in report(name, a).chunks}
    assert forms == {"huff", "stored"}


def check_runs_regimes():
    reps = {name: report(name, a) for name, a in runs_cases()}
    for name, rep in reps.items():
        assert [c.form for c in rep.chunks] == ["huff"], name            # (a stored chunk would hide its tokens)
    zero = reps["all-zero 64 px row"].chunks[0].tokens
    assert R.format_tokens(zero) == "L4 L0 M62 L0 M63 L0 M63 L0 M63 L0"
    sent = [int(t) - R.MATCH for t in reps["every match length"].chunks[0].tokens if t >= R.MATCH]
    assert sent == list(range(3, 64))
    assert {R.LENGTH[n][0] for n in sent} == set(range(257, 277))         # 277 and up are matches of 67 bytes and more: never sent
    assert {eb: any(R.LENGTH[n][1] == eb and R.LENGTH[n][2] for n in sent) for eb in (1, 2, 3)} == {1: True, 2: True, 3: True}
    assert max(R.LENGTH[n][1] for n in sent) == 3
    for t in (5, 9, 33, 61):                                              # the last token is the match that ends with the chunk
        assert int(reps["run to the last byte, ragged span of %d" % t].chunks[0].tokens[-1]) == R.MATCH + t - 1
    tail = R.format_tokens(reps["run through the last boundary to the last byte"].chunks[0].tokens[-4:])
    assert tail == "L9 M4 L9 M8", tail


def check_boundary_regimes():
    ties, wins = boundary_rows()
    assert len(ties) >= 3 and len(wins) >= 3, (len(ties), len(wins))
    for name, a in boundary_cases():
        c = report(name, a).chunks[-1]
        assert len(report(name, a).chunks) == (1 if name.endswith("chunk 0") else 2), name
        if "tie" in name:
            assert c.form == "stored" and c.huff_size == c.stored_size, name
        else:
            assert c.form == "huff" and c.huff_size == c.stored_size - 1, name


def check_pad_regimes():
    seen = {c.pads for name, a in all_cases() for c in report(name, a).chunks}
    assert seen == set(range(16)), sorted(seen)


def check_code_regimes():
    reps = {name: report(name, a).chunks for name, a in code_cases()}
    assert all(len(c) == 1 for c in reps.values())
    assert reps["many equal counts"][0].form == "huff" and reps["fibonacci counts"][0].form == "huff"
    most = reps["most rounds"][0]
    assert most.form == "huff" and most.rounds >= 5, most.rounds
    assert sum(c[0].form == "huff" for c in reps.values()) >= 12


def check_slab_regimes():
    name, a = slab_case()
    chunks = report(name, a).chunks
    assert len(chunks) == 800 and R.host_slabs(800) == [768, 32]
    assert {c.form for c in chunks[:768]} == {"huff", "stored"} and {c.form for c in chunks[768:]} == {"huff", "stored"}
