"""The inputs of the PNG window-match tests (tests/test_png_match_reference.py judges them on the CPU, tests/test_gpu_png_match.py and
tests/test_node_png_match.py run them on the GPU): (name, HxWx4 uint8 canvas) pairs, and report(name, a, bpp, adaptive), the CPU
reference's window encode of a canvas (tests/png_match_reference.py), computed once per process."""
import functools

import numpy as np

from tests import png_match_reference as M
from tests import png_stream_cases as C

_reports = {}


def report(name, a, bpp=4, adaptive=False):
    key = (name, bpp, adaptive)
    if key not in _reports:
        _reports[key] = M.encode_window(a, bpp, adaptive)
    return _reports[key]


# ---- contents -----------------------------------------------------------------------------------------------------------------
def text_like(seed, h, w, vocab=9):
    """dark glyphs of 5 x 7 pixels with grey edges out of a small vocabulary on white, in lines 9 pixels apart: after the filter the
    same short residual patterns return at a distance - what rendered text does"""
    rng = np.random.default_rng(seed)
    glyphs = rng.choice(np.array([255, 255, 20, 20, 130], np.uint8), (vocab, 7, 5))
    a = np.full((h, w, 4), 255, np.uint8)
    for y in range(1, h, 9):
        for x in range(1, w - 5, 6):
            g = glyphs[int(rng.integers(0, vocab))][:max(0, min(7, h - y))]
            if rng.integers(0, 6):
                a[y:y + g.shape[0], x:x + 5, :3] = g[:, :, None]
    return a


def rendered_text(seed, w, h, vocab):
    """white with dark text in PIL's default font: lines of 14 words, random letter strings out of a vocabulary of `vocab` words"""
    from PIL import Image, ImageDraw, ImageFont
    rng = np.random.RandomState(seed)
    words = ["".join(chr(97 + c) for c in rng.randint(0, 26, rng.randint(2, 9))) for _ in range(vocab)]
    im = Image.new("RGBA", (w, h), (255, 255, 255, 255))
    draw, font = ImageDraw.Draw(im), ImageFont.load_default()
    for y in range(4, h - 10, 14):
        draw.text((4, y), " ".join(words[i] for i in rng.randint(0, vocab, 14)), fill=(20, 20, 20, 255), font=font)
    return np.asarray(im).copy()


def flat(h, w):
    return np.full((h, w, 4), 255, np.uint8)


def half_text_half_noise(seed, h, w):
    a = text_like(seed, h, w)
    a[:, w // 2:] = C.noise(seed + 1, h, w - w // 2)
    return a


def text_over_photo(seed, h, w, rows):
    """text in the first `rows` rows, a photograph-like canvas below: with `rows` the rows of a chunk, a window chunk and run chunks"""
    a = C.photo_like(seed, h, w)
    a[:rows] = text_like(seed + 1, rows, w)
    return a


def periodic(seed, period, n, first=None):
    """a one-row canvas whose filtered stream (n bytes, filter byte included) has the given period: random bytes that never run, the
    stream's first byte being the filter byte 4 - so position 0's key returns every period"""
    rng = np.random.default_rng(seed)
    unit = rng.integers(5, 250, period, dtype=np.uint8)
    unit[1:][unit[1:] == unit[:-1]] ^= 1
    unit[0] = 4
    if unit[-1] == 4:
        unit[-1] = 7
    stream = np.tile(unit, -(-n // period))[:n]
    assert (n - 1) % 4 == 0
    return C.row_image(stream[1:])


SHAPES = ((1, 1), (3, 1), (15, 1), (16, 5), (64, 70), (720, 12), (4200, 3))      # (w, h); 5462 x 2 in RGB
RGB_SHAPE = (5462, 2)


@functools.lru_cache(None)
def shape_cases():
    """every shape with text-like content (window wins where a chunk has earlier spans to copy from), and the other contents on the
    shapes with more than one chunk"""
    out = []
    for w, h in SHAPES + (RGB_SHAPE,):
        out.append(("match text %dx%d" % (w, h), text_like(4000 + w, h, w)))
    for w, h in ((64, 70), (720, 12)):
        out.append(("match noise %dx%d" % (w, h), C.noise(4100 + w, h, w)))
        out.append(("match flat %dx%d" % (w, h), flat(h, w)))
        out.append(("match text|noise %dx%d" % (w, h), half_text_half_noise(4200 + w, h, w)))
        out.append(("match photo %dx%d" % (w, h), C.photo_like(4300 + w, h, w)))
    out.append(("match text over photo 720x12", text_over_photo(4400, 12, 720, 5)))
    out.append(("match text|noise 4200x3", half_text_half_noise(4500, 3, 4200)))
    out.append(("match one distance 1024x1", periodic(4600, 128, 4097)))
    out.append(("match period 3 257x1", periodic(4700, 3, 1029)))
    out.append(("match period 67 300x1", periodic(4800, 67, 1201)))
    return out


def by_name():
    return dict(shape_cases())


# a window-winning and a run-winning canvas for one batch launch
BATCH = ("match text 64x70", "match photo 64x70", "match text 1x1", "match text over photo 720x12", "match noise 64x70")


# ---- what the inputs reach ----------------------------------------------------------------------------------------------------
def regimes(rep):
    """the set of regimes the chunks of one encode reach (names as in check_regimes)"""
    got = set()
    forms = [c.form for c in rep.chunks]
    got |= {"form " + f for f in forms}
    if "window" in forms and "huff" in forms:
        got.add("run beside window")
    if len(rep.chunks) > 1 and len(rep.chunks[-1].data) < len(rep.chunks[0].data):
        got.add("short last chunk")
    for c in rep.chunks:
        if c.form != "window":
            continue
        n = len(c.data)
        data = c.data.tolist()
        if len(c.dist_symbols) == 1 and c.dist_symbols[0] > 0:
            got.add("one distance symbol")
        if c.dist_rounds >= 1:
            got.add("distance slack rounds")
        key, H, cand = M.keys(c.data), M.hashes(c.data), M.candidates(c.data)
        for p in range(len(H)):
            if cand[p] >= 0 and key[cand[p]] != key[p]:
                got.add("hash collision")
                break
        for t in c.win_tokens:
            if t.kind != M.WIN:
                continue
            src = t.pos - t.dist
            if src == 0:
                got.add("candidate at position 0")
            if t.dist < t.length:
                got.add("overlapping copy")
            end = t.pos + t.length
            goes_on = end < n and data[src + t.length] == data[end]
            if end % 64 == 0 and goes_on and t.length < 63:
                got.add("cut by the span end")
            if t.length == 63 and t.pos % 64 == 0 and goes_on:
                got.add("capped at 63")
            if n % 64 and t.pos >= n - n % 64:
                got.add("ragged last span")
    return got


ALL_REGIMES = {"form window", "form huff", "form stored", "run beside window", "short last chunk", "one distance symbol", "distance slack rounds",
               "hash collision", "candidate at position 0", "overlapping copy", "cut by the span end", "capped at 63", "ragged last span"}
