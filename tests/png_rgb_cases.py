"""The inputs of the RGB PNG tests (tests/test_png_rgb_reference.py judges them on the CPU, tests/test_gpu_png_rgb.py and
tests/test_node_png_rgb.py run them on the GPU): (name, HxWx4 uint8 canvas) pairs, and report(name, a), the CPU reference's RGB
encode of a canvas (tests/png_rgb_reference.py), computed once per process."""
import functools

import numpy as np

from tests import png_rgb_reference as G
from tests import png_stream_cases as C

_reports = {}


def report(name, a):
    if name not in _reports:
        _reports[name] = G.encode_rgb(a)
    return _reports[name]


# (w, h): the smallest shapes that reach each form of the RGB grid, with the filtered bytes of every chunk
SHAPES = ((1, 1), (3, 5), (100, 130), (2730, 5), (2731, 3), (4096, 2), (5461, 3), (5462, 2), (10923, 2))
CHUNK_BYTES = {(1, 1): [4], (3, 5): [50], (100, 130): [54 * 301, 54 * 301, 22 * 301], (2730, 5): [2 * 8191, 2 * 8191, 8191],
               (2731, 3): [8194] * 3, (4096, 2): [12289] * 2, (5461, 3): [16384] * 3, (5462, 2): [16384, 3] * 2,
               (10923, 2): [16384, 16383, 3] * 2}
# both sides of both boundaries of the two grids (RGB: rows up to 5461 px are one chunk; RGBA: up to 4095), for ist_debug_png_grid
BOUNDARY_SHAPES = ((4095, 3), (4096, 3), (4097, 3), (5460, 4), (5461, 4), (5462, 4), (5463, 4), (2730, 7), (2731, 7), (2047, 9), (2048, 9))


def with_random_alpha(a, seed):
    b = a.copy()
    b[..., 3] = np.random.default_rng(seed).integers(0, 256, a.shape[:2], dtype=np.uint8)
    return b


def opaque(a):
    b = a.copy()
    b[..., 3] = 255
    return b


@functools.lru_cache(None)
def shape_cases():
    """for every shape a photograph-like canvas with RANDOM alpha (its file must be the file of the opaque canvas: alpha is neither
    read nor leaked); flat content and noise on the shapes of each grid form"""
    out = [("rgb photo %dx%d, random alpha" % (w, h), with_random_alpha(C.photo_like(2000 + w, h, w), 2100 + w)) for w, h in SHAPES]
    out += [("rgb flat %dx%d" % (w, h), C.flat_with_lines(2200 + w, h, w)) for w, h in ((3, 5), (100, 130), (2731, 3), (5462, 2), (10923, 2))]
    out += [("rgb noise %dx%d" % (w, h), C.noise(2300 + w, h, w)) for w, h in ((100, 130), (5461, 3), (5462, 2))]
    return out


@functools.lru_cache(None)
def slab_case():
    """5462 x 400: two pieces per row (16384 and 3 bytes), 800 chunks - slabs of 768 and 32 on the host path; flat with lines and a
    band of noise rows on either side of the slab boundary (built as png_stream_cases.slab_case is)"""
    h, w = 400, 5462
    a = np.full((h, w, 4), 255, np.uint8)
    a[::37, 100:900, :3] = 30
    a[5::53, 3000:, :3] = (40, 120, 200)
    a[380:383] = C.noise(7, 3, w)                                     # (chunks 760..765 in the first slab ...)
    a[390:392] = C.noise(8, 2, w)                                     # (... and 780..783 in the second)
    return "rgb slabs 5462x400", a


def all_cases():
    return shape_cases() + [slab_case()]


def check_regimes():
    """every input reaches the grid form it was built for, and both chunk forms occur"""
    for name, a in shape_cases():
        h, w = a.shape[:2]
        assert [len(c.data) for c in report(name, a).chunks] == CHUNK_BYTES[(w, h)], name
    forms = {c.form for name, a in shape_cases() for c in report(name, a).chunks}
    assert forms == {"huff", "stored"}
    name, a = slab_case()
    chunks = report(name, a).chunks
    assert len(chunks) == 800 and [len(c.data) for c in chunks] == [16384, 3] * 400
    assert {c.form for c in chunks[:768]} == {"huff", "stored"} and {c.form for c in chunks[768:]} == {"huff", "stored"}
    assert {c.form for c in chunks[760:766:2]} == {"stored"} and {c.form for c in chunks[780:784:2]} == {"stored"}      # the noise rows
