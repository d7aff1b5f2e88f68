"""The inputs of the adaptive-row-filter PNG tests (tests/test_png_filter_reference.py judges them on the CPU, tests/test_gpu_png_filter.py
and tests/test_node_png_filter.py run them on the GPU): (name, HxWx4 uint8 canvas) pairs per colour form, and report(name, a, bpp),
the CPU reference's adaptive encode of a canvas (tests/png_filter_reference.py), computed once per process."""
import functools

import numpy as np

from tests import png_deflate_reference as R
from tests import png_filter_reference as F
from tests import png_rgb_cases as K
from tests import png_stream_cases as C

_reports = {}


def report(name, a, bpp):
    if (name, bpp) not in _reports:
        _reports[(name, bpp)] = F.encode_adaptive(a, bpp)
    return _reports[(name, bpp)]


# (w, h): the smallest shapes that reach each form of the chunk grid - whole rows, several per chunk; one row per chunk; two and three
# pieces per row - in either colour form
SHAPES = {4: ((1, 1), (3, 5), (257, 19), (4095, 2), (4096, 2), (8191, 2)), 3: ((2730, 5), (5461, 3), (5462, 2), (10923, 2))}
ROWS_PER_CHUNK = {(1, 1): 1, (3, 5): 5, (257, 19): 15, (4095, 2): 1, (4096, 2): 0, (8191, 2): 0, (2730, 5): 2, (5461, 3): 1, (5462, 2): 0, (10923, 2): 0}
PIECES = {(4096, 2): 2, (8191, 2): 3, (5462, 2): 2, (10923, 2): 3}


def repeated_below(row, seed):
    out = row.copy()
    out[::5] = C.noise(seed, 1, len(row[::5]))[0]
    return out


def rows_of_kinds(seed, w, spec):
    """a canvas of len(spec) rows: 'n' a noise row, 'u' the row above again with every fifth pixel drawn anew (Up pays for those pixels
    only; Paeth, which ties with Up on an exact copy, also mispredicts their right neighbours), 'a' pixels alternating 1 and 255 (None
    costs 1 a byte, Sub 2, and under a noise row everything else far more), 'p' a row of a photograph-like canvas; alpha is noise in
    'n' and 'u' rows (the RGB form must not read it)"""
    h = len(spec)
    photo = C.photo_like(seed, h, w)
    a = np.empty((h, w, 4), np.uint8)
    for y, kind in enumerate(spec):
        if kind == "n":
            a[y] = C.noise(seed + 17 * y, 1, w)[0]
        elif kind == "u":
            a[y] = repeated_below(a[y - 1], seed + 17 * y)
        elif kind == "a":
            a[y] = np.where(np.arange(w) % 2 == 0, 1, 255).astype(np.uint8)[:, None]
        else:
            a[y] = photo[y]
    return a


SPECS = {2: ("nu", "na"), 3: ("nua",), 5: ("nunap",), 19: ("nunapppnuanppppppnu",)}


@functools.lru_cache(None)
def shape_cases(bpp):
    """for every shape: photograph-like content (Average, mostly), flat content with lines (Paeth, Sub, Up) and rows of chosen kinds
    (Up, None)"""
    out = []
    for w, h in SHAPES[bpp]:
        out.append(("filter photo %dx%d" % (w, h), K.with_random_alpha(C.photo_like(3000 + w, h, w), 3100 + w) if bpp == 3 else C.photo_like(3000 + w, h, w)))
        for spec in SPECS.get(h, ()):
            out.append(("filter rows %s %dx%d" % (spec, w, h), rows_of_kinds(3200 + w, w, spec)))
    for w, h in {4: ((3, 5), (257, 19), (8191, 2)), 3: ((2730, 5), (10923, 2))}[bpp]:
        out.append(("filter flat %dx%d" % (w, h), C.flat_with_lines(3300 + w, h, w)))
    if bpp == 4:
        out.append(("filter flat 300x40", C.flat_with_lines(3, 40, 300)))           # (lines above one another: rows where Sub beats Paeth)
        out.append(("filter white 64x33", np.full((33, 64, 4), 255, np.uint8)))     # (nothing beats Paeth: the default form's file)
    else:
        out.append(("filter flat 300x40", C.flat_with_lines(3, 40, 300)))
    return out


def _slab_cut(w, seed):
    """155 rows of five pieces: 775 chunks, on the host path a first slab of 768 = 153 rows + 3 pieces, so rows 0..153 are evaluated on
    one stream and rows 153, 154 on the other.  Noise rows on both sides of the cut; the cut row 153 repeats row 152 but for every fifth
    pixel (Up)."""
    h = 155
    a = np.full((h, w, 4), 255, np.uint8)
    a[::37, 100:900, :3] = 30
    a[150] = np.where(np.arange(w) % 2 == 0, 1, 255).astype(np.uint8)[:, None]
    a[151] = C.noise(seed, 1, w)[0]
    a[152] = C.noise(seed + 1, 1, w)[0]
    a[153] = repeated_below(a[152], seed + 3)
    a[154] = C.noise(seed + 2, 1, w)[0]
    return a


@functools.lru_cache(None)
def slab_cut_case(bpp):
    w = {4: 16381, 3: 21845}[bpp]
    return "filter slab cut %dx155" % w, _slab_cut(w, 3400 + bpp)


def all_cases(bpp):
    return shape_cases(bpp) + [slab_cut_case(bpp)]


def tie_rows(a, bpp):
    """rows y > 0 that are not flat and on which two filters share the least, non-zero cost"""
    cost = F.row_costs(a, bpp)
    least = cost.min(axis=1)
    shared = (cost == least[:, None]).sum(axis=1) >= 2
    varied = np.array([len(np.unique(a[y, :, :bpp].reshape(-1, bpp), axis=0)) > 1 for y in range(a.shape[0])])
    return [y for y in range(1, a.shape[0]) if shared[y] and least[y] > 0 and varied[y]]


def check_regimes():
    """every input reaches what it was built for: the grid form of its shape, all five types over the set, a tie that is neither row 0's
    nor a flat row's, a chunk of several rows of different types, and files that each near miss of the rule changes"""
    chosen, ties, mixed_chunks = set(), 0, 0
    changed = {k: 0 for k in F.NEAR_MISSES}
    for bpp in (4, 3):
        for name, a in shape_cases(bpp):
            h, w = a.shape[:2]
            rep, types = report(name, a, bpp), F.row_filters(a, bpp)
            assert types[0] not in (F.SUB, F.NONE), name                  # (row 0: Sub is Paeth and None is Up there, and both lose that tie)
            chosen |= set(types.tolist())
            ties += len(tie_rows(a, bpp))
            grid = F._grid(w, h, bpp)
            if (w, h) in ROWS_PER_CHUNK:
                assert len(grid) == (h * PIECES[(w, h)] if ROWS_PER_CHUNK[(w, h)] == 0 else -(-h // ROWS_PER_CHUNK[(w, h)])), name
            mixed_chunks += sum(1 for y0, rows, x0, px in grid if rows > 1 and len(set(types[y0:y0 + rows].tolist())) > 1)
            assert bytes(rep.filtered[::bpp * w + 1]) == bytes(types), name
            for k, rule in F.NEAR_MISSES.items():
                changed[k] += F.encode_adaptive(a, bpp, rule).stream != rep.stream
    assert chosen == {F.NONE, F.SUB, F.UP, F.AVERAGE, F.PAETH}, chosen
    assert ties >= 1 and mixed_chunks >= 1, (ties, mixed_chunks)
    assert all(v >= 1 for v in changed.values()), changed
    for bpp in (4, 3):
        name, a = slab_cut_case(bpp)
        h, w = a.shape[:2]
        types = F.row_filters(a, bpp)
        assert len(F._grid(w, h, bpp)) == 775 and R.host_slabs(775) == [768, 7] and 768 == 153 * 5 + 3
        assert types[153] == F.UP and types[150] == F.NONE and set(types[:150].tolist()) == {F.PAETH, F.SUB}, types[148:].tolist()
