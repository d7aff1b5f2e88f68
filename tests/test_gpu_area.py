"""filter 'area' (IST_FILTER_AREA, the box filter) against the fp64 oracle across its whole shrink range.

A canvas pixel averages a max(1, |kx|) x max(1, |ky|) box of source pixels, so the kernel that runs depends on the scale
(ist_compile.cpp, cell classification): the streamed box filter (tile_area_stream) with tiles of up to 128 pixels (2 per
lane) while a tile's x footprint fits one 256-pixel pass, narrow tiles of 16 / 8 / 4 / 2 pixels up to |kx| = 200, and the
per-pixel general loop beyond that or past |ky| = 64.  Tolerance: the op-list rule (solid pixels within 1 LSB, translucent
readback within 1 + ceil(255 / a)), and differences must be rare and unbiased: of the solid channel bytes, fewer than 1 %
may differ, and their signed sum stays within 0.001 LSB per byte plus three standard deviations of unbiased +-1 noise.
Measured on an MI355X (differing solid channel bytes, mean signed difference in LSB): op-list fuzz 13 of 4.4e6 (+1.6e-6),
regime sweep x 328 of 2.1e6 (+1.5e-4), y 154 of 1.8e6 (+4.7e-5), min strips 7 and 4 of 2.6e5 (-2.7e-5, +7.8e-6), platform
plans 1-3 of 1.6e4-3.2e5.  The sweep's differences are nearly all +1, most likely because its dyadic row weights (|ky| 1.5,
2 and 4 at offsets 0, 0.25 and 0.5) put many means close to x.5, where the fp32 sum can round onto the tie (and then up) while
the fp64 one stays just below it."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from imagestitching_amd.stitch import _ctx
from oracle import oracle as O
from tests import util as U

pytestmark = pytest.mark.gpu
AREA, AA = 2, 0x100


def _c_ops(ops_o):
    ops = (L.Op * len(ops_o))()
    for i, o in enumerate(ops_o):
        ops[i].m[:] = o["m"]
        if o["kind"] == "fill":
            ops[i].kind = 0; ops[i].image = -1; ops[i].d[:] = o["rect"]; ops[i].rgba[:] = o["rgba"]
        else:
            ops[i].kind = 1; ops[i].image = o["image"]; ops[i].s[:] = o["s"]; ops[i].d[:] = o["d"]
    return ops


def _descs(px, opaque=None):
    return (L.ImageDesc * len(px))(*[L.ImageDesc(a.shape[1], a.shape[0], 1, 0, 0, int(bool(opaque and opaque[k])), 0) for k, a in enumerate(px)])


def _render_host(cw, ch, clear, ops_o, px, aa):
    """ist_render_rgba8: host buffers in, host canvas out"""
    ops = _c_ops(ops_o)
    n = len(px)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in px])
    pit = (C.c_size_t * n)(*[a.strides[0] for a in px])
    out = np.zeros((ch, cw, 4), np.uint8)
    L.check(L.lib.ist_render_rgba8(_ctx(0), cw, ch, (C.c_uint8 * 4)(*clear), ops, len(ops_o), _descs(px), ptrs, pit, n,
                                   AREA | (AA if aa else 0), None, out.ctypes.data, out.strides[0]))
    return out


def _render_job(cw, ch, clear, ops_o, px, opaque):
    """a compiled job on device tensors: returns (canvas, job.info)"""
    job = ist.Stitcher(0).compile_ops(cw, ch, _c_ops(ops_o), len(ops_o), _descs(px, opaque), len(px), AREA, clear=clear)
    out = torch.full((ch, cw, 4), 0x5A, dtype=torch.uint8, device="cuda")
    job.launch([torch.from_numpy(a).cuda() for a in px], out)
    torch.cuda.synchronize()
    info = dict(job.info)
    job.close()
    return out.cpu().numpy(), info


def _m(t, sc, e, f):
    """one of the 8 axis-aligned transforms: bit 0 flips x, bit 1 flips y, bit 2 turns a quarter"""
    sx, sy = (-sc if t & 1 else sc), (-sc if t & 2 else sc)
    return [0, sx, sy, 0, e, f] if t & 4 else [sx, 0, 0, sy, e, f]


# ------------------------------------------------------------------------------------------------ op-list fuzz
def test_random_op_lists_under_the_area_filter():
    """op lists as the Canvas shim records them, filter 'area': per-axis scales log-uniform from 0.5 to 300 (one axis may stretch
    while the other shrinks), all eight transforms, fractional offsets, source rectangles that leave the bitmap, overlapping and
    translucent draws, opaque or transparent canvases, edge AA on a third of the cases"""
    rng = np.random.default_rng(2024)
    stats = U.RareDiff()
    for case in range(120):
        cw, ch = int(rng.integers(8, 200)), int(rng.integers(8, 200))
        ops_o, px = [], []
        if rng.integers(0, 2):
            ops_o.append({"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": tuple(int(v) for v in rng.integers(0, 256, 3)) + (255,)})
        for _ in range(int(rng.integers(1, 5))):
            kx, ky = (float(math.exp(rng.uniform(math.log(0.5), math.log(300.0)))) for _ in range(2))
            t = int(rng.integers(0, 8))
            sc = 1.0 if rng.integers(0, 2) else float(rng.uniform(0.5, 2.0))
            dw, dh = float(rng.uniform(2, 150)), float(rng.uniform(2, 150))
            shrink = math.sqrt(dw * dh * sc * sc * kx * ky / 6.0e5)         # keep the source (and the oracle's box sums) small
            if shrink > 1.0:
                dw, dh = max(1.0, dw / shrink), max(1.0, dh / shrink)
            sw, sh = kx * sc * dw, ky * sc * dh                              # |k| = (sw / dw) / sc
            w, h = max(2, int(sw * rng.uniform(0.6, 1.3))), max(2, int(sh * rng.uniform(0.6, 1.3)))
            px.append(U.rand_image(5000 + 11 * case + len(px), h, w, opaque=bool(rng.integers(0, 2))))
            s = [float(rng.uniform(-5, max(0.0, w - sw / 2))), float(rng.uniform(-5, max(0.0, h - sh / 2))), sw, sh]
            e, f = float(rng.integers(0, cw)), float(rng.integers(0, ch))
            if rng.integers(0, 2):
                e += float(rng.uniform(0, 1)); f += float(rng.uniform(0, 1))
            d = [float(rng.uniform(-20, 20)), float(rng.uniform(-20, 20)), dw, dh]
            ops_o.append({"kind": "draw", "image": len(px) - 1, "m": _m(t, sc, e, f), "s": s, "d": d})
        clear = (0, 0, 0, 0) if rng.integers(0, 2) else tuple(int(v) for v in rng.integers(0, 256, 3)) + (255,)
        aa = bool(rng.integers(0, 3) == 0)
        descs_o = [{"width": a.shape[1], "height": a.shape[0]} for a in px]
        ref = O.render_ops(cw, ch, ops_o, descs_o, px, "area", clear=clear, edge_aa=aa)
        out = _render_host(cw, ch, clear, ops_o, px, aa)
        try:
            stats.add(U.oracle_tolerance(out, ref))
        except AssertionError as e:
            raise AssertionError("case %d (aa %s): %s; ops %r" % (case, aa, e, ops_o))
    print("area op-list fuzz:", stats)
    stats.check()


# ------------------------------------------------------------------------------------------------ regime sweep
def _tile_w(akx):
    """the streamed tile width ist_compile.cpp picks for |kx| (one 64-lane pass), 0 = the general path"""
    bwx = max(akx, 1.0)
    foot = lambda w: (math.ceil((w - 1) * akx + bwx) + 2 + 3) & ~3                  # noqa: E731
    w = int(min(128.0, math.floor((253.0 - bwx) / akx) + 1.0)) if 253.0 - bwx >= 0 else 0
    if w >= 24:
        return w
    if akx <= 200.0:
        for w in (16, 8, 4, 2, 1):
            if foot(w) <= 768:
                return w
    return 0


def _tile_h(aky):
    rows = math.ceil(max(aky, 1.0)) + 1
    return 32 if rows <= 4 else 8 if rows <= 6 else 4


# |kx| just below / above each boundary of the tile width: 128 px (253 / |kx| >= 128), 2 px per lane (> 64), the widest streamed
# tile (>= 24), narrow tiles 16 -> 8 -> 4 -> 2 (footprint <= 768 px) and the general path (|kx| > 200)
X_SCALES = [1.95, 2.0, 3.85, 3.95, 10.5, 10.6, 47.8, 47.95, 95.7, 95.8, 191.4, 191.6, 199.9, 200.1]
# |ky| around the tile heights (box rows <= 4: 32, <= 6: 8, else 4) and the general path (|ky| > 64); 0.6 stretches
Y_SCALES = [2.95, 3.05, 4.95, 5.05, 63.9, 64.1, 0.6]
OFFSETS = [0.0, 0.25, 0.5 - 1e-6, 0.5, 0.999]


def _sweep_case(rng, kx, ky, off, flip, past, opaque_draw, seed):
    """one draw covering the whole canvas over an opaque fill; returns (ops, pixels, canvas size, expected tile shape or None)"""
    tw = _tile_w(kx) if ky <= 64.0 else 0
    cw = max(9, min(2 * tw + 13 if tw else 77, int(2.5e4 / kx)))           # never a multiple of the tile width
    if tw:
        assert cw % tw, (kx, cw, tw)
    ch = max(5, min(45, int(4.0e4 / max(ky, 1.0) / max(cw * kx / 300.0, 1.0))))
    sw, sh = kx * cw, ky * ch
    if past:       # the source rectangle starts 3 pixels before the bitmap and ends 3 after it: chunks straddle cx0 and cx1
        w, h = max(2, int(math.ceil(sw)) - 6 + 1), max(2, int(math.ceil(sh)) - 6 + 1)
        s = [-3.0 + off, -3.0 + off, sw, sh]
    else:          # cropped out of a larger bitmap at an offset that is not a multiple of 4 pixels
        w, h = int(math.ceil(sw)) + 9, int(math.ceil(sh)) + 9
        s = [5.0 + off, 5.0 + off, sw, sh]
    px = [U.rand_image(seed, h, w, opaque=opaque_draw)]
    fill = tuple(int(v) for v in rng.integers(0, 256, 3)) + (255,)
    ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": fill},
           {"kind": "draw", "image": 0, "m": _m(flip, 1.0, cw if flip & 1 else 0, ch if flip & 2 else 0), "s": s, "d": [0, 0, cw, ch]}]
    return ops, px, cw, ch, (tw, _tile_h(ky)) if tw else None


def _box_rows(ky, oy, ch):
    """(number of source rows in each output row's box) mod 4, as the kernel walks them"""
    bh = max(abs(ky), 1.0)
    yc = ky * (np.arange(ch) + 0.5) + oy
    return set(((np.ceil(yc + 0.5 * bh) - np.floor(yc - 0.5 * bh)).astype(np.int64) % 4).tolist())


@pytest.mark.parametrize("axis", ["x", "y"])
def test_area_regimes_at_their_boundaries(axis):
    """scales just below and above every boundary of ist_compile.cpp's choice: the streamed path (tiles_general == 0, and the tile
    count of the width / height the compiler's rule picks) or the general one; fractional offsets, canvas widths that are not a
    multiple of the tile width, 16-byte chunks that straddle the source's clamp box, every box row count mod 4, an opaque and a
    translucent draw (the OPAQUE template flag), flips"""
    rng = np.random.default_rng(31 if axis == "x" else 32)
    stats = U.RareDiff()
    residues, paths = set(), {}
    ky_cycle = [1.5, 2.0, 3.0, 4.0, 5.0, 2.6]
    for n, scale in enumerate(X_SCALES if axis == "x" else Y_SCALES):
        for k, off in enumerate(OFFSETS):
            for opaque_draw in (True, False):
                kx, ky = (scale, ky_cycle[(n + k) % len(ky_cycle)]) if axis == "x" else (2.5 + 0.7 * k, scale)
                flip = (n + k) % 4
                ops, px, cw, ch, tile = _sweep_case(rng, kx, ky, off, flip, past=(k % 2 == 1), opaque_draw=opaque_draw, seed=7000 + 97 * n + 2 * k + opaque_draw)
                out, info = _render_job(cw, ch, (0, 0, 0, 0), ops, px, [opaque_draw])
                what = (axis, scale, off, opaque_draw, info)
                if tile:
                    tw, th = tile
                    assert info["tiles_general"] == 0 and info["tiles_sample"] == info["n_tiles"] == -(-cw // tw) * -(-ch // th), what
                else:
                    assert info["tiles_sample"] == 0 and info["tiles_general"] > 0, what
                paths[scale] = (tile[0] if axis == "x" else tile[1]) if tile else 0          # 0: the general path
                ref = O.render_ops(cw, ch, ops, [{"width": px[0].shape[1], "height": px[0].shape[0]}], px, "area")
                try:
                    stats.add(U.oracle_tolerance(out, ref))
                except AssertionError as e:
                    raise AssertionError("%r: %s" % (what, e))
                if ky > 1.0:
                    oy = ops[1]["s"][1] if not flip & 2 else ops[1]["s"][1] + ops[1]["s"][3]
                    residues |= _box_rows(-ky if flip & 2 else ky, oy, ch)
    print("area regimes (%s):" % axis, paths, stats)
    assert residues == {0, 1, 2, 3}
    scales = X_SCALES if axis == "x" else Y_SCALES[:6]
    assert all(paths[a] != paths[b] for a, b in zip(scales[::2], scales[1::2])), paths      # each pair straddles a boundary
    assert paths[scales[-2]] > 0 and paths[scales[-1]] == 0
    stats.check()


# ------------------------------------------------------------------------------------------------ known answer
@pytest.mark.parametrize("k", [2, 3, 7, 64, 65, 250])
def test_block_aligned_integer_shrinks_give_the_block_colours_exactly(k):
    """a source of k x k blocks of random constant colours shrunk k times with every box on a block: each canvas pixel is its
    block's colour exactly.  A box shifted by one row or column, or a wrong normalisation, mixes neighbours (a large error)."""
    rng = np.random.default_rng(k)
    W, H = {2: (150, 70), 3: (150, 70), 7: (100, 37), 64: (21, 12), 65: (21, 12), 250: (9, 5)}[k]
    B = rng.integers(0, 256, (H + 3, W + 2, 4), dtype=np.uint8)
    B[..., 3] = 255
    src = np.ascontiguousarray(np.repeat(np.repeat(B, k, axis=0), k, axis=1))
    want_b = B[2:2 + H, 1:1 + W]
    for t in range(8):
        cw, ch = (H, W) if t & 4 else (W, H)
        sx, sy = (-1 if t & 1 else 1), (-1 if t & 2 else 1)
        e = (cw if (sy if t & 4 else sx) < 0 else 0)
        f = (ch if (sx if t & 4 else sy) < 0 else 0)
        ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": (1, 2, 3, 255)},
               {"kind": "draw", "image": 0, "m": _m(t, 1.0, e, f), "s": [k * 1, k * 2, k * W, k * H], "d": [0, 0, W, H]}]
        want = want_b.transpose(1, 0, 2) if t & 4 else want_b
        if (sx if not t & 4 else sy) < 0:
            want = want[:, ::-1]
        if (sy if not t & 4 else sx) < 0:
            want = want[::-1]
        out, info = _render_job(cw, ch, (0, 0, 0, 0), ops, [src], [True])
        streamed = not t & 4 and k <= 64
        assert (info["tiles_general"] == 0) == streamed, (k, t, info)
        bad = (out != want).any(axis=-1)
        assert not bad.any(), (k, t, int(bad.sum()), U.max_abs_diff(out, np.ascontiguousarray(want)))


# ------------------------------------------------------------------------------------------------ planner-driven strong shrinks
@pytest.mark.parametrize("direction", ["vertical", "horizontal"])
def test_min_strips_mixing_a_narrow_image_with_large_ones(direction):
    """mode 'min' strips in which one narrow image sets the strip's width: one draw shrinks more than 200x (the general path) and the
    others 10-60x, under all eight orientations"""
    sizes = [(36, 300), (8000, 900), (1500, 500), (700, 260), (400, 1200)]          # (w, h): shrinks ~222x, 42x, 19x, 11x
    if direction == "horizontal":
        sizes = [(h, w) for w, h in sizes]
    px = [U.rand_image(6100 + i, h, w, opaque=(i != 3)) for i, (w, h) in enumerate(sizes)]
    stats = U.RareDiff()
    for ori in ([1, 1, 1, 1, 1], [1, 2, 3, 4, 5], [4, 3, 6, 7, 8], [2, 1, 8, 5, 6]):
        opts = {"filter": "area", "mode": "min", "gap": 2}
        p = ist.plan(U.hip_images(px, ori), direction, opts)
        along = "dw" if direction == "vertical" else "dh"
        shrink = [(px[r["image"]].shape[1] if direction == "vertical" else px[r["image"]].shape[0]) / r[along] for r in p.rects]
        assert max(shrink) > 200, shrink          # the wide image is never turned, so it shrinks > 200x
        got = ist.stitch(U.hip_images(px, ori), direction, opts)["data"]
        ref, _, _ = U.oracle_stitch(px, direction, opts, orientations=ori)
        try:
            stats.add(U.oracle_tolerance(got, ref))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (ori, e))
    print("area min strips (%s):" % direction, stats)
    stats.check()


@pytest.mark.parametrize("opts", [{"platform": "android", "maxSide": 128}, {"platform": "ios", "superSample": 1, "maxSide": 96},
                                  {"platform": "android", "maxSide": 700, "maxPixels": 40000}])
def test_platform_plans_with_edge_antialiasing(opts):
    """the reference platforms' capped plans (fractional seams, edge AA on by default) shrinking strongly under 'area'"""
    px = [U.rand_image(6200 + i, h, w, opaque=(i != 1)) for i, (w, h) in enumerate([(1600, 1200), (900, 1500), (2400, 700), (500, 380)])]
    ori = [1, 6, 3, 8]
    o = dict(opts, filter="area")
    assert U.edge_aa_of(o)
    stats = U.RareDiff()
    for direction in ("vertical", "horizontal"):
        got = ist.stitch(U.hip_images(px, ori), direction, o)["data"]
        ref, _, _ = U.oracle_stitch(px, direction, o, orientations=ori)
        stats.add(U.oracle_tolerance(got, ref))
    print("area platform plans %r:" % opts, stats)
    stats.check()
