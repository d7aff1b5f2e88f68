"""filter 'cubic' (IST_FILTER_CUBIC: Catmull-Rom on axes that do not shrink, the box of 'area' on axes that do) on the GPU, against
tests/cubic_reference.py (numpy, fp64) under the op-list tolerance rule: solid bytes within 1 LSB, translucent readback within
1 + ceil(255 / a), fewer than 1 % of the solid channel bytes different, differences unbiased (tests/util.py).

Which kernel runs depends on the draw (ist_compile.cpp): the streamed cubic path (tile_cubic_stream) for ONE axis-aligned draw that
shrinks on neither axis over an opaque colour, the streamed box filter for one that shrinks on both, the per-pixel stack for the
rest (one axis each way, quarter turns, overlaps, anti-aliased strips, translucent over translucent), and the copy path - the flat
form included - for 1:1 draws at integer offsets, where the cubic weights are (0, 1, 0, 0).
Reference anchor: index.js:1363, 1426-1428 (the small-job plan super-samples 2.2-2.6x), index.js:1416-1421 (smoothing quality)."""
import ctypes as C
import hashlib
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from imagestitching_amd.stitch import _ctx
from tests import cubic_reference as R
from tests import cubic_render as G
from tests import util as U

pytestmark = pytest.mark.gpu
CUBIC, AA = G.CUBIC, G.AA
_c_ops, _descs = G.c_ops, G.descs


def _render_host(cw, ch, clear, ops_o, px, aa):
    """ist_render_rgba8: host buffers in, host canvas out"""
    ops = _c_ops(ops_o)
    n = len(px)
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in px])
    pit = (C.c_size_t * n)(*[a.strides[0] for a in px])
    out = np.zeros((ch, cw, 4), np.uint8)
    L.check(L.lib.ist_render_rgba8(_ctx(0), cw, ch, (C.c_uint8 * 4)(*clear), ops, len(ops_o), _descs(px), ptrs, pit, n,
                                   CUBIC | (AA if aa else 0), None, out.ctypes.data, out.strides[0]))
    return out


_render_job = G.render_job          # (guard rows, a wider canvas pitch, sources embedded in poison: tests/cubic_render.py)


# ------------------------------------------------------------------------------------------------ op-list fuzz
def test_random_op_lists_under_the_cubic_filter():
    """op lists as the Canvas shim records them, filter 'cubic': per-axis scales log-uniform over 0.1 .. 8 (enlarged, shrunk and
    mixed axes all occur), all eight transforms, fractional offsets, source rectangles that leave the bitmap, overlapping and
    translucent draws, opaque or transparent canvases, edge AA on a third of the cases"""
    rng = np.random.default_rng(3003)
    stats = U.RareDiff()
    for case in range(120):
        cw, ch, ops_o, px, clear, aa = R.random_op_list(rng, case, 0.1, 8.0)
        ref = R.render_ops(cw, ch, ops_o, None, px, "cubic", clear=clear, edge_aa=aa)
        out = _render_host(cw, ch, clear, ops_o, px, aa)
        try:
            stats.add(U.oracle_tolerance(out, ref))
        except AssertionError as e:
            raise AssertionError("case %d (aa %s): %s; ops %r" % (case, aa, e, ops_o))
    print("cubic op-list fuzz:", stats)
    stats.check()


# ------------------------------------------------------------------------------------------------ regime sweep of the fast path
SCALES = [1.0, 0.9, 0.75, 0.5, 1 / 2.2, 1 / 2.6, 0.25, 0.1]       # |k|: source pixels per canvas pixel


def _sweep_case(rng, k, flip, past, opaque_draw, seed, cw, ch):
    """one draw covering the whole canvas over an opaque fill.  past: the source rectangle starts 2.5 pixels before the bitmap and ends
    after it (the bitmap's edge falls inside a tile: chunks straddle the clamp box); otherwise it is cropped out of a larger bitmap
    at a fractional offset that is not a multiple of 4 pixels."""
    sw, sh = k * cw, k * ch
    if past:
        w, h = max(1, int(math.ceil(sw)) - 5), max(1, int(math.ceil(sh)) - 5)
        s = [-2.5, -2.25, sw, sh]
    else:
        w, h = int(math.ceil(sw)) + 9, int(math.ceil(sh)) + 9
        s = [5.3, 5.6, sw, sh]
    px = [U.rand_image(seed, h, w, opaque=opaque_draw)]
    fill = tuple(int(v) for v in rng.integers(0, 256, 3)) + (255,)
    ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": fill},
           {"kind": "draw", "image": 0, "m": R.transform(flip, 1.0, cw if flip & 1 else 0, ch if flip & 2 else 0), "s": s, "d": [0, 0, cw, ch]}]
    return ops, px


def test_cubic_fast_path_across_its_scales():
    """one draw at |k| = 1 (fractional offset) down to 0.1 (a 10x enlargement), plain and mirrored on either axis, opaque and
    translucent bitmaps (the OPAQUE template flag), canvases of full and partial tiles, and bitmaps whose edge falls inside a tile.
    job.info says which path ran: every tile of these jobs is a streamed one (tiles_general == 0), so the sweep cannot pass on the
    per-pixel path alone."""
    rng = np.random.default_rng(41)
    stats = U.RareDiff()
    for n, k in enumerate(SCALES):
        for v in range(4):
            opaque_draw = v % 2 == 0
            flip = (n + v) % 4
            cw, ch = (2 * 256 + 13, 70) if v < 2 else (300 - 7 * n, 33 + n)
            ops, px = _sweep_case(rng, k, flip, past=(v in (1, 2)), opaque_draw=opaque_draw, seed=8000 + 10 * n + v, cw=cw, ch=ch)
            out, info = _render_job(cw, ch, (0, 0, 0, 0), ops, px, [opaque_draw])
            what = (k, v, flip, info)
            assert info["tiles_general"] == 0 and info["tiles_sample"] == info["n_tiles"] == -(-cw // 256) * -(-ch // 32), what
            ref = R.render_ops(cw, ch, ops, None, px, "cubic")
            try:
                stats.add(U.oracle_tolerance(out, ref))
            except AssertionError as e:
                raise AssertionError("%r: %s" % (what, e))
    print("cubic fast path sweep:", stats)
    stats.check()


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 3), (3, 2), (3, 3)])
def test_sources_so_narrow_that_every_tap_clamps(w, h):
    stats = U.RareDiff()
    for flip in range(4):
        px = [U.rand_image(8200 + 7 * w + h + flip, h, w, opaque=bool(flip & 1))]
        cw, ch = 40 * w + 3, 37 * h
        ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, cw, ch], "rgba": (200, 100, 50, 255)},
               {"kind": "draw", "image": 0, "m": R.transform(flip, 1.0, cw if flip & 1 else 0, ch if flip & 2 else 0), "s": [0, 0, w, h], "d": [0, 0, cw, ch]}]
        out, info = _render_job(cw, ch, (0, 0, 0, 0), ops, px, [bool(flip & 1)])
        assert info["tiles_general"] == 0 and info["tiles_sample"] == info["n_tiles"], info
        stats.add(U.oracle_tolerance(out, R.render_ops(cw, ch, ops, None, px, "cubic")))
    stats.check()


def test_mixed_jobs_hold_both_streamed_paths_and_the_per_pixel_stack():
    """one op list with an enlarged draw, a draw shrunk on both axes, one with an axis each way and a quarter-turned enlargement,
    side by side on a transparent canvas: the streamed cubic and box paths and the per-pixel stack in ONE launch (kernel kind 6),
    and without the last two draws the form without the per-pixel stack (kind 5)"""
    px = [U.rand_image(8300, 50, 60), U.rand_image(8301, 200, 260), U.rand_image(8302, 40, 300, opaque=False), U.rand_image(8303, 30, 45)]
    ident = [1, 0, 0, 1, 0, 0]
    draws = [{"kind": "draw", "image": 0, "m": ident, "s": [0, 0, 60, 50], "d": [0, 0, 150, 120]},
             {"kind": "draw", "image": 1, "m": ident, "s": [0, 0, 260, 200], "d": [150, 0, 100, 80]},
             {"kind": "draw", "image": 2, "m": ident, "s": [0, 0, 300, 40], "d": [0, 120, 120, 90]},
             {"kind": "draw", "image": 3, "m": [0, 1, -1, 0, 250, 120], "s": [0, 0, 45, 30], "d": [0, 0, 90, 60]}]
    stats = U.RareDiff()
    for n_draws, general in ((2, False), (4, True)):
        ops = draws[:n_draws]
        out, info = _render_job(260, 215, (0, 0, 0, 0), ops, px, [True, True, False, True])
        assert info["tiles_sample"] > 0 and (info["tiles_general"] > 0) == general, info
        stats.add(U.oracle_tolerance(out, R.render_ops(260, 215, ops, None, px, "cubic")))
    print("cubic mixed job:", stats)
    stats.check()


# ------------------------------------------------------------------------------------------------ plans
def _stitch_against_reference(px, direction, opts, ori=None):
    o = dict(opts, filter="cubic")
    images = U.hip_images(px, ori)
    p = ist.plan(images, direction, o)
    got = ist.stitch(images, direction, o)["data"]
    ref = R.render_ops(p.canvas_w, p.canvas_h, R.plan_ops(p), None, px, "cubic", edge_aa=U.edge_aa_of(o))
    return U.oracle_tolerance(got, ref), p


@pytest.mark.parametrize("platform,ss", [("devtools", 2.6), ("ios", 2.2)])
def test_the_super_sampled_small_job_plan(platform, ss):
    """plan golden G1 as the reference renders it: 3 x 640x480 under ctx.scale(2.6) (2.2 on iOS), edge AA on"""
    px = [U.smooth_image(8400 + i, 480, 640) if i == 1 else U.rand_image(8400 + i, 480, 640) for i in range(3)]
    stats = U.RareDiff()
    s, p = _stitch_against_reference(px, "vertical", {"platform": platform})
    assert p.super_sample == ss and (p.canvas_w, p.canvas_h) == (math.floor(640 * ss), math.floor(1440 * ss))
    stats.add(s)
    print("cubic G1 %s:" % platform, stats)
    stats.check()


@pytest.mark.parametrize("direction", ["vertical", "horizontal"])
def test_mode_max_strips(direction):
    """mode 'max' enlarges every image narrower than the widest (G5: 1920 -> 4032, 2.1x)"""
    sizes = [(4032, 150), (1920, 130), (3000, 90), (4031, 60)]
    if direction == "horizontal":
        sizes = [(h, w) for w, h in sizes]
    px = [U.rand_image(8500 + i, h, w, opaque=(i != 2)) for i, (w, h) in enumerate(sizes)]
    stats = U.RareDiff()
    s, p = _stitch_against_reference(px, direction, {"mode": "max", "gap": 3})
    assert (p.canvas_w if direction == "vertical" else p.canvas_h) == 4032
    stats.add(s)
    print("cubic max strip (%s):" % direction, stats)
    stats.check()


def test_orientations_2_to_8_enlarged():
    """EXIF 2-4 mirror (the streamed path, negative k), 5-8 turn a quarter (the per-pixel stack)"""
    px = [U.rand_image(8600 + i, 40 + 3 * i, 70 - 4 * i, opaque=(i % 3 != 1)) for i in range(7)]
    stats = U.RareDiff()
    for direction in ("vertical", "horizontal"):
        s, _ = _stitch_against_reference(px, direction, {"mode": "max", "superSample": 2.2, "edgeAA": direction == "horizontal"}, ori=[2, 3, 4, 5, 6, 7, 8])
        stats.add(s)
    print("cubic orientations:", stats)
    stats.check()


@pytest.mark.parametrize("opts", [{"mode": "min"}, {"mode": "min", "platform": "android", "maxSide": 300, "superSample": 1}])
def test_a_shrinking_plan_is_area_byte_for_byte(opts):
    """no draw of these plans has an axis with |k| <= 1 other than the identity: 'cubic' is 'area' there"""
    px = [U.rand_image(8700 + i, h, w, opaque=(i != 1)) for i, (w, h) in enumerate([(600, 200), (1500, 700), (2400, 500), (600, 90)])]
    for direction in ("vertical", "horizontal"):
        imgs = [np.ascontiguousarray(a.transpose(1, 0, 2)) for a in px] if direction == "horizontal" else px
        p = ist.plan(U.hip_images(imgs), direction, opts)
        for r in p.rects:
            a = imgs[r["image"]]
            kx, ky = a.shape[1] / (r["dw"] * p.super_sample), a.shape[0] / (r["dh"] * p.super_sample)
            assert (kx > 1 and ky > 1) or (kx == 1 and ky == 1), (kx, ky)
        cubic = ist.stitch(U.hip_images(imgs), direction, dict(opts, filter="cubic"))["data"]
        area = ist.stitch(U.hip_images(imgs), direction, dict(opts, filter="area"))["data"]
        assert np.array_equal(cubic, area), (direction, U.max_abs_diff(cubic, area))


def test_identity_strips_move_the_same_bytes_and_keep_the_flat_form():
    """BASELINE configs[1] geometry (equal widths, vertical, 1:1) at reduced size: byte-identical under 'cubic' and 'bilinear', and the
    flat form of the copy path is launched for both"""
    st = ist.Stitcher(0)
    tall = [U.rand_image(8800 + k, h, 612) for k, h in enumerate((411, 289, 350))]
    outs = []
    for filt in ("bilinear", "cubic"):
        p, job = st.compile([{"width": 612, "height": a.shape[0], "opaque": True} for a in tall], "vertical", {"filter": filt})
        assert job.info["tiles_sample"] == 0 and job.info["tiles_general"] == 0, (filt, job.info)
        out = torch.full((p.canvas_h, p.canvas_w, 4), 0x5A, dtype=torch.uint8, device="cuda")
        before = L.lib.ist_debug_flat_launches()
        job.launch([torch.from_numpy(a).cuda() for a in tall], out)
        torch.cuda.synchronize()
        assert L.lib.ist_debug_flat_launches() == before + 1, filt
        outs.append(out.cpu().numpy())
        job.close()
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[1], np.concatenate(tall, 0))


# ------------------------------------------------------------------------------------------------ every entry point once
def _enlarging_request(seed, n=3, w=200):
    px = [U.rand_image(seed + i, 60 + 11 * i, w - 37 * i, opaque=(i != 1)) for i in range(n)]
    return px, "vertical", {"mode": "max", "filter": "cubic", "gap": 2}


def test_stitch_on_the_banded_host_path():
    """a canvas of 32 MB and more goes down band by band while later bands render (the duplex host path): every band uploads the
    source rows ist_shard_parts says it holds - under cubic, one row more at either end than under bilinear"""
    px = [U.rand_image(8900 + i, h, w) for i, (w, h) in enumerate([(1000, 900), (2048, 700), (700, 640)])]
    opts = {"mode": "max", "filter": "cubic"}
    p = ist.plan(U.hip_images(px), "vertical", opts)
    assert p.canvas_w * p.canvas_h * 4 >= 32 << 20
    stats = U.RareDiff()
    s, _ = _stitch_against_reference(px, "vertical", {"mode": "max"})
    stats.add(s)
    print("cubic banded host path:", stats)
    stats.check()


def test_png_batch_bitmap_and_group_entry_points_agree_with_stitch():
    px, direction, opts = _enlarging_request(9000)
    images = U.hip_images(px)
    want = ist.stitch(images, direction, opts)["data"]
    p = ist.plan(images, direction, opts)
    stats = U.RareDiff()
    stats.add(U.oracle_tolerance(want, R.render_ops(p.canvas_w, p.canvas_h, R.plan_ops(p), None, px, "cubic")))
    stats.check()
    # PNG export
    png = ist.stitch_png(images, direction, opts)
    assert np.array_equal(ist.decode_png(png["png"]), want)
    # batches with mixed filters in one call: every request equals its own stitch()
    px2, _, _ = _enlarging_request(9100, n=2, w=150)
    reqs = [(images, direction, opts), (U.hip_images(px2), "horizontal", {"mode": "max", "filter": "bilinear"}),
            (U.hip_images(px2), "vertical", {"mode": "min", "filter": "area"}), (U.hip_images(px2), "horizontal", {"mode": "max", "filter": "cubic", "superSample": 2.6}),
            (U.hip_images([px[0]]), "vertical", {"filter": "cubic"})]
    each = [ist.stitch(*r)["data"] for r in reqs]
    got = ist.stitch_batch(reqs)
    for k in range(len(reqs)):
        assert np.array_equal(got[k], each[k]), k
    files = ist.stitch_png_batch(reqs)
    for k in range(len(reqs)):
        assert np.array_equal(ist.decode_png(files[k]["png"]), each[k]), k
    # resident bitmaps
    bitmaps = [ist.upload_bitmap(im) for im in images]
    assert np.array_equal(ist.stitch(bitmaps, direction, opts)["data"], want)
    assert np.array_equal(ist.decode_png(ist.stitch_png(bitmaps, direction, opts)["png"]), want)
    # a device group on one GPU: canvas rows and images dealt to three slots
    for split in ("rows", "image"):
        many = ist.stitch(images, direction, dict(opts, devices=[0, 0, 0], split=split))["data"]
        assert np.array_equal(many, want), split


NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_node_stitch_with_filter_cubic(tmp_path):
    px, direction, opts = _enlarging_request(9200)
    imgs = []
    for i, a in enumerate(px):
        f = tmp_path / ("i%d.rgba" % i)
        np.ascontiguousarray(a).tofile(f)
        imgs.append({"width": a.shape[1], "height": a.shape[0], "file": str(f)})
    script = tmp_path / "cubic.js"
    script.write_text("""
const fs = require('fs'); const crypto = require('crypto');
const api = require(%s);
const imgs = JSON.parse(process.argv[2]).map((m) => ({width: m.width, height: m.height, data: fs.readFileSync(m.file)}));
const r = api.stitchSync(imgs, %s, %s);
console.log(JSON.stringify([r.width, r.height, crypto.createHash('sha256').update(r.data).digest('hex')]));
""" % (json.dumps(os.path.join(U.ROOT, "node", "index.js")), json.dumps(direction), json.dumps(opts)))
    r = subprocess.run([NODE, str(script), json.dumps(imgs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    w, h, digest = json.loads(r.stdout.strip().splitlines()[-1])
    want = ist.stitch(U.hip_images(px), direction, opts)["data"]
    assert (h, w) == want.shape[:2] and digest == hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()
