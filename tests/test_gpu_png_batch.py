"""Batched PNG export on the GPU (ist_stitch_png_batch / stitch_png_batch, ist_png_encode_batch_device / encode_png_batch_device,
the Node stitchPngBatch): every file of a batch is the export step of one unchanged onStitch (pages/index/index.js:1577-1579), so
its zlib stream must be byte for byte what the single-file encoder gives for the same canvas (IDAT chunk boundaries may differ),
and it must decode to exactly the canvas stitch_batch renders for the request."""
import ctypes as C
import io
import json
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from imagestitching_amd.stitch import _batch_requests, _ctx_png
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = (0, 1)


def _chunks(png):
    """(IHDR data, concatenated IDAT data); every chunk's CRC checked"""
    png = bytes(png)
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    at, ihdr, idat, names = 8, None, b"", []
    while at < len(png):
        n, = struct.unpack(">I", png[at:at + 4])
        kind, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", png[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data) & 0xFFFFFFFF, (kind, at)
        names.append(kind)
        if kind == b"IHDR":
            ihdr = data
        elif kind == b"IDAT":
            idat += data
        at += 12 + n
    assert at == len(png) and names[-1] == b"IEND"
    return ihdr, idat


def _decode(png):
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(png)))
    assert im.mode == "RGBA"
    return np.asarray(im)


def _flat(seed, h, w):
    """screenshot-like: a few flat colour bands"""
    rng = np.random.default_rng(seed)
    a = np.empty((h, w, 4), np.uint8)
    cuts = sorted(int(v) for v in rng.integers(0, h, 3))
    for k, (y0, y1) in enumerate(zip([0] + cuts, cuts + [h])):
        a[y0:y1] = rng.integers(0, 256, 4, dtype=np.uint8) | np.array([0, 0, 0, 255], np.uint8)
    return a


def _img(a, opaque=True):
    return {"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": opaque}


def _requests(seed):
    """seeded random requests with the shapes the encoder splits differently: 1x1, rows longer than one 16 KiB chunk (pieces of a
    row), more than 65535 rows, translucent pixels, flat content, and requests without images"""
    rng = np.random.default_rng(seed)
    reqs = [([_img(U.rand_image(seed, 1, 1))], "vertical"),
            ([_img(U.rand_image(seed + 1, 3, 4200)), _img(U.rand_image(seed + 2, 2, 4200))], "vertical", {"filter": "nearest"}),
            ([_img(U.smooth_image(seed + 3, 22000 + k, 6)) for k in range(3)], "vertical"),
            ([], "horizontal"),
            ([_img(U.rand_image(seed + 4, 40, 50, opaque=False), False), _img(U.rand_image(seed + 5, 30, 70, opaque=False), False)],
             "horizontal", {"gap": 3}),
            ([_img(_flat(seed + 6, 900, 600)), _img(_flat(seed + 7, 500, 600))], "vertical")]
    for k in range(int(rng.integers(3, 7))):
        n = int(rng.integers(1, 5))
        px = [U.smooth_image(seed * 100 + 10 * k + i, int(rng.integers(5, 300)), int(rng.integers(5, 300)), opaque=bool(rng.random() < 0.7))
              for i in range(n)]
        reqs.append(([_img(a, bool(a[..., 3].min() == 255)) for a in px], str(rng.choice(["vertical", "horizontal"])),
                     {"filter": str(rng.choice(["nearest", "bilinear", "area"])), "mode": str(rng.choice(["min", "max", "original"])),
                      "gap": int(rng.choice([0, 4]))}))
    order = rng.permutation(len(reqs))
    return [reqs[i] for i in order]


def _check_against_loop(reqs, got, level, canvases=None):
    canvases = canvases if canvases is not None else ist.stitch_batch(reqs)
    assert len(got) == len(reqs)
    for k, r in enumerate(reqs):
        if not r[0]:
            assert got[k] is None and canvases[k] is None, k
            continue
        want = ist.stitch_png(*r[:2], dict(r[2], pngLevel=level) if len(r) == 3 else {"pngLevel": level})
        assert (got[k]["width"], got[k]["height"]) == (want["width"], want["height"]), k
        gi, gz = _chunks(got[k]["png"])
        wi, wz = _chunks(want["png"])
        assert gi == wi, k
        assert gz == wz, (k, len(gz), len(wz))
        assert np.array_equal(_decode(got[k]["png"]), canvases[k]), k


@pytest.mark.parametrize("level", LEVELS)
def test_stitch_png_batch_equals_the_loop(level):
    for seed in (3, 17):
        reqs = _requests(seed + level)
        assert any(len(r[0]) and sum(im["height"] for im in r[0]) > 65535 for r in reqs)
        got = ist.stitch_png_batch(reqs, level=level)
        _check_against_loop(reqs, got, level)


@pytest.mark.parametrize("level", LEVELS)
def test_encode_png_batch_device_equals_encode_png_device(level):
    rng = np.random.default_rng(5 + level)
    shapes = [(1, 1), (7, 4200), (300, 257), (66000, 3), (64, 64)]
    cans = []
    for k, (h, w) in enumerate(shapes):
        pad = int(rng.choice([0, 16, 4 * 13]))
        raw = torch.full((h, w * 4 + pad), 0xEE, dtype=torch.uint8, device=DEV)
        a = U.rand_image(40 + k, h, w, opaque=bool(k % 2)) if k != 4 else _flat(9, h, w)
        raw[:, :w * 4] = torch.from_numpy(a.reshape(h, w * 4)).to(DEV)
        cans.append((raw[:, :w * 4].view(h, w, 4), a))
    before = L.lib.ist_debug_png_batch_launches()
    files = ist.encode_png_batch_device([c for c, _ in cans], level=level)
    assert L.lib.ist_debug_png_batch_launches() == before + 1
    for k, ((c, a), (t, n)) in enumerate(zip(cans, files)):
        one, m = ist.encode_png_device(c, level=level)
        got, want = t.cpu().numpy().tobytes(), one.cpu().numpy().tobytes()
        assert n == len(got) and m == len(want)
        assert _chunks(got)[1] == _chunks(want)[1], k
        assert got == want, k                               # (one slab, one IDAT on both sides: the files are the same)
        assert np.array_equal(_decode(got), a), k


@pytest.mark.parametrize("level", LEVELS)
def test_one_compression_launch_per_sub_batch(level):
    reqs = _requests(29)[:5]
    before = L.lib.ist_debug_png_batch_launches()
    ist.stitch_png_batch([r for r in reqs if r[0]] or reqs, level=level)
    assert L.lib.ist_debug_png_batch_launches() == before + 1
    # sources + canvas + file (+ chunk slots) of these requests are ~200-400 MiB each: more than one 512 MiB sub-batch
    big = np.tile(U.smooth_image(77, 512, 2048), (16, 1, 1))
    reqs = [([_img(big)], "vertical"), ([_img(big[::-1].copy())], "vertical"), ([], "vertical"), ([_img(big[:6000])], "horizontal")]
    before = L.lib.ist_debug_png_batch_launches()
    got = ist.stitch_png_batch(reqs, level=level)
    launches = L.lib.ist_debug_png_batch_launches() - before
    assert launches >= 2, launches
    _check_against_loop(reqs, got, level)


def test_a_failing_request_fails_the_whole_batch_and_the_next_one_succeeds():
    reqs = _requests(41)
    live = [k for k, r in enumerate(reqs) if r[0]]
    creqs, keep = _batch_requests(reqs, "")
    bad = live[len(live) // 2]
    creqs[bad].src[0] = None                                # request `bad`: its first image has no buffer
    n = len(reqs)
    plans, outs, lens = (L.Plan * n)(), (C.POINTER(C.c_uint8) * n)(), (C.c_int64 * n)()
    ctx = _ctx_png(0, 1)
    rc = L.lib.ist_stitch_png_batch(ctx, creqs, n, plans, outs, lens)
    assert rc == -6 and ("request %d" % bad) in L.last_error(), (rc, L.last_error())
    assert all(not outs[k] for k in range(n)) and all(lens[k] == 0 for k in range(n))
    assert all(plans[k].canvas_w == 0 and not plans[k].rects for k in range(n))
    got = ist.stitch_png_batch(reqs, level=1)
    _check_against_loop(reqs, got, 1)


@pytest.mark.parametrize("level", LEVELS)
def test_a_second_identical_batch_allocates_nothing(level):
    reqs = _requests(53)
    ist.stitch_png_batch(reqs, level=level)
    before = L.lib.ist_debug_device_allocs()
    got = ist.stitch_png_batch(reqs, level=level)
    assert L.lib.ist_debug_device_allocs() == before
    assert all((g is None) == (not r[0]) for g, r in zip(got, reqs))


NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
@pytest.mark.parametrize("level", LEVELS)
def test_node_stitch_png_batch_equals_stitch_png(tmp_path, level):
    reqs = [r for r in _requests(61) if not r[0] or sum(im["height"] for im in r[0]) < 20000]
    jreqs = []
    for k, r in enumerate(reqs):
        imgs = []
        for i, im in enumerate(r[0]):
            f = tmp_path / ("r%d_%d.rgba" % (k, i))
            np.ascontiguousarray(im["data"]).tofile(f)
            imgs.append({"width": im["width"], "height": im["height"], "opaque": im["opaque"], "file": str(f)})
        jreqs.append({"images": imgs, "direction": r[1], "opts": dict(r[2]) if len(r) == 3 else {}})
    script = tmp_path / "png_batch.js"
    script.write_text("""
const fs = require('fs'); const path = require('path');
const api = require(%s);
const dir = process.argv[3];
const reqs = JSON.parse(fs.readFileSync(process.argv[2])).map((r) => ({direction: r.direction, opts: r.opts,
  images: r.images.map((m) => ({width: m.width, height: m.height, opaque: m.opaque, data: fs.readFileSync(m.file)}))}));
(async () => {
  api.setPngLevel(%d);
  const sync = api.stitchPngBatchSync(reqs);
  const prom = await api.stitchPngBatch(reqs);
  const out = [];
  for (let k = 0; k < reqs.length; k++) {
    const one = reqs[k].images.length ? await api.stitchPng(reqs[k].images, reqs[k].direction, reqs[k].opts) : null;
    for (const [tag, x] of [['sync', sync[k]], ['prom', prom[k]], ['one', one]]) if (x) fs.writeFileSync(path.join(dir, tag + k + '.png'), x.png);
    out.push([sync[k] === null, prom[k] === null, one === null]);
  }
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
""" % (json.dumps(os.path.join(U.ROOT, "node", "index.js")), level))
    jp = tmp_path / "reqs.json"
    jp.write_text(json.dumps(jreqs))
    r = subprocess.run([NODE, str(script), str(jp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    nulls = json.loads(r.stdout.strip().splitlines()[-1])
    for k, rq in enumerate(reqs):
        assert nulls[k] == [not rq[0]] * 3, k
        if not rq[0]:
            continue
        one = _chunks((tmp_path / ("one%d.png" % k)).read_bytes())
        for tag in ("sync", "prom"):
            assert _chunks((tmp_path / ("%s%d.png" % (tag, k))).read_bytes()) == one, (tag, k)
