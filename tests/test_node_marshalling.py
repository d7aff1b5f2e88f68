"""The Node addon's marshalling rules (node/addon.c: bytes_of, images_parse, images_missing, files_parse, bitmaps_parse), on the native
functions, without a device.  Every entry marshals before it asks for its context, and without a device a call that gets past
marshalling fails with code '-5' (IST_E_NO_DEVICE): the exception type of each case below is therefore also the proof of that order.
Each test is one node process that prints JSON.  The gpu-marked test at the end runs every job kind through its Promise and through
its synchronous twin."""
import base64
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests.test_node_host import NODE, ROOT, needs_node

pytestmark = needs_node

PRELUDE = r"""
const api = require(process.argv[1]);
const N = api.native;
const arg = process.argv[2] ? JSON.parse(process.argv[2]) : {};
const S = [0, 0, 0, null, 1];                                    // direction, mode, gap, limits, filter
const OK = () => ({ width: 2, height: 2, data: new Uint8Array(16) });
const REQUESTS = {                                               // every entry whose image pixels have to be there
  stitch: (im) => N.stitch([im], ...S),
  stitchSync: (im) => N.stitchSync([im], ...S),
  stitchBatch: (im) => N.stitchBatch([[[im], ...S]]),
  stitchBatchSync: (im) => N.stitchBatchSync([[[im], ...S]]),
  stitchPngBatch: (im) => N.stitchPngBatch([[[im], ...S]]),
  stitchPngBatchSync: (im) => N.stitchPngBatchSync([[[im], ...S]]),
  stitchJpegBatch: (im) => N.stitchJpegBatch([[[im], ...S, 90, 1]]),
  stitchJpegBatchSync: (im) => N.stitchJpegBatchSync([[[im], ...S, 90, 1]]),
  uploadBitmap: (im) => N.uploadBitmap([im]),
};
const render = (im, ops, region) => N.render(2, 2, new Uint8Array(4), ops || new Float64Array(18), [im], 1, region || null);
const PIXELS = Object.assign({ render }, REQUESTS);              // every entry that takes image pixels
// how a call ends: thrown on this thread, a rejected / resolved Promise, or a plain return
async function outcome(f) {
  const err = (how, e) => ({ how, type: e && e.constructor && e.constructor.name, message: String(e && e.message), code: e && e.code });
  let p;
  try { p = f(); } catch (e) { return err('threw', e); }
  if (!p || typeof p.then !== 'function') return { how: 'returned' };
  try { await p; return { how: 'resolved' }; } catch (e) { return err('rejected', e); }
}
async function table(entries, inputs) {
  const out = {};
  for (const [name, call] of Object.entries(entries)) for (const [tag, make] of Object.entries(inputs)) out[name + ' / ' + tag] = await outcome(() => call(make()));
  return out;
}
const main = (f) => f().then((r) => console.log(JSON.stringify(r)), (e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""

ASYNC = {"stitch", "stitchBatch", "stitchPngBatch", "stitchJpegBatch"}
REQUESTS = sorted(ASYNC | {"stitchSync", "stitchBatchSync", "stitchPngBatchSync", "stitchJpegBatchSync", "uploadBitmap"})
PIXELS = sorted(REQUESTS + ["render"])


def _node(body, arg=None):
    r = subprocess.run([NODE, "-e", PRELUDE + body, os.path.join(ROOT, "node", "index.js"), json.dumps(arg or {})], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _file(fmt):
    buf = io.BytesIO()
    Image.fromarray(np.full((8, 8, 3), 90, np.uint8)).save(buf, fmt)
    return base64.b64encode(buf.getvalue()).decode()


def test_image_data_that_is_not_bytes_is_a_type_error():
    out = _node(r"""
main(() => table(PIXELS, {
  Float32Array: () => ({ width: 2, height: 2, data: new Float32Array(16) }),
  Uint16Array: () => ({ width: 2, height: 2, data: new Uint16Array(16) }),
  DataView: () => ({ width: 2, height: 2, data: new DataView(new ArrayBuffer(16)) }),
  string: () => ({ width: 2, height: 2, data: 'x'.repeat(16) }),
}));""")
    assert sorted(out) == sorted("%s / %s" % (e, t) for e in PIXELS for t in ("Float32Array", "Uint16Array", "DataView", "string"))
    for case, o in out.items():          # thrown on the caller's thread, by the asynchronous entries too
        assert (o["how"], o["type"], o["message"]) == ("threw", "TypeError", "image data must be a Uint8Array / Buffer"), case


def test_image_data_smaller_than_the_stored_size_is_a_range_error():
    out = _node(r"""
main(() => table(PIXELS, {
  short: () => ({ width: 2, height: 2, data: new Uint8Array(15) }),
  bmpWidth: () => ({ width: 2, height: 2, bmpWidth: 9, data: new Uint8Array(16) }),
  clamped: () => ({ width: 2, height: 2, data: new Uint8ClampedArray(15) }),
  buffer: () => ({ width: 2, height: 2, data: Buffer.alloc(15) }),
}));""")
    assert len(out) == 4 * len(PIXELS)
    for case, o in out.items():
        assert (o["how"], o["type"], o["message"]) == ("threw", "RangeError", "image data is smaller than width*height*4"), case


def test_missing_pixels_are_the_decode_failure():
    out = _node(r"""
main(() => table(REQUESTS, {
  absent: () => ({ width: 2, height: 2 }),
  null: () => ({ width: 2, height: 2, data: null }),
  undefined: () => ({ width: 2, height: 2, data: undefined }),
}));""")
    assert len(out) == 3 * len(REQUESTS)
    for case, o in out.items():
        entry = case.split(" / ")[0]
        assert o["how"] == ("rejected" if entry in ASYNC else "threw"), case
        assert o.get("code") == "-6" and o["message"] == "拼图失败：" + ("request 0: " if "Batch" in entry else "") + "图片0解码异常", case


BYTES = r"""
const BYTES = {
  encodePng: (x) => N.encodePng(x, 2, 2),
  encodeJpeg: (x) => N.encodeJpeg(x, 2, 2, 90, 1),
  decodeImage: (x) => N.decodeImage(x),
  decodePng: (x) => N.decodePng(x),
  stitchFiles: (x) => N.stitchFiles([x], ...S),
  decodeBitmaps: (x) => N.decodeBitmaps([x]),
};
"""
MESSAGES = {"encodePng": "encodePng expects a Buffer / Uint8Array", "encodeJpeg": "encodeJpeg expects a Buffer / Uint8Array",
            "decodeImage": "decodeImage expects a Buffer / Uint8Array", "decodePng": "decodePng expects a Buffer / Uint8Array",
            "stitchFiles": "files[i] must be a Buffer / Uint8Array", "decodeBitmaps": "files[i] must be a Buffer / Uint8Array"}


def test_byte_arguments_that_are_not_bytes_are_a_type_error():
    out = _node(BYTES + r"""
main(() => table(BYTES, {
  string: () => 'x'.repeat(64),
  Float64Array: () => new Float64Array(8),
  DataView: () => new DataView(new ArrayBuffer(64)),
  null: () => null,
  object: () => ({ length: 64 }),
}));""")
    assert len(out) == 5 * len(MESSAGES)
    for case, o in out.items():
        assert (o["how"], o["type"], o["message"]) == ("threw", "TypeError", MESSAGES[case.split(" / ")[0]]), case


def test_pixels_too_short_for_an_encoder_are_a_range_error():
    out = _node(BYTES + r"""
main(() => table({ encodePng: BYTES.encodePng, encodeJpeg: BYTES.encodeJpeg }, {
  Uint8Array: () => new Uint8Array(15), clamped: () => new Uint8ClampedArray(15), buffer: () => Buffer.alloc(15), empty: () => new Uint8Array(0),
}));""")
    assert len(out) == 8
    for case, o in out.items():
        assert (o["how"], o["type"], o["message"]) == ("threw", "RangeError", "data is smaller than width*height*4"), case


def test_the_other_refusals_are_what_they_were():
    out = _node(r"""
main(async () => ({
  images: await outcome(() => N.stitchSync(5, ...S)),
  request: await outcome(() => N.stitchBatchSync([[[OK()], 0, 0, 0, null]])),
  requestAsync: await outcome(() => N.stitchJpegBatch([[[OK()], 0, 0, 0, null]])),
  twoImages: await outcome(() => N.uploadBitmap([OK(), OK()])),
  desc: await outcome(() => N.bitmapDesc({})),
  thumbnails: await outcome(() => N.thumbnails([{}], 2, 2, 0, true)),
  stitchBitmaps: await outcome(() => N.stitchBitmaps([{}], ...S)),
  ops: await outcome(() => render(OK(), new Float64Array(17))),
  region: await outcome(() => render(OK(), null, { x: 0, y: 0, w: 0, h: 1 })),
  devices: await outcome(() => N.stitchSync([OK()], ...S, false, new Array(65).fill(0), 0)),
  level: await outcome(() => N.setPngLevel('x')),
  color: await outcome(() => N.setPngColor('x')),
}));""")
    want = {"images": ("TypeError", "images must be an array"),
            "request": ("TypeError", "stitchBatch: requests[k] must be [images, direction, mode, gap, limits, filter]"),
            "requestAsync": ("TypeError", "stitchBatch: requests[k] must be [images, direction, mode, gap, limits, filter]"),
            "twoImages": ("TypeError", "uploadBitmap takes one image"),
            "desc": ("TypeError", "not a Bitmap handle"), "thumbnails": ("TypeError", "not a Bitmap handle"), "stitchBitmaps": ("TypeError", "not a Bitmap handle"),
            "ops": ("TypeError", "ops must be a Float64Array with 18 doubles per op"), "region": ("RangeError", "empty region"),
            "devices": ("RangeError", "devices: at most 64 entries"),
            "level": ("TypeError", "setPngLevel(level)"), "color": ("TypeError", "setPngColor(color)")}
    assert sorted(out) == sorted(want)
    for case, o in out.items():
        assert (o["how"], o["type"], o["message"]) == ("threw",) + want[case], case


def test_well_formed_calls_get_as_far_as_the_context():
    """the other half of the proof: a well-formed call gets past marshalling (no device here: -5; with one, the call succeeds)"""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out = _node(BYTES + r"""
const file = (k) => Buffer.from(arg[k], 'base64');
main(async () => Object.assign(await table(PIXELS, { ok: OK, clamped: () => ({ width: 2, height: 2, data: new Uint8ClampedArray(16) }), buffer: () => ({ width: 2, height: 2, data: Buffer.alloc(16) }) }), {
  encodePng: await outcome(() => N.encodePng(new Uint8Array(16), 2, 2)),
  encodeJpeg: await outcome(() => N.encodeJpeg(new Uint8ClampedArray(16), 2, 2, 90, 1)),
  decodeImage: await outcome(() => N.decodeImage(file('jpeg'))),
  stitchFiles: await outcome(() => N.stitchFiles([file('png'), new Uint8Array(file('jpeg'))], ...S)),
  decodeBitmaps: await outcome(() => N.decodeBitmaps([file('png')])),
  stitchBitmaps: await outcome(() => N.stitchBitmaps([null], ...S)),
  stitchBitmapsSync: await outcome(() => N.stitchBitmapsSync([null], ...S)),
  thumbnails: await outcome(() => N.thumbnails([null], 2, 2, 0, true)),
  renderNoPixels: await outcome(() => render({ width: 2, height: 2 })),
  setPngLevel: await outcome(() => N.setPngLevel(1)),
  decodePng: await outcome(() => N.decodePng(file('png'))),
  decodeImagePng: await outcome(() => N.decodeImage(file('png'))),
}));""", {"png": _file("PNG"), "jpeg": _file("JPEG")})
    assert len(out) == 3 * len(PIXELS) + 12
    promises = ASYNC | {"stitchFiles", "decodeBitmaps", "stitchBitmaps", "thumbnails"}
    for case, o in out.items():
        entry = case.split(" / ")[0]
        if entry in ("decodePng", "decodeImagePng"):                  # a PNG is decoded on the host: no context is asked for
            assert o["how"] == "returned", case
            continue
        assert o["how"] == ("rejected" if entry in promises else "threw") and o.get("code") == "-5" and o["message"].startswith("拼图失败："), (case, o)


@pytest.mark.gpu
def test_every_job_settles_like_its_synchronous_twin():
    """stitch, stitchBitmaps and the three batches, awaited one after another, against their ...Sync twins: the same bytes and plans,
    null for an empty request in both, -6 for a missing image, and no bitmap bytes left once every Bitmap is released"""
    out = _node(r"""
const assert = require('assert');
const image = (w, h, seed) => { const data = new Uint8Array(w * h * 4); for (let i = 0; i < data.length; i++) data[i] = (i * 37 + seed * 101 + (i >> 5) * 13) & 255; return { width: w, height: h, data }; };
const ims = [image(8, 6, 1), image(5, 7, 2)];
const KEYS = ['data', 'png', 'jpeg'];
// a result and its twin: the same shape, the same bytes under the one key it has, the same plan
function same(a, b, key) {
  if (a === null || b === null) return a === b;
  assert.deepStrictEqual(KEYS.filter((k) => k in a), [key]);
  assert.deepStrictEqual(KEYS.filter((k) => k in b), [key]);
  assert.deepStrictEqual(a.plan, b.plan);
  return a.width === b.width && a.height === b.height && a.width === a.plan.canvasW && a[key].length > 0 && Buffer.compare(a[key], b[key]) === 0;
}
main(async () => {
  const out = { same: {}, widths: {} };
  const EXPORTS = { data: false, png: true, jpeg: { quality: 90, subsampling: 1 } };
  for (const [key, as] of Object.entries(EXPORTS)) {
    const a = await N.stitch(ims, ...S, as), b = N.stitchSync(ims, ...S, as);
    out.same['stitch ' + key] = same(a, b, key);
    out.widths['stitch ' + key] = [a.width, a.height, key === 'data' ? a.data.length : 0];
  }
  const hs = ims.map((im) => N.uploadBitmap([im]));
  out.bytesHeld = N.debugBitmapBytes();
  for (const [key, as] of Object.entries(EXPORTS)) {
    const a = await N.stitchBitmaps(hs, ...S, as), b = N.stitchBitmapsSync(hs, ...S, as);
    out.same['stitchBitmaps ' + key] = same(a, b, key) && same(a, N.stitchSync(ims, ...S, as), key);
  }
  const reqs = (tail) => [[ims, ...S, ...tail], [[], ...S, ...tail], [[ims[1]], 1, 0, 2, null, 1, ...tail]];
  const BATCHES = { data: ['stitchBatch', []], png: ['stitchPngBatch', []], jpeg: ['stitchJpegBatch', [90, 1]] };
  for (const [key, [name, tail]] of Object.entries(BATCHES)) {
    const a = await N[name](reqs(tail)), b = N[name + 'Sync'](reqs(tail));
    out.same[name] = a.length === 3 && b.length === 3 && a.every((x, k) => same(x, b[k], key));
    out[name + ' nulls'] = [a.map((x) => x === null), b.map((x) => x === null)];
    out.same[name + ' is stitch'] = same(a[0], N.stitchSync(ims, ...S, EXPORTS[key]), key);
  }
  out.missing = await outcome(() => N.stitch([ims[0], { width: 5, height: 7 }], ...S));
  hs.forEach((h) => N.bitmapRelease(h));
  out.bytesLeft = N.debugBitmapBytes();
  return out;
});""")
    assert len(out["same"]) == 12 and all(out["same"].values()), out["same"]
    w, h, n = out["widths"]["stitch data"]
    assert w == 5 and n == w * h * 4 and out["widths"]["stitch png"][:2] == [w, h] and out["widths"]["stitch jpeg"][:2] == [w, h]
    for name in ("stitchBatch", "stitchPngBatch", "stitchJpegBatch"):
        assert out[name + " nulls"] == [[False, True, False]] * 2
    m = out["missing"]
    assert (m["how"], m["code"], m["message"]) == ("rejected", "-6", "拼图失败：图片1解码异常")
    assert out["bytesHeld"] > 0 and out["bytesLeft"] == 0
