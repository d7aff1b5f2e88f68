"""Resident bitmaps through the Node host (node/index.js Bitmap, decodeBitmaps, uploadBitmap) on the GPU: the same pixels as the host
images and as stitchFiles, memory that comes back on release() and on collection, and a stitch whose bitmaps are released before it
settles."""
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")]

JS = r"""
const api = require(process.argv[1]);
const fs = require('fs');
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const settle = async () => { for (let k = 0; k < 20; k++) { global.gc(); await new Promise((r) => setImmediate(r)); } };
(async () => {
  const base = api.debugBitmapBytes();
  // parity: stitch(decodeBitmaps(paths)) == stitch(decodeImage data with the same descs)
  const bms = await api.decodeBitmaps(job.paths);
  out.held = api.debugBitmapBytes() - base;
  out.desc = bms.map((b) => [b.width, b.height, b.orientation, b.opaque, b.fileSize]);
  const host = job.paths.map((p) => { const f = fs.readFileSync(p); return Object.assign(api.decodeImage(f), { fileSize: f.length }); });
  out.same = [];
  for (const [dir, opts] of job.layouts) {
    const a = await api.stitch(bms, dir, opts), b = await api.stitch(host, dir, opts), c = api.stitchSync(bms, dir, opts);
    out.same.push(a.width === b.width && a.height === b.height && a.data.equals(b.data) && c.data.equals(a.data));
  }
  // stitchPng from bitmaps; stitchFiles of the same paths (compared in Python, decoded)
  fs.writeFileSync(job.out + '.bitmaps.png', (await api.stitchPng(bms, 'vertical', {})).png);
  fs.writeFileSync(job.out + '.files.png', (await api.stitchFiles(job.paths, 'vertical', {})).png);
  out.downloadSame = bms.every((b, k) => b.download().equals(host[k].data));
  // upload round trip
  const up = api.uploadBitmap({ width: 5, height: 3, data: Buffer.from(job.small, 'base64'), orientation: 6, fileSize: 99 });
  out.up = [up.width, up.height, up.orientation, up.fileSize, up.download().toString('base64') === job.small];
  // released before the promise settles: the stitch still resolves to the right pixels
  const want = await api.stitch(bms, 'horizontal', { gap: 3 });
  const early = await api.decodeBitmaps(job.paths);
  const p = api.stitch(early, 'horizontal', { gap: 3 });
  early.forEach((b) => b.release());
  early.forEach((b) => b.release());                 // (again: nothing)
  const got = await p;
  out.early = got.data.equals(want.data);
  out.afterRelease = (() => { try { early[0].download(); return 'no error'; } catch (e) { return e.constructor.name; } })();
  out.stitchAfterRelease = await api.stitch(early, 'vertical').then(() => 'resolved', (e) => e.constructor.name);
  // release() and collection give the memory back
  bms.forEach((b) => b.release());
  up.release();
  await settle();
  out.afterRelease0 = api.debugBitmapBytes() - base;
  let dropped = await api.decodeBitmaps(job.paths);
  out.held2 = api.debugBitmapBytes() - base;
  dropped = null;
  await settle();
  out.afterGc = api.debugBitmapBytes() - base;
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""


def _save(im, fmt, **kw):
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


def test_node_bitmaps_match_the_host_images_and_stitch_files(tmp_path):
    photos = [U.smooth_image(40 + k, 90 + 13 * k, 120 - 7 * k) for k in range(4)]
    files = [_save(Image.fromarray(photos[0][..., :3]), "JPEG", quality=90),
             _save(Image.fromarray(photos[1], "RGBA"), "PNG"),
             _save(Image.fromarray(photos[2][..., :3]), "JPEG", quality=85, progressive=True),
             _save(Image.fromarray(photos[3][..., :3]), "WEBP", lossless=True)]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d" % k)))
        open(paths[-1], "wb").write(f)
    small = U.rand_image(7, 3, 5, opaque=False)
    import base64
    job = {"paths": paths, "out": str(tmp_path / "r"), "small": base64.b64encode(small.tobytes()).decode(),
           "layouts": [["vertical", {}], ["horizontal", {"gap": 4, "mode": "max"}], ["vertical", {"filter": "area", "platform": "ios"}]]}
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, "--expose-gc", "-e", JS, os.path.join(ROOT, "node", "index.js"), str(tmp_path / "job.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    blocks = sum(((Image.open(io.BytesIO(f)).size[0] * 4 * Image.open(io.BytesIO(f)).size[1] + 256 + 255) & ~255) for f in files)
    assert out["held"] == blocks and out["held2"] == blocks
    assert [d[4] for d in out["desc"]] == [len(f) for f in files]
    assert [d[3] for d in out["desc"]] == [True, False, True, False]
    assert out["same"] == [True, True, True]
    assert out["downloadSame"]
    assert out["up"] == [5, 3, 6, 99, True]
    assert out["early"] and out["afterRelease"] == "Error" and out["stitchAfterRelease"] == "Error"
    assert out["afterRelease0"] == 0 and out["afterGc"] == 0
    a = np.asarray(Image.open(str(tmp_path / "r.bitmaps.png")).convert("RGBA"))
    b = np.asarray(Image.open(str(tmp_path / "r.files.png")).convert("RGBA"))
    assert np.array_equal(a, b)
