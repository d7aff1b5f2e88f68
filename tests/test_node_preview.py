"""Previews through the Node host (node/index.js: stitchPng / stitchFiles with opts.preview, Bitmap.preview) on the GPU: the file is
the one the call without the option resolves, the preview is the oracle's area shrink of the file's own pixels (the redraw into the
preview node, pages/index/index.js:1597-1603), and the calls that keep no canvas behind an export refuse the option."""
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from oracle import oracle as O
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
const name = async (p) => { try { await p; return 'resolved'; } catch (e) { return e.constructor.name; } };
const put = (tag, r) => {
  fs.writeFileSync(job.out + '.' + tag + '.png', r.png);
  fs.writeFileSync(job.out + '.' + tag + '.rgba', r.preview.data);
  out[tag] = [r.width, r.height, r.preview.width, r.preview.height, r.preview.data.length];
};
(async () => {
  const box = { width: 343, height: 457 };
  const host = job.paths.map((p) => { const f = fs.readFileSync(p); return Object.assign(api.decodeImage(f), { fileSize: f.length }); });
  const bms = await api.decodeBitmaps(job.paths);
  for (const dir of ['vertical', 'horizontal']) {
    const plain = await api.stitchPng(host, dir, { gap: 5 });
    out['noPreview_' + dir] = plain.preview === undefined;
    const a = await api.stitchPng(host, dir, { gap: 5, preview: box });
    out['samePng_' + dir] = a.png.equals(plain.png);
    put('host_' + dir, a);
    const b = await api.stitchPng(bms, dir, { gap: 5, preview: box });
    out['samePngBitmaps_' + dir] = b.png.equals((await api.stitchPng(bms, dir, { gap: 5 })).png);
    put('bitmaps_' + dir, b);
    const c = await api.stitchFiles(job.paths, dir, { gap: 5, preview: box });
    out['samePngFiles_' + dir] = c.png.equals((await api.stitchFiles(job.paths, dir, { gap: 5 })).png);
    put('files_' + dir, c);
  }
  const t = bms[0].preview(64, 64);
  fs.writeFileSync(job.out + '.thumb.rgba', t.data);
  fs.writeFileSync(job.out + '.thumb.full', bms[0].download());
  out.thumb = [bms[0].bmpWidth, bms[0].bmpHeight, t.width, t.height, t.data.length];
  // refusals
  out.stitch = await name(api.stitch(host, 'vertical', { preview: box }));
  out.stitchSync = (() => { try { api.stitchSync(host, 'vertical', { preview: box }); return 'no error'; } catch (e) { return e.constructor.name; } })();
  out.batch = await name(api.stitchPngBatch([{ images: host, direction: 'vertical', opts: { preview: box } }]));
  out.devices = await name(api.stitchPng(host, 'vertical', { preview: box, devices: [0] }));
  out.shape = await name(api.stitchPng(host, 'vertical', { preview: 343 }));
  out.badBox = await api.stitchPng(host, 'vertical', { preview: { width: 0, height: 457 } }).then(() => 'resolved', (e) => e.code);
  out.badThumb = (() => { try { bms[0].preview(-1, 5); return 'no error'; } catch (e) { return e.constructor.name; } })();
  bms.forEach((b) => b.release());
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""


def _save(im, fmt, **kw):
    b = io.BytesIO()
    im.save(b, fmt, **kw)
    return b.getvalue()


def _oracle_preview(img, pw, ph):
    h, w = img.shape[:2]
    draw = {"kind": "draw", "image": 0, "m": [1, 0, 0, 1, 0, 0], "s": [0, 0, w, h], "d": [0, 0, pw, ph]}
    return O.render_ops(pw, ph, [draw], [{"width": w, "height": h}], [img], filter="area", clear=(0, 0, 0, 0))


def test_node_previews_match_the_oracle_and_leave_the_file_alone(tmp_path):
    photos = [U.smooth_image(50 + k, 700 + 31 * k, 900 - 17 * k) for k in range(3)]
    files = [_save(Image.fromarray(photos[0][..., :3]), "JPEG", quality=90),
             _save(Image.fromarray(photos[1], "RGBA"), "PNG"),
             _save(Image.fromarray(photos[2][..., :3]), "JPEG", quality=85, progressive=True)]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d" % k)))
        open(paths[-1], "wb").write(f)
    job = {"paths": paths, "out": str(tmp_path / "r")}
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, "-e", JS, os.path.join(ROOT, "node", "index.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for d in ("vertical", "horizontal"):
        assert out["noPreview_" + d] and out["samePng_" + d] and out["samePngBitmaps_" + d] and out["samePngFiles_" + d], d
        for tag in ("host_", "bitmaps_", "files_"):
            w, h, pw, ph, n = out[tag + d]
            canvas = np.asarray(Image.open(str(tmp_path / ("r.%s%s.png" % (tag, d)))).convert("RGBA"))
            assert canvas.shape == (h, w, 4) and (pw, ph) == ist.preview_fit(w, h, 343, 457) and n == pw * ph * 4
            got = np.frombuffer(open(str(tmp_path / ("r.%s%s.rgba" % (tag, d))), "rb").read(), np.uint8).reshape(ph, pw, 4)
            U.oracle_tolerance(got, _oracle_preview(canvas, pw, ph))
    bw, bh, tw, th, n = out["thumb"]
    assert (tw, th) == ist.preview_fit(bw, bh, 64, 64) and n == tw * th * 4
    full = np.frombuffer(open(str(tmp_path / "r.thumb.full"), "rb").read(), np.uint8).reshape(bh, bw, 4)
    thumb = np.frombuffer(open(str(tmp_path / "r.thumb.rgba"), "rb").read(), np.uint8).reshape(th, tw, 4)
    U.oracle_tolerance(thumb, _oracle_preview(full, tw, th))
    assert out["stitch"] == "TypeError" and out["stitchSync"] == "TypeError" and out["batch"] == "TypeError"
    assert out["devices"] == "TypeError" and out["shape"] == "TypeError"
    assert out["badBox"] == "-1" and out["badThumb"] == "Error"
