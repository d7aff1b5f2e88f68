"""The RGB PNG option in the Node host (opts.pngColor, setPngColor): stitchPng and stitchPngBatch with pngColor 'rgb' write the files
the CPU statement (tests/png_rgb_reference.py) predicts for the canvases the Python host stitches from the same images, and pngColor
'rgba' is the call without the option.  Reference anchor: the export step of onStitch (utils/canvas.js:205-242)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from tests import png_rgb_cases as K
from tests import png_rgb_reference as G
from tests import png_stream_cases as C
from tests import util as U

NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")]

SCRIPT = """
const fs = require('fs'); const path = require('path');
const api = require(%s);
const dir = process.argv[3];
const reqs = JSON.parse(fs.readFileSync(process.argv[2])).map((r) => ({direction: r.direction, opts: r.opts,
  images: r.images.map((m) => ({width: m.width, height: m.height, opaque: true, data: fs.readFileSync(m.file)}))}));
const put = (tag, x) => fs.writeFileSync(path.join(dir, tag + '.png'), x.png);
(async () => {
  const out = {};
  try { await api.stitchPng(reqs[0].images, reqs[0].direction, {pngColor: 'rgbx'}); out.unknown = 'resolved'; } catch (e) { out.unknown = e.constructor.name; }
  try { api.stitchPngBatchSync([{images: reqs[0].images, direction: 'vertical', opts: {pngColor: 'rgb'}}]); out.perRequest = 'ok'; } catch (e) { out.perRequest = e.constructor.name; }
  const r0 = reqs[0];
  put('plain', await api.stitchPng(r0.images, r0.direction, r0.opts));
  put('rgba', await api.stitchPng(r0.images, r0.direction, Object.assign({pngColor: 'rgba'}, r0.opts)));
  put('rgb', await api.stitchPng(r0.images, r0.direction, Object.assign({pngColor: 'rgb'}, r0.opts)));
  const batch = await api.stitchPngBatch(reqs, {pngLevel: 1, pngColor: 'rgb'});
  batch.forEach((x, k) => put('batch' + k, x));
  api.stitchPngBatchSync(reqs, {pngColor: 'rgba'}).forEach((x, k) => put('batchRgba' + k, x));
  api.stitchPngBatchSync(reqs).forEach((x, k) => put('batchPlain' + k, x));
  api.setPngColor('rgb');
  put('sticky', await api.stitchPng(r0.images, r0.direction, r0.opts));
  api.setPngColor('rgba');
  put('back', await api.stitchPng(r0.images, r0.direction, r0.opts));
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
"""


def test_node_stitch_png_and_batch_in_rgb(tmp_path):
    sizes = [((90, 60), (60, 90), (75, 50)), ((100, 130),), ((5462, 2),)]
    reqs, jreqs = [], []
    for r, shapes in enumerate(sizes):
        imgs = [{"width": w, "height": h, "data": K.opaque(C.photo_like(80 + 10 * r + k, h, w)), "opaque": True} for k, (w, h) in enumerate(shapes)]
        opts = {"gap": 3, "mode": "max"} if r == 0 else {}
        reqs.append((imgs, "vertical", opts))
        jimgs = []
        for k, im in enumerate(imgs):
            f = tmp_path / ("r%d_%d.rgba" % (r, k))
            np.ascontiguousarray(im["data"]).tofile(f)
            jimgs.append({"width": im["width"], "height": im["height"], "file": str(f)})
        jreqs.append({"images": jimgs, "direction": "vertical", "opts": opts})
    script = tmp_path / "png_rgb.js"
    script.write_text(SCRIPT % json.dumps(os.path.join(U.ROOT, "node", "index.js")))
    jp = tmp_path / "reqs.json"
    jp.write_text(json.dumps(jreqs))
    run = subprocess.run([NODE, str(script), str(jp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert json.loads(run.stdout.strip().splitlines()[-1]) == {"unknown": "TypeError", "perRequest": "TypeError"}
    read = lambda tag: open(tmp_path / (tag + ".png"), "rb").read()
    canvases = [np.ascontiguousarray(c) for c in ist.stitch_batch(reqs)]
    assert canvases[1].shape == (130, 100, 4) and canvases[2].shape == (2, 5462, 4)      # rows per chunk | pieces of a row
    want = [G.file_bytes_rgb(c, K.report("rgb node request %d" % k, c).stream) for k, c in enumerate(canvases)]
    assert read("rgb") == want[0] and read("sticky") == want[0]
    assert read("rgba") == read("plain") == read("back") and read("plain")[25] == 6
    assert np.array_equal(ist.decode_png(read("plain")), canvases[0])
    for k in range(3):
        assert read("batch%d" % k) == want[k], k
        assert read("batchRgba%d" % k) == read("batchPlain%d" % k) and read("batchPlain%d" % k)[25] == 6, k
        assert np.array_equal(ist.decode_png(read("batchPlain%d" % k)), canvases[k]), k
