"""The PNG window-match option in the Node host (opts.pngMatch, setPngMatch): stitchPng, stitchPngBatch and encodePng with pngMatch
'window' write the files the CPU statement (tests/png_match_reference.py) predicts for the canvases the Python host stitches from
the same images - the files the Python host writes - and pngMatch 'run' is the call without the option.  Reference anchor: the export
step of onStitch (utils/canvas.js:205-242)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from tests import png_deflate_reference as R
from tests import png_match_cases as K
from tests import png_match_reference as M
from tests import png_rgb_cases as KR
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
const put = (tag, x) => fs.writeFileSync(path.join(dir, tag + '.png'), x.png || x);
const kind = (f) => { try { f(); return 'ok'; } catch (e) { return e.constructor.name; } };
(async () => {
  const out = {};
  try { await api.stitchPng(reqs[0].images, reqs[0].direction, {pngMatch: 'lz77'}); out.unknown = 'resolved'; } catch (e) { out.unknown = e.constructor.name; }
  try { await api.stitchPngBatch(reqs, {pngMatch: 2}); out.unknownBatch = 'resolved'; } catch (e) { out.unknownBatch = e.constructor.name; }
  out.perRequest = kind(() => api.stitchPngBatchSync([{images: reqs[0].images, direction: 'vertical', opts: {pngMatch: 'window'}}]));
  out.setter = [kind(() => api.setPngMatch('lazy')), kind(() => api.setPngMatch(1)), kind(() => api.setPngMatch())];
  out.encode = kind(() => api.encodePng(reqs[1].images[0].data, reqs[1].images[0].width, reqs[1].images[0].height, {pngMatch: 4}));
  const r0 = reqs[0], m1 = reqs[1].images[0];
  put('plain', await api.stitchPng(r0.images, r0.direction, r0.opts));
  put('run', await api.stitchPng(r0.images, r0.direction, Object.assign({pngMatch: 'run'}, r0.opts)));
  put('window', await api.stitchPng(r0.images, r0.direction, Object.assign({pngMatch: 'window'}, r0.opts)));
  put('windowRgbAdaptive', await api.stitchPng(r0.images, r0.direction, Object.assign({pngMatch: 'window', pngColor: 'rgb', pngFilter: 'adaptive'}, r0.opts)));
  api.setPngColor('rgba'); api.setPngFilter('paeth');
  const batch = await api.stitchPngBatch(reqs, {pngLevel: 1, pngMatch: 'window'});
  batch.forEach((x, k) => put('batch' + k, x));
  api.stitchPngBatchSync(reqs, {pngMatch: 'run'}).forEach((x, k) => put('batchRun' + k, x));
  api.stitchPngBatchSync(reqs).forEach((x, k) => put('batchPlain' + k, x));
  put('encode', api.encodePng(m1.data, m1.width, m1.height, {pngMatch: 'window'}));
  put('encodeRun', api.encodePng(m1.data, m1.width, m1.height, {pngMatch: 'run'}));
  api.setPngMatch('window');
  put('sticky', await api.stitchPng(r0.images, r0.direction, r0.opts));
  api.setPngMatch('run');
  put('back', await api.stitchPng(r0.images, r0.direction, r0.opts));
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
"""


def test_node_stitch_png_batch_and_encode_with_window_matches(tmp_path):
    cases = K.by_name()
    groups = [[K.text_like(4900 + k, 60, 90) for k in range(3)], [KR.opaque(cases["match text over photo 720x12"])], [KR.opaque(cases["match text|noise 4200x3"])]]
    reqs, jreqs = [], []
    for r, datas in enumerate(groups):
        imgs = [{"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": True} for a in datas]
        opts = {"gap": 3, "mode": "max"} if r == 0 else {}
        reqs.append((imgs, "vertical", opts))
        jimgs = []
        for k, im in enumerate(imgs):
            f = tmp_path / ("r%d_%d.rgba" % (r, k))
            np.ascontiguousarray(im["data"]).tofile(f)
            jimgs.append({"width": im["width"], "height": im["height"], "file": str(f)})
        jreqs.append({"images": jimgs, "direction": "vertical", "opts": opts})
    script = tmp_path / "png_match.js"
    script.write_text(SCRIPT % json.dumps(os.path.join(U.ROOT, "node", "index.js")))
    jp = tmp_path / "reqs.json"
    jp.write_text(json.dumps(jreqs))
    run = subprocess.run([NODE, str(script), str(jp), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert json.loads(run.stdout.strip().splitlines()[-1]) == {"unknown": "TypeError", "unknownBatch": "TypeError", "perRequest": "TypeError",
                                                                "setter": ["TypeError"] * 3, "encode": "TypeError"}
    read = lambda tag: open(tmp_path / (tag + ".png"), "rb").read()
    canvases = [np.ascontiguousarray(c) for c in ist.stitch_batch(reqs)]
    assert canvases[1].shape == (12, 720, 4) and canvases[2].shape == (3, 4200, 4)        # whole rows per chunk | pieces of a row
    reps = [K.report("match node request %d" % k, c) for k, c in enumerate(canvases)]
    want = [M.file_bytes_window(c, 4, reps[k].stream) for k, c in enumerate(canvases)]
    assert all("form window" in K.regimes(r) for r in reps) and "run beside window" in K.regimes(reps[1])
    assert read("window") == want[0] and read("sticky") == want[0]
    assert read("window") == bytes(ist.stitch_png(*reqs[0][:2], dict(reqs[0][2], pngMatch="window"))["png"])      # the Python host's file
    assert read("windowRgbAdaptive") == M.file_bytes_window(canvases[0], 3, adaptive=True)
    assert read("run") == read("plain") == read("back") == R.file_bytes(canvases[0]) and len(want[0]) < len(read("plain"))
    for k in range(3):
        assert read("batch%d" % k) == want[k], k
        assert read("batchRun%d" % k) == read("batchPlain%d" % k) == R.file_bytes(canvases[k]), k
    assert read("batch1") == bytes(ist.stitch_png_batch(reqs, level=1, match="window")[1]["png"])
    assert read("encode") == want[1] and read("encodeRun") == R.file_bytes(canvases[1])
