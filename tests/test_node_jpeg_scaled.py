"""Reduced-size JPEG decode through the Node host (node/index.js decodeBitmaps(files, {scale}), decodeScaleFit) on the GPU: the
downloads equal the Python host's for the same files and scales, the descs keep the natural size beside the stored one, the held
memory is the scaled bitmaps', and a bad scale rejects with the library's message before anything is decoded."""
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from tests import jpeg_writer as JW
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
(async () => {
  const base = api.debugBitmapBytes();
  const bms = await api.decodeBitmaps(job.paths, { scale: job.scales });
  out.held = api.debugBitmapBytes() - base;
  out.desc = bms.map((b) => [b.width, b.height, b.bmpWidth, b.bmpHeight]);
  bms.forEach((b, k) => fs.writeFileSync(job.out + '.' + k + '.rgba', b.download()));
  const one = await api.decodeBitmaps(job.paths, { scale: 4 });
  out.oneScale = one.map((b) => [b.bmpWidth, b.bmpHeight]);
  const plain = await api.decodeBitmaps(job.paths), ones = await api.decodeBitmaps(job.paths, { scale: 1 });
  out.plainSame = plain.every((b, k) => b.download().equals(ones[k].download()) && b.bmpWidth === b.width);
  out.bad = await api.decodeBitmaps(job.paths, { scale: job.scales.map((d, k) => (k === 1 ? 3 : d)) }).then(() => 'resolved', (e) => String(e.message));
  out.badType = await api.decodeBitmaps(job.paths, { scale: [1, 2] }).then(() => 'resolved', (e) => e.constructor.name);
  out.fit = [api.decodeScaleFit(4032, 3024, 100, 100), api.decodeScaleFit(4032, 3024, 1080, 100), api.decodeScaleFit(9, 9, 6, 5)];
  out.fitBad = (() => { try { api.decodeScaleFit(0, 1, 1, 1); return 'no error'; } catch (e) { return e.code; } })();
  [...bms, ...one, ...plain, ...ones].forEach((b) => b.release());
  out.after = api.debugBitmapBytes() - base;
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""


def test_node_scaled_bitmaps_equal_the_python_hosts(tmp_path):
    big = JW.large_cases()
    png = io.BytesIO()
    Image.fromarray(U.rand_image(5, 30, 50, opaque=False)).save(png, "PNG")
    files = [big[0]["data"], big[2]["data"], png.getvalue(), big[3]["data"], JW.size_cases("422")[140]["data"]]
    scales = [2, 4, 8, 8, 1]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d" % k)))
        open(paths[-1], "wb").write(f)
    job = {"paths": paths, "scales": scales, "out": str(tmp_path / "r")}
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, "-e", JS, os.path.join(ROOT, "node", "index.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    want = ist.decode_bitmaps(files, scale=scales)
    held = 0
    for k, (b, d) in enumerate(zip(want, out["desc"])):
        rows, cols, _ = b.shape
        assert d == [b.width, b.height, cols, rows], k
        px = np.fromfile(str(tmp_path / ("r.%d.rgba" % k)), np.uint8).reshape(rows, cols, 4)
        assert np.array_equal(px, b.download()), k
        held += (4 * cols * rows + 256 + 255) & ~255
        b.close()
    assert out["held"] == held and out["after"] == 0
    infos = [ist.image_info(f) for f in files]
    assert out["oneScale"] == [list(ist.scaled_size(w, h, 4)) if k != 2 else [w, h] for k, (w, h, _) in enumerate(infos)]      # (the PNG stays 1 / 1)
    assert out["plainSame"]
    assert "image 1" in out["bad"] and "3" in out["bad"], out["bad"]
    assert out["badType"] == "TypeError"
    assert out["fit"] == [8, 2, 1] and out["fitBad"] == "-1"      # (the addon's error code is a string)
