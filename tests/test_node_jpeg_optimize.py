"""The Node host's JPEG export with optimize: true (encodeJpeg, stitchJpeg, stitchJpegBatch): every file equals the Python host's
for the same call - and so the numpy contract, which tests/test_gpu_jpeg_optimize.py holds the Python host to."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import util as U
from tests.test_gpu_jpeg_encode import photo, three_images

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_node_optimize_equals_the_python_host(tmp_path):
    import imagestitching_amd as ist
    a = photo(61, 45)
    imgs = three_images()
    np.ascontiguousarray(a).tofile(tmp_path / "a.rgba")
    for k, im in enumerate(imgs):
        np.ascontiguousarray(im).tofile(tmp_path / ("i%d.rgba" % k))
    sizes = [[im.shape[1], im.shape[0]] for im in imgs]
    script = tmp_path / "jpeg_optimize.js"
    script.write_text("""
const fs = require('fs'); const path = require('path');
const api = require(%s);
const dir = process.argv[2];
const sizes = %s;
const imgs = sizes.map((s, k) => ({width: s[0], height: s[1], opaque: true, data: fs.readFileSync(path.join(dir, 'i' + k + '.rgba'))}));
(async () => {
  const a = fs.readFileSync(path.join(dir, 'a.rgba'));
  fs.writeFileSync(path.join(dir, 'enc_opt.jpg'), api.encodeJpeg(a, 61, 45, {quality: 90, optimize: true}));
  fs.writeFileSync(path.join(dir, 'enc_opt444.jpg'), api.encodeJpeg(a, 61, 45, {quality: 50, subsampling: '444', optimize: true}));
  fs.writeFileSync(path.join(dir, 'enc_std.jpg'), api.encodeJpeg(a, 61, 45, {quality: 90, optimize: false}));
  const s = await api.stitchJpeg(imgs, 'vertical', {quality: 75, optimize: true});
  fs.writeFileSync(path.join(dir, 'stitch_opt.jpg'), s.jpeg);
  const reqs = [{images: imgs, direction: 'vertical', opts: {quality: 90, optimize: true}},
                {images: imgs.slice(0, 2), direction: 'horizontal', opts: {gap: 3, subsampling: '444'}},
                {images: imgs.slice(1), direction: 'horizontal', opts: {quality: 50, subsampling: '444', optimize: true}}];
  const b = await api.stitchJpegBatch(reqs);
  b.forEach((x, k) => fs.writeFileSync(path.join(dir, 'batch' + k + '.jpg'), x.jpeg));
  console.log(JSON.stringify([s.width, s.height]));
})().catch((e) => { console.error(e); process.exit(1); });
""" % (json.dumps(os.path.join(U.ROOT, "node", "index.js")), json.dumps(sizes)))
    r = subprocess.run([NODE, str(script), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    read = lambda name: (tmp_path / name).read_bytes()
    assert read("enc_opt.jpg") == ist.encode_jpeg(a, 90, "420", optimize=True)
    assert read("enc_opt444.jpg") == ist.encode_jpeg(a, 50, "444", optimize=True)
    assert read("enc_std.jpg") == ist.encode_jpeg(a, 90, "420") != read("enc_opt.jpg")
    want = ist.stitch_jpeg(imgs, "vertical", {"quality": 75, "optimize": True})
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [want["width"], want["height"]]
    assert read("stitch_opt.jpg") == want["jpeg"] != ist.stitch_jpeg(imgs, "vertical", {"quality": 75})["jpeg"]
    reqs = [(imgs, "vertical", {"quality": 90, "optimize": True}), (imgs[:2], "horizontal", {"gap": 3, "subsampling": "444"}),
            (imgs[1:], "horizontal", {"quality": 50, "subsampling": "444", "optimize": True})]
    for k, w in enumerate(ist.stitch_jpeg_batch(reqs)):
        assert read("batch%d.jpg" % k) == w["jpeg"], k
