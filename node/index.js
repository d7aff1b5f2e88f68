'use strict';
/**
 * Node host of the MI355X strip stitcher: the reference's stitch surface as one function.
 *
 * Reference: Page.onStitch (miniprogram-stitch/miniprogram/pages/index/index.js:1186-1633) reads
 * this.data.{images, direction, gap, verticalStitchMode, horizontalStitchMode}.  Here:
 *
 *   stitch(images, direction, opts?) -> Promise<{width, height, data: Buffer, plan}>
 *   stitchBatch([{images, direction, opts?}, ...]) -> Promise<({width, height, data, plan} | null)[]>   (one GPU, many stitches)
 *   stitchJpeg(images | Bitmap[], direction, opts + {quality, subsampling, optimize}) -> Promise<{width, height, jpeg, plan}>   (baseline JFIF)
 *   encodeJpeg(data, width, height, {quality, subsampling, optimize}) -> Buffer
 *   stitchPngBatch([{images, direction, opts?}, ...]) -> Promise<({width, height, png, plan} | null)[]>   (one GPU, many PNG files)
 *   stitchJpegBatch([{images, direction, opts?}, ...]) -> Promise<({width, height, jpeg, plan} | null)[]>  (one GPU, many JPEG files)
 *   joinJpegCheck(files, direction) -> {ok, reason, image, width, height, subsampling},  joinJpeg(files, direction, {optimize}) -> Promise<Buffer>   (lossless: compatible JPEG files joined in the coefficient domain)
 *   decodeBitmaps(files, {scale?, colorProfile?}) -> Promise<Bitmap[]>,  imageColor(file) -> 'none' | 'identity' | 'convert' | 'unsupported',  decodeScaleFit(w, h, minW, minH) -> 1 | 2 | 4 | 8,  uploadBitmap(image) -> Bitmap   (images kept in GPU memory: stitch, stitchSync,
 *       stitchPng and plan take Bitmap[] in place of images, and a restitch decodes and uploads nothing)
 *   stitchPng / stitchFiles with opts.preview = {width, height} also resolve preview: {width, height, data}: the canvas shrunk to fit
 *       that box (the redraw into the preview node, index.js:1597-1603), reduced in GPU memory beside the export;
 *       Bitmap.preview(width, height) is the same of a resident bitmap
 *   thumbnails(bitmaps, {width, height, mode, orient}) resolves [{width, height, data}]: the grid of chosen images, every bitmap cropped
 *       ('fill') or fitted ('fit') to the cell, turned by its EXIF orientation and shrunk, in one launch pair and one copy down
 *
 * images[i] = {width, height, data: Uint8Array (RGBA8, straight alpha, row-major), orientation?: 1..8, fileSize?, opaque?}
 * direction = 'vertical' | 'horizontal'                         (data.direction, index.js:16)
 * opts      = {mode: 'min'|'max'|'original' (default 'min', index.js:19-20), gap: 0..20 (default 0, index.js:17),
 *              filter: 'bilinear'|'nearest' (imageSmoothingEnabled, index.js:1416) | 'area' | 'cubic' (opt-in quality filters), platform: 'ios'|'android'|'devtools'
 *              (reproduces the phone caps, index.js:1323-1336; default: caps lifted, superSample 1),
 *              maxSide, maxPixels (deviceMaxCanvasSize/Pixels), superSample (MAX_SUPER_SAMPLE, index.js:1363),
 *              onProgress: (percent) => void  (the stitchProgress checkpoints of index.js:1193-1611),
 *              edgeAA: anti-alias fractional rectangle edges by area coverage (default: true when `platform` is given - a
 *              reference plan has fractional edges as a rule - false otherwise: pixel-centre rule),
 *              devices: number[] - shard the stitch over these GPUs from this one process (devices[0] = root; parts render
 *              on their GPUs, one grouped RCCL send/recv batch over xGMI gathers the bands into the root's canvas),
 *              split: 'image' (image i -> devices[i mod n], the BASELINE layout) | 'band' (equal output rows per GPU, cut draw by draw)
 *                     | 'rows' (GPU s owns a band of canvas rows across ALL draws: full-width bands for horizontal strips too,
 *                     index.js:1540-1553) | 'auto' (default: 'image' when its parts are full-width, else 'rows'),
 *              preview: {width, height} - stitchPng / stitchFiles only: the box the result's preview is fitted into}
 * Errors reject with Error('拼图失败：' + reason) like the reference's catch (index.js:1618-1624); err.code is the
 * C-ABI code.  No pixel arithmetic happens in JavaScript; there is no CPU fallback.
 */
const path = require('path');
const native = require(path.join(__dirname, 'imagestitch.node'));

const DIRECTION = { vertical: 0, horizontal: 1 };
const MODE = { min: 0, max: 1, original: 2 };
const FILTER = { nearest: 0, bilinear: 1, area: 2, cubic: 3 };
const PLATFORM = { other: 0, devtools: 0, windows: 0, mac: 0, ios: 1, android: 2 };
const KNOWN = ['mode', 'gap', 'filter', 'platform', 'maxSide', 'maxPixels', 'superSample', 'onProgress', 'edgeAA', 'pngLevel', 'pngColor', 'pngFilter', 'pngMatch', 'devices', 'split', 'preview', 'overlap', 'colorProfile'];
const SPLIT = { image: 0, band: 1, rows: 2, auto: 3 };
const FILTER_EDGE_AA = 0x100;    // IST_FILTER_EDGE_AA: anti-alias fractional rectangle edges by area coverage

function limitsOf(opts) {
  const o = opts || {};
  const lim = {};
  if (o.platform !== undefined && o.platform !== null) {
    if (!(o.platform in PLATFORM)) throw new TypeError('unknown platform ' + o.platform);
    lim.platform = PLATFORM[o.platform];
  }
  if (typeof o.maxSide === 'number') lim.maxSide = o.maxSide;
  if (typeof o.maxPixels === 'number') lim.maxPixels = o.maxPixels;
  if (typeof o.superSample === 'number') lim.superSample = o.superSample;
  return Object.keys(lim).length ? lim : null;
}

// Coverage rule for fractional rectangle edges.  Unset: ON whenever a reference platform's plan is requested (the
// reference's default plans scale the canvas by superSample 2.2 / 2.6 for fewer than 7 images, index.js:1363,1426-1428, and
// keep an unrounded cursor when gap > 0 and scaleDown < 1, :1432, so fractional edges are normal there and a Canvas raster
// anti-aliases them); OFF for the lifted MI355X default (every output pixel owned by exactly one image).
function edgeAA(o) { return (o.edgeAA === undefined || o.edgeAA === null) ? (o.platform !== undefined && o.platform !== null) : !!o.edgeAA; }

const OVERLAP_NEEDS = 'option overlap applies to stitch / stitchSync / stitchPng / stitchJpeg of a vertical strip of Bitmaps (uploadBitmap / decodeBitmaps): the overlaps are searched where the pixels are resident';
// opts.colorProfile / decodeBitmaps' colorProfile: 'ignore' = the pixels as decoded (default), 'srgb' = a file tagged with a matrix/TRC
// ICC profile (Display P3, Adobe RGB) is converted to sRGB on the GPU behind its decode (include/imagestitch.h "colour profiles").
// The value travels with its native call; an unknown one is a TypeError before any native call.
const COLOR_PROFILE = { ignore: 0, srgb: 1 };      // IST_COLOR_PROFILE_IGNORE / IST_COLOR_PROFILE_SRGB
const COLOR_KIND = ['none', 'identity', 'convert', 'unsupported'];      // IST_COLOR_*
const COLOR_NEEDS = 'option colorProfile applies to stitchFiles and decodeBitmaps: a profile comes with a file, raw pixels carry none';
function colorProfileOf(opts) {
  if (!opts || opts.colorProfile === undefined || opts.colorProfile === null) return COLOR_PROFILE.ignore;
  if (typeof opts.colorProfile !== 'string' || !Object.prototype.hasOwnProperty.call(COLOR_PROFILE, opts.colorProfile)) throw new TypeError("colorProfile must be 'ignore' or 'srgb'");
  return COLOR_PROFILE[opts.colorProfile];
}
function args(images, direction, opts, files) {
  const o = opts || {};
  for (const k of Object.keys(o)) if (!KNOWN.includes(k)) throw new TypeError('unknown stitch option ' + k);
  if (!files && o.colorProfile !== undefined && o.colorProfile !== null) throw new TypeError(COLOR_NEEDS);
  if (o.overlap !== undefined && o.overlap !== null) throw new TypeError(OVERLAP_NEEDS);      // (withOverlap takes the option out where it applies)
  if (!(direction in DIRECTION)) throw new TypeError("direction must be 'vertical' or 'horizontal'");
  const mode = o.mode || 'min';                      // `|| 'min'` (index.js:1257)
  if (!(mode in MODE)) throw new TypeError('unknown mode ' + mode);
  const filter = o.filter || 'bilinear';
  if (!(filter in FILTER)) throw new TypeError('unknown filter ' + filter);
  return [images || [], DIRECTION[direction], MODE[mode], Number(o.gap) || 0, limitsOf(o), FILTER[filter] | (edgeAA(o) ? FILTER_EDGE_AA : 0)];
}

// The reference reports progress through setData({stitchProgress}): 1 at the start (index.js:1193), 25 when every image
// is prepared (:1247-1248), 30 after planning (:1358), 30 + 60*(i+1)/n (capped at 90) per drawn image (:1556-1557), 96
// after the export (:1581), 100 at the end (:1611).  Here the draw loop is ONE launch, so the per-image steps collapse
// into 90; opts.onProgress(percent) receives the same checkpoints.
function withProgress(opts, run) {
  const cb = opts && typeof opts.onProgress === 'function' ? opts.onProgress : null;
  if (!cb) return run();
  cb(1); cb(25); cb(30);
  return run().then((r) => { cb(90); cb(96); cb(100); return r; }, (e) => { cb(0); throw e; });       // failure resets to 0 (:1622)
}

// opts.devices -> the (devices, split) arguments that follow asPng in the native call ([] without a device group)
function groupArgs(opts) {
  const o = opts || {};
  if (o.devices === undefined || o.devices === null) return [];
  if (!Array.isArray(o.devices) || !o.devices.length || !o.devices.every((d) => Number.isInteger(d) && d >= 0)) throw new TypeError('devices must be a non-empty array of GPU indices');
  const split = o.split || 'auto';
  if (!(split in SPLIT)) throw new TypeError('unknown split ' + split);
  return [o.devices, SPLIT[split]];
}
// opts.preview -> the trailing (previewWidth, previewHeight) arguments of a native PNG call ([] without one)
function previewArgs(opts) {
  const p = opts ? opts.preview : undefined;
  if (p === undefined || p === null) return [];
  if (opts.devices !== undefined && opts.devices !== null) throw new TypeError('preview does not apply with devices: previews run on one GPU');
  if (typeof p !== 'object' || typeof p.width !== 'number' || typeof p.height !== 'number') throw new TypeError('preview must be {width, height}');
  return [p.width, p.height];
}
// the calls that hand the pixels to the caller, or run a batch, keep no canvas behind an export to preview
function noPreview(opts, who) {
  if (opts && opts.preview !== undefined && opts.preview !== null) throw new TypeError(who + ': option preview does not apply (the caller gets the pixels; use stitchPng / stitchFiles)');
}
// ---- resident bitmaps ----------------------------------------------------------------------------------------------------------
const MADE_HERE = Symbol('Bitmap');
/** One decoded RGBA8 image kept in GPU memory by the library (the page's bitmap cache, index.js:534-627): made by decodeBitmaps /
 *  uploadBitmap, stitched again and again by stitch / stitchSync / stitchPng with nothing decoded or uploaded.  width, height,
 *  orientation, opaque and fileSize are what the planner reads.  release() drops it (again: nothing); using it afterwards throws.
 *  A Bitmap that is collected unreleased is released then; a stitch in flight holds the bitmap until it settles. */
class Bitmap {
  constructor(token, handle) {
    if (token !== MADE_HERE) throw new TypeError('Bitmaps are made by decodeBitmaps / uploadBitmap');
    const d = native.bitmapDesc(handle);
    const ro = (value) => ({ value, enumerable: true });
    Object.defineProperties(this, {
      handle: { value: handle },
      width: ro(d.width), height: ro(d.height), orientation: ro(d.orientation), opaque: ro(d.opaque), fileSize: ro(d.fileSize),
      bmpWidth: ro(d.bmpWidth), bmpHeight: ro(d.bmpHeight),
    });
  }
  /** the pixels as they are stored (bmpWidth x bmpHeight, RGBA8, dense rows) */
  download() { return native.bitmapDownload(this.handle); }
  /** the stored pixels shrunk to fit a width x height box (index.js:1600-1602; EXIF orientation is not applied, as in download()):
   *  {width, height, data}, reduced in GPU memory - a thumbnail without the download */
  preview(width, height) { return native.bitmapPreview(this.handle, width, height); }
  /** rows [y0, y0 + n) of the stored pixels as a Bitmap of their own: a view that shares this bitmap's memory and keeps it alive,
   *  copies nothing, and goes wherever a Bitmap goes.  Refused (err.code '-7') for EXIF orientation > 1 and reduced-scale decodes. */
  rows(y0, n) { return new Bitmap(MADE_HERE, native.bitmapRows(this.handle, y0, n)); }
  release() { native.bitmapRelease(this.handle); }
}
// a request made of Bitmaps -> their native handles (null entries stay null: the library rejects them as a missing image); null for a
// request of host images.  A request is one or the other.
function bitmapHandles(images, opts) {
  if (!Array.isArray(images) || !images.some((x) => x instanceof Bitmap)) return null;
  if (!images.every((x) => x === null || x === undefined || x instanceof Bitmap)) throw new TypeError('a request is either all Bitmaps or all host images, not a mix');
  if (opts && opts.devices !== undefined && opts.devices !== null) throw new TypeError('devices does not apply to Bitmaps: a bitmap lives on one GPU');
  return images.map((x) => (x ? x.handle : null));
}
/** Image files (Buffers, or paths read here as stitchFiles reads them) -> Bitmaps, decoded straight into GPU memory by the decoder
 *  of stitchFiles; each one's width / height / orientation / opaque / fileSize is what stitchFiles plans with.  All or nothing: a
 *  file that does not decode rejects with '图片k解码异常: ...' and no bitmap is kept.
 *  opts.scale: 1, 2, 4 or 8, one for all files or one per file - a JPEG is decoded at 1 / scale of its size (libjpeg-turbo's
 *  decode-to-scale, byte for byte) and kept at that size: width / height stay the natural size, bmpWidth / bmpHeight are the stored
 *  one, and stitch, previews and thumbnails take the bitmap as it is.  Other file types decode at 1 / 1.
 *  opts.colorProfile: 'ignore' (default) or 'srgb' - a file tagged with an ICC profile the colour contract takes lands converted to sRGB;
 *  untagged, sRGB-tagged and unsupported files stay as decoded (imageColor says which a file is). */
async function decodeBitmaps(files, opts) {
  if (!Array.isArray(files)) throw new TypeError('decodeBitmaps(files: (Uint8Array | string)[], {scale?, colorProfile?})');
  const profile = colorProfileOf(opts);
  const scale = opts === undefined || opts === null ? undefined : opts.scale;
  let scales;
  if (scale !== undefined && scale !== null) {
    scales = Array.isArray(scale) ? scale : files.map(() => scale);
    if (scales.length !== files.length || !scales.every((d) => typeof d === 'number')) throw new TypeError('decodeBitmaps: scale must be a number or one number per file');
  }
  const fs = require('fs');
  const bufs = files.map((f) => (typeof f === 'string' ? fs.readFileSync(f) : f));
  if (!bufs.length) return [];
  const handles = await native.decodeBitmaps(bufs, scales, profile);
  return handles.map((h) => new Bitmap(MADE_HERE, h));
}
// the IST_JOIN_* reason codes of joinJpegCheck, by value
const JOIN_REASON = ['ok', 'not_jpeg', 'layout', 'mixed', 'tables', 'size', 'align', 'orient', 'limit', 'range'];
function joinArgs(files, direction, usage) {
  if (!Array.isArray(files) || !files.length) throw new TypeError(usage);
  if (!(direction in DIRECTION)) throw new TypeError("direction must be 'vertical' or 'horizontal'");
  const fs = require('fs');
  return [files.map((f) => (typeof f === 'string' ? fs.readFileSync(f) : f)), DIRECTION[direction]];
}
/** Can these JPEG files (Buffers, or paths read here) be joined losslessly?  Headers only, pure CPU.  Returns {ok, reason, image,
 *  width, height, subsampling}: reason 'ok' or the first refusal ('not_jpeg', 'layout', 'mixed', 'tables', 'size', 'align', 'orient',
 *  'limit'), image the first image it applies to (-1: none), width / height the joined file's size when ok (else 0), subsampling
 *  '444' / '420' of image 0 once known (else null). */
function joinJpegCheck(files, direction) {
  const [bufs, dir] = joinArgs(files, direction, "joinJpegCheck(files: (Uint8Array | string)[], direction)");
  const r = native.joinJpegCheck(bufs, dir);
  return { ok: r.ok, reason: JOIN_REASON[r.reason], image: r.image, width: r.width, height: r.height, subsampling: r.subsampling === 0 ? '444' : r.subsampling === 1 ? '420' : null };
}
/** JPEG files -> ONE JPEG file (a Buffer) that carries exactly the sources' quantised coefficients and quantisation tables: what
 *  jpegtran does for one file, done for a strip, on the GPU.  No pixel is made, nothing is lost, no quality is chosen.  The sources
 *  share a width (vertical) or height (horizontal), a sampling layout (4:4:4 / 4:2:0) and their quantisation tables (joinJpegCheck
 *  says whether a set qualifies).  opts.optimize (a boolean, default false): the file's own Huffman tables.  An ineligible set
 *  rejects with the library's Error (IST_E_UNSUPPORTED, the message names the image and the reason); nothing falls back to pixels. */
function joinJpeg(files, direction, opts) {
  let a, optimize;
  try {
    a = joinArgs(files, direction, "joinJpeg(files: (Uint8Array | string)[], direction, {optimize?})");
    optimize = (opts && opts.optimize !== undefined && opts.optimize !== null) ? opts.optimize : false;
    if (typeof optimize !== 'boolean') throw new TypeError('optimize must be a boolean');
  } catch (e) { return Promise.reject(e); }
  return native.joinJpeg(a[0], a[1], optimize ? 0x100 : 0);
}
/** The colour kind of an image file: 'none' (untagged), 'identity' (tagged sRGB), 'convert' (what colorProfile 'srgb' converts) or
 *  'unsupported' (a profile the contract does not take: LUT-only, GRAY, CMYK, damaged).  Pure CPU. */
function imageColor(file) { return COLOR_KIND[native.imageColor(typeof file === 'string' ? require('fs').readFileSync(file) : file)]; }
/** The largest scale in {1, 2, 4, 8} at which a width x height file still decodes to at least minWidth x minHeight pixels (1 if none
 *  does): what to pass as decodeBitmaps' scale for a file that is only ever shown that small.  Pure CPU. */
function decodeScaleFit(width, height, minWidth, minHeight) { return native.decodeScaleFit(width, height, minWidth, minHeight); }
/** One host image ({width, height, data, orientation?, fileSize?, opaque?}, as stitch takes it) -> a Bitmap with that desc. */
function uploadBitmap(image) { return new Bitmap(MADE_HERE, native.uploadBitmap([image])); }
/** The grid of chosen images (index.wxml:4-22): every Bitmap as a thumbnail for a width x height cell, all of them cropped or fitted,
 *  turned and shrunk in GPU memory by one launch pair and brought down in one copy.  mode 'fill' (default) crops to the cell's aspect
 *  ratio (aspectFill), 'fit' fits the whole image into the cell (aspectFit, index.wxml:202); orient: false shows the stored pixels as
 *  Bitmap.preview does.  Resolves [{width, height, data}] (RGBA8, straight alpha, dense rows), in the order given. */
function thumbnails(bitmaps, cell) {
  const c = cell || {};
  if (!Array.isArray(bitmaps) || !bitmaps.every((x) => x === null || x === undefined || x instanceof Bitmap)) return Promise.reject(new TypeError('thumbnails(bitmaps: Bitmap[], {width, height, mode?, orient?})'));
  if (typeof c.width !== 'number' || typeof c.height !== 'number') return Promise.reject(new TypeError('thumbnails: the cell must be {width, height}'));
  const mode = c.mode === undefined ? 'fill' : c.mode;
  if (mode !== 'fill' && mode !== 'fit') return Promise.reject(new TypeError("thumbnails: mode must be 'fill' or 'fit'"));
  if (!bitmaps.length) return Promise.resolve([]);
  try { return native.thumbnails(bitmaps.map((x) => (x ? x.handle : null)), c.width, c.height, mode === 'fit' ? 1 : 0, c.orient !== false); } catch (e) { return Promise.reject(e); }      // (a released Bitmap throws on this thread)
}
// {tolerance, minRows, minInformative} of an overlap search (the contract's defaults, include/imagestitch.h), checked
function overlapArgs(o) {
  const v = Object.assign({ tolerance: 8, minRows: 16, minInformative: 8 }, o || {});
  for (const k of Object.keys(v)) if (!['tolerance', 'minRows', 'minInformative'].includes(k)) throw new TypeError('unknown overlap option ' + k);
  for (const k of Object.keys(v)) if (!Number.isInteger(v[k]) || v[k] < 0) throw new RangeError(k + ' must be a non-negative integer');
  return [v.tolerance, v.minRows, v.minInformative];
}
function overlapHandles(bitmaps) {
  if (!Array.isArray(bitmaps) || !bitmaps.every((x) => x instanceof Bitmap)) throw new TypeError('findOverlaps(bitmaps: Bitmap[], {tolerance?, minRows?, minInformative?}): ' + OVERLAP_NEEDS);
  return bitmaps.map((x) => x.handle);
}
/** Per neighbouring pair of a vertical strip of Bitmaps (scrolled screenshots, top to bottom): {header, footer, overlap, cost} - the
 *  rows of a bar both shots repeat at the top and at the bottom, the rows of the upper shot's body the lower one shows again, and
 *  the summed row difference there.  Found on the GPU from the resident pixels (three launches); the rule and its limits are in
 *  include/imagestitch.h.  The defaults are the contract's, not measured optima: tolerance 8 is two 8-bit levels per pixel. */
function findOverlaps(bitmaps, opts) {
  try { return native.findOverlaps(overlapHandles(bitmaps), ...overlapArgs(opts)); } catch (e) { return Promise.reject(e); }
}
function findOverlapsSync(bitmaps, opts) { return native.findOverlapsSync(overlapHandles(bitmaps), ...overlapArgs(opts)); }
/** The crop rule (pure CPU): [[top, bot]] per image - image i keeps rows [top, bot) - for findOverlaps' records and the heights. */
function overlapRows(pairs, heights) { return native.overlapRows(pairs, heights); }
// opts.overlap ('auto' or {tolerance, minRows, minInformative}) around one stitch call: the overlaps are found, the call runs on row
// views of the bitmaps with the option taken out, the views are released, and the result carries the records as `overlaps`
function overlapOf(images, direction, opts) {
  const v = opts ? opts.overlap : undefined;
  if (v === undefined || v === null) return null;
  if (v !== 'auto' && (typeof v !== 'object' || Array.isArray(v))) throw new TypeError("overlap must be 'auto' or {tolerance, minRows, minInformative}");
  const o = overlapArgs(v === 'auto' ? null : v);
  if (direction !== 'vertical' || !Array.isArray(images) || !images.length || !images.every((x) => x instanceof Bitmap) || (opts.devices !== undefined && opts.devices !== null)) throw new TypeError(OVERLAP_NEEDS);
  const rest = Object.assign({}, opts);
  delete rest.overlap;
  return { o, rest };
}
function cropViews(images, records) {
  const rows = native.overlapRows(records, images.map((b) => b.bmpHeight));
  const views = [];
  try { images.forEach((b, i) => views.push(b.rows(rows[i][0], rows[i][1] - rows[i][0]))); } catch (e) { views.forEach((x) => x.release()); throw e; }
  return views;
}
function withOverlap(fn) {
  return (images, direction, opts) => {
    let w;
    try { w = overlapOf(images, direction, opts); } catch (e) { return Promise.reject(e); }
    if (!w) return fn(images, direction, opts);
    const found = images.length > 1 ? native.findOverlaps(images.map((x) => x.handle), ...w.o) : Promise.resolve([]);
    return found.then((records) => {
      const views = cropViews(images, records);
      const done = () => views.forEach((x) => x.release());
      return fn(views, direction, w.rest).then((r) => { done(); if (r) r.overlaps = records; return r; }, (e) => { done(); throw e; });
    });
  };
}
function withOverlapSync(fn) {
  return (images, direction, opts) => {
    const w = overlapOf(images, direction, opts);
    if (!w) return fn(images, direction, opts);
    const records = images.length > 1 ? native.findOverlapsSync(images.map((x) => x.handle), ...w.o) : [];
    const views = cropViews(images, records);
    try { const r = fn(views, direction, w.rest); if (r) r.overlaps = records; return r; } finally { views.forEach((x) => x.release()); }
  };
}
/** device bytes held by the live bitmaps of this process */
function debugBitmapBytes() { return native.debugBitmapBytes(); }

// One stitch through the native call of its sources: the handles h of a Bitmap request, or (h null) the host images of a = args().
// asPng is the native argument of that name (false, true, or the JPEG export's {quality, subsampling}), rest what follows it for host
// images, pv = previewArgs(opts); before (pngForm) runs inside the progress, ahead of the call.
function runStitch(opts, h, a, asPng, rest, pv, before) {
  const run = () => { if (before) before(); return h ? native.stitchBitmaps(h, a[1], a[2], a[3], a[4], a[5], asPng, ...pv) : native.stitch(...a, asPng, ...rest, ...pv); };
  if (!h) return withProgress(opts, run);
  // (the native call retains every bitmap before it returns: a release() from here on does not free one under the stitch)
  try { return withProgress(opts, run); } catch (e) { return Promise.reject(e); }      // (a released Bitmap throws on this thread)
}
function stitch(images, direction, opts) {
  let a, h, g;
  try { noPreview(opts, 'stitch'); h = bitmapHandles(images, opts); a = args(images, direction, opts); g = h ? [] : groupArgs(opts); } catch (e) { return Promise.reject(e); }
  if (!a[0].length) return Promise.resolve(null);      // `if (!originalImages.length) return;` (index.js:1189): no progress, no error
  return runStitch(opts, h, a, false, g, []);
}
function stitchSync(images, direction, opts) {
  noPreview(opts, 'stitchSync');
  const h = bitmapHandles(images, opts);
  const a = args(images, direction, opts), g = h ? [] : groupArgs(opts);
  if (!a[0].length) return null;
  return h ? native.stitchBitmapsSync(h, a[1], a[2], a[3], a[4], a[5], false) : native.stitchSync(...a, false, ...g);
}
// A batch runs on one GPU and returns pixels: the device-group and PNG options do not apply to its requests.
const BATCH_REFUSED = ['devices', 'split', 'pngLevel', 'pngColor', 'pngFilter', 'pngMatch', 'preview', 'overlap'];
// the native arguments of request k of a batch, opts given apart (the JPEG batch takes its own two out first)
function batchRequest(r, k, o) {
  for (const key of BATCH_REFUSED) if (key in o) throw new TypeError('request ' + k + ': option ' + key + ' does not apply to a batch');
  if (Array.isArray(r.images) && r.images.some((x) => x instanceof Bitmap)) throw new TypeError('request ' + k + ': Bitmaps do not apply to a batch');
  return args(r.images, r.direction, o);
}
// the requests of a batch, each turned into its native arguments by one(r, k)
function eachRequest(requests, one) {
  if (!Array.isArray(requests)) throw new TypeError('requests must be an array of {images, direction, opts?}');
  return requests.map((r, k) => {
    if (!r || typeof r !== 'object') throw new TypeError('request ' + k + ' must be {images, direction, opts?}');
    return one(r, k);
  });
}
function batchArgs(requests) { return eachRequest(requests, (r, k) => batchRequest(r, k, r.opts || {})); }
/** Many independent stitches in one call (one GPU): resolves an array with one {width, height, data, plan} per request
 *  - the same bytes stitchSync returns for it - and null for a request without images.  Each request is one onStitch
 *  (index.js:1186-1633); their canvases are rendered by one kernel launch per kernel form. */
function stitchBatch(requests) {
  let a;
  try { a = batchArgs(requests); } catch (e) { return Promise.reject(e); }
  if (!a.length) return Promise.resolve([]);
  return native.stitchBatch(a);
}
function stitchBatchSync(requests) { const a = batchArgs(requests); return a.length ? native.stitchBatchSync(a) : []; }
/** stitchBatch with the reference's export: resolves one {width, height, png: Buffer, plan} per request - the PNG stitchPng gives
 *  for it, in the form setPngLevel / setPngColor / setPngFilter / setPngMatch chose or opts = {pngLevel, pngColor, pngFilter, pngMatch}
 *  chooses for the whole batch (a per-request pngLevel, pngColor, pngFilter or pngMatch is refused) - and null for a request without images. The canvases never leave the GPU; one compression
 *  launch encodes every file of a sub-batch. */
function stitchPngBatch(requests, opts) {
  let a;
  try { a = batchArgs(requests); pngColorOf(opts); pngFilterOf(opts); pngMatchOf(opts); } catch (e) { return Promise.reject(e); }
  if (!a.length) return Promise.resolve([]);
  try { pngForm(opts); } catch (e) { return Promise.reject(e); }
  return native.stitchPngBatch(a);
}
function stitchPngBatchSync(requests, opts) { const a = batchArgs(requests); pngColorOf(opts); pngFilterOf(opts); pngMatchOf(opts); if (!a.length) return []; pngForm(opts); return native.stitchPngBatchSync(a); }
/** stitch + the reference's export step: resolves {width, height, png: Buffer (a lossless PNG file), plan}. The canvas
 *  never leaves the GPU; only the PNG bytes cross PCIe (utils/canvas.js:205-242, index.js:1577-1579). */
function stitchPng(images, direction, opts) {
  let a, h, pv;
  try { h = bitmapHandles(images, opts); a = args(images, direction, opts); pv = previewArgs(opts); pngColorOf(opts); pngFilterOf(opts); pngMatchOf(opts); } catch (e) { return Promise.reject(e); }
  if (!a[0].length) return Promise.resolve(null);
  return runStitch(opts, h, a, true, pv.length ? [null, 0] : [], pv, () => pngForm(opts));      // (no devices, split 0 ahead of the preview box)
}
// requests[k] of stitchJpegBatch -> [...what a batch request is, quality, subsampling]; every error names its request
function jpegBatchArgs(requests) {
  return eachRequest(requests, (r, k) => {
    const o = Object.assign({}, r.opts || {});
    try {
      const j = jpegArgs(o); delete o.quality; delete o.subsampling; delete o.optimize;
      return batchRequest(r, k, o).concat([j.quality, j.subsampling]);
    } catch (e) {
      if (!e.message.startsWith('request ' + k)) e.message = 'request ' + k + ': ' + e.message;
      throw e;
    }
  });
}
/** stitchPngBatch with the JPEG export: resolves one {width, height, jpeg: Buffer, plan} per request - the file stitchJpeg gives for
 *  it - and null for a request without images. Each request's opts may carry quality (1..100, default 90) and subsampling ('420'
 *  default, '444'). One transform, one entropy and one gather launch encode every file of a sub-batch. */
function stitchJpegBatch(requests) {
  let a;
  try { a = jpegBatchArgs(requests); } catch (e) { return Promise.reject(e); }
  if (!a.length) return Promise.resolve([]);
  return native.stitchJpegBatch(a);
}
function stitchJpegBatchSync(requests) { const a = jpegBatchArgs(requests); return a.length ? native.stitchJpegBatchSync(a) : []; }
const SUBSAMPLING = { 444: 0, 420: 1 };          // IST_JPEG_444 / IST_JPEG_420
// {quality, subsampling} of a JPEG export, checked: an integer quality 1..100 (default 90), subsampling '420' (default) or '444',
// optimize a boolean (default false: the file's own Huffman tables, IST_JPEG_OPTIMIZE = 0x100 OR-ed into the subsampling)
function jpegArgs(o) {
  const quality = (o && o.quality !== undefined && o.quality !== null) ? o.quality : 90;
  const ss = String((o && o.subsampling !== undefined && o.subsampling !== null) ? o.subsampling : '420');
  if (!Number.isInteger(quality) || quality < 1 || quality > 100) throw new RangeError('quality must be an integer 1..100');
  if (!(ss in SUBSAMPLING)) throw new TypeError("subsampling must be '420' or '444'");
  const optimize = (o && o.optimize !== undefined && o.optimize !== null) ? o.optimize : false;
  if (typeof optimize !== 'boolean') throw new TypeError('optimize must be a boolean');
  return { quality, subsampling: SUBSAMPLING[ss] | (optimize ? 0x100 : 0) };
}
/** stitch + the export with fileType 'jpg' (utils/canvas.js:205-221): resolves {width, height, jpeg: Buffer (a baseline JFIF file),
 *  plan}. opts.quality (1..100, default 90) and opts.subsampling ('420' default, '444') and opts.optimize (a boolean, default false: the file's own Huffman tables) choose the file, which is pinned byte for
 *  byte by include/imagestitch.h; alpha is not read. images may be Bitmap[]. The canvas never leaves the GPU. preview and devices
 *  do not apply. */
function stitchJpeg(images, direction, opts) {
  let a, h, j;
  try {
    const o = Object.assign({}, opts || {});
    j = jpegArgs(o); delete o.quality; delete o.subsampling; delete o.optimize;
    if (o.preview !== undefined && o.preview !== null) throw new TypeError('stitchJpeg: option preview does not apply (previews are built beside the PNG export)');
    if (o.devices !== undefined && o.devices !== null) throw new TypeError('stitchJpeg: option devices does not apply (the JPEG export runs on one GPU)');
    h = bitmapHandles(images, o); a = args(images, direction, o);
  } catch (e) { return Promise.reject(e); }
  if (!a[0].length) return Promise.resolve(null);
  return runStitch(opts, h, a, j, [], []);
}
/** Baseline JFIF file of RGBA8 pixels, encoded on the GPU: encodeJpeg(data, width, height, {quality, subsampling}). Synchronous. */
function encodeJpeg(data, width, height, opts) { const j = jpegArgs(opts); return native.encodeJpeg(data, width, height, j.quality, j.subsampling); }
/** opts.pngLevel: 0 = stored deflate blocks (file = raw size, fastest), 1 = Paeth + run-length + Huffman on the GPU
 *  (photographs about half, screenshots a few per cent). A process-wide setting of the native context. */
function pngLevel(opts) { if (opts && opts.pngLevel !== undefined && opts.pngLevel !== null) native.setPngLevel(opts.pngLevel | 0); }
function setPngLevel(level) { native.setPngLevel(level | 0); }
/** The native value of opts[key], one of the names of `table` (null: not given); anything else is a TypeError before any native call. */
function pngOption(opts, key, table, message) {
  const v = opts ? opts[key] : undefined;
  if (v === undefined || v === null) return null;
  if (typeof v !== 'string' || !Object.prototype.hasOwnProperty.call(table, v)) throw new TypeError(message);
  return table[v];
}
/** setPngColor / setPngFilter / setPngMatch: the option's check, then its native setter (a missing value is refused too). */
function pngSetter(of, key, message, apply) {
  return (value) => {
    const v = of({ [key]: value });
    if (v === null) throw new TypeError(message);
    native[apply](v);
  };
}
/** opts.pngColor: 'rgba' = colour type 6 (default), 'rgb' = colour type 2 - alpha is not read (every stitched canvas is opaque; a
 *  caller with a translucent one composites it first), pngLevel 1 only: 12-17 per cent fewer bytes on photographs. A process-wide
 *  setting of the native context, like pngLevel; an unknown value is a TypeError before any native call. */
const PNG_COLOR = { rgba: 0, rgb: 1 };             // IST_PNG_RGBA / IST_PNG_RGB
const PNG_COLOR_ERR = "pngColor must be 'rgba' or 'rgb'";
function pngColorOf(opts) { return pngOption(opts, 'pngColor', PNG_COLOR, PNG_COLOR_ERR); }
/** opts.pngFilter: 'paeth' = filter type 4 on every row (default), 'adaptive' = a type per row, chosen on the GPU by the least sum of
 *  absolute residuals (include/imagestitch.h states the rule), pngLevel 1 only: 6-7 per cent fewer bytes on photographs, 1-4 on flat
 *  content. A process-wide setting of the native context, like pngColor; an unknown value is a TypeError before any native call. */
const PNG_FILTER = { paeth: 0, adaptive: 1 };      // IST_PNG_FILTER_PAETH / IST_PNG_FILTER_ADAPTIVE
const PNG_FILTER_ERR = "pngFilter must be 'paeth' or 'adaptive'";
function pngFilterOf(opts) { return pngOption(opts, 'pngFilter', PNG_FILTER, PNG_FILTER_ERR); }
/** opts.pngMatch: 'run' = runs of equal bytes inside a 64-byte span (default), 'window' = a chunk also copies from its earlier spans,
 *  found on the GPU (include/imagestitch.h states the rule), pngLevel 1 only: never a larger file, half the bytes on rendered text
 *  (profiles/r17_png_match.json), a slower encoder. A process-wide setting of the native context, like pngColor; an unknown value is a TypeError
 *  before any native call. */
const PNG_MATCH = { run: 0, window: 1 };      // IST_PNG_MATCH_RUN / IST_PNG_MATCH_WINDOW
const PNG_MATCH_ERR = "pngMatch must be 'run' or 'window'";
function pngMatchOf(opts) { return pngOption(opts, 'pngMatch', PNG_MATCH, PNG_MATCH_ERR); }
function pngForm(opts) {
  const c = pngColorOf(opts), f = pngFilterOf(opts), m = pngMatchOf(opts);          // (all checked before the first native call)
  pngLevel(opts);
  if (c !== null) native.setPngColor(c);
  if (f !== null) native.setPngFilter(f);
  if (m !== null) native.setPngMatch(m);
}
const setPngMatch = pngSetter(pngMatchOf, 'pngMatch', PNG_MATCH_ERR, 'setPngMatch');
const setPngFilter = pngSetter(pngFilterOf, 'pngFilter', PNG_FILTER_ERR, 'setPngFilter');
const setPngColor = pngSetter(pngColorOf, 'pngColor', PNG_COLOR_ERR, 'setPngColor');
/** PNG file bytes -> {width, height, data} (RGBA8, straight alpha). Host decode: the Image.src step for 'png' inputs
 *  (utils/canvas.js:27-121; SUPPORTED_IMAGE_TYPES, index.js:4). JPEG / WebP / HEIC are not built: err.code '-7'. */
function decodePng(file) { return native.decodePng(file); }
/** PNG or JPEG file bytes -> {width, height, orientation, opaque, data}. JPEG (baseline): Huffman decoding on the host,
 *  IDCT / chroma upsampling / colour conversion on the GPU; orientation = EXIF tag 0x0112 (what getImageInfo feeds the
 *  planner, index.js:734). WebP / HEIC reject with err.code '-7'. */
function decodeImage(file) { return native.decodeImage(file); }
/** File to file (PNG and JPEG inputs): decode -> stitch -> PNG export. Resolves {width, height, png, plan}; writes
 *  outPath when given. A file that does not decode rejects with '图片N解码异常' like index.js:1512-1514. */
async function stitchFiles(paths, direction, opts, outPath) {
  const fs = require('fs');
  const a = args([], direction, opts, true);
  const pv = previewArgs(opts);
  pngColorOf(opts);
  pngFilterOf(opts);
  pngMatchOf(opts);
  const profile = colorProfileOf(opts);
  if (!paths || !paths.length) return null;
  const files = paths.map((p) => fs.readFileSync(p));
  // one native call: Huffman / inflate on host threads, reconstruction + stitch + PNG on the GPU, buffers stay in HBM
  const res = await withProgress(opts, () => { pngForm(opts); return native.stitchFiles(files, a[1], a[2], a[3], a[4], a[5], pv[0], pv[1], profile); });
  if (res && outPath) fs.writeFileSync(outPath, res.png);
  return res;
}
/** Lossless PNG of RGBA8 pixels, encoded on the GPU. */
function encodePng(data, width, height, opts) { pngForm(opts); return native.encodePng(data, width, height); }
function plan(images, direction, opts) {
  bitmapHandles(images, opts);                        // (the all-or-none rule; a Bitmap carries the fields the planner reads)
  const a = args(images, direction, opts);
  return native.plan(a[0], a[1], a[2], a[3], a[4]);
}

module.exports = { stitch: withOverlap(stitch), stitchSync: withOverlapSync(stitchSync), stitchBatch, stitchBatchSync, stitchPngBatch, stitchPngBatchSync, stitchJpegBatch, stitchJpegBatchSync, stitchPng: withOverlap(stitchPng), stitchJpeg: withOverlap(stitchJpeg), stitchFiles, encodePng, encodeJpeg, setPngLevel, setPngColor, setPngFilter, setPngMatch, decodePng, decodeImage, plan,
                   decodeBitmaps, joinJpegCheck, joinJpeg, imageColor, decodeScaleFit, uploadBitmap, thumbnails, debugBitmapBytes, findOverlaps, findOverlapsSync, overlapRows, Bitmap, native, DIRECTION, MODE, FILTER, PLATFORM, SPLIT };
