"""Host-side mirror of the reference's stitch surface, over the C-ABI (no pixel arithmetic in Python).

Reference: Page.onStitch (miniprogram-stitch/miniprogram/pages/index/index.js:1186-1633) reads
this.data.{images, direction, gap, verticalStitchMode, horizontalStitchMode}; here that is
`stitch(images, direction, opts)` with opts = {mode, gap, platform, maxSide, maxPixels, superSample, filter}.

Two ways in:
  stitch(images, direction, opts)      host RGBA8 arrays in, host RGBA8 array out   (ist_stitch_rgba8)
  Stitcher(device).compile(...)        device-resident: torch CUDA tensors in/out, one fused launch per call
and their batched forms: stitch_batch(requests) (ist_stitch_rgba8_batch), stitch_png_batch(requests) (ist_stitch_png_batch),
launch_jobs(jobs, srcs, outs) (ist_jobs_launch), encode_png_batch_device(canvases) (ist_png_encode_batch_device),
stitch_jpeg_batch(requests) (ist_stitch_jpeg_batch) and encode_jpeg_batch_device(canvases) (ist_jpeg_encode_batch_device).
Resident bitmaps (ist_bitmap_*): decode_bitmaps(files) / upload_bitmap(image) keep images in HBM, and plan / stitch / stitch_png take
a list of them in place of host images, so a restitch (reordered, other direction, new gap) uploads and decodes nothing.
Previews (ist_preview_*): opts['preview'] = (box_w, box_h) on stitch_png / stitch_files adds the canvas shrunk to fit that box to the
result, reduced from HBM beside the export; Bitmap.preview(box_w, box_h) is a thumbnail of a resident bitmap; preview_device(tensor,
pw, ph) is the device-to-device form and preview_fit(w, h, box_w, box_h) the fit rule.
Thumbnails (ist_thumb_*): thumbnails(bitmaps, cell) is the page's grid of chosen images - every bitmap cropped to the cell's aspect
ratio ('fill') or fitted into it ('fit'), turned by its EXIF orientation and shrunk, all in one launch pair and one copy down;
thumbnails_device(tensors, cell) is the device-to-device form and thumbnail_layout(descs, cell, mode) the rule.

What callers bring is judged in one place each, before any context is asked for: host pixels by _host_sources (type, stored size, and a
view with padded rows is read where it is - only reversed, repeated or interleaved layouts are copied, once), canvases in HBM by
_check_canvas, an encoder's output tensor by _file_out.  _plan_args / _plan_size are the argument run and the epilogue of every
planning call, _stitch the one choice of entry point behind stitch / stitch_png / stitch_jpeg, _run_batch the three batches' call.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L

_DIRECTIONS = {"vertical": L.VERTICAL, "horizontal": L.HORIZONTAL}
_MODES = {"min": L.MODE_MIN, "max": L.MODE_MAX, "original": L.MODE_ORIGINAL}
_FILTERS = {"nearest": L.FILTER_NEAREST, "bilinear": L.FILTER_BILINEAR, "area": L.FILTER_AREA, "cubic": L.FILTER_CUBIC}
FILTER_EDGE_AA = 0x100


def edge_aa_of(o):
    """Coverage rule for fractional rectangle edges.  Unset: ON whenever a reference platform's plan is requested
    (opts.platform: the reference's own default behaviour scales the canvas by superSample 2.2 / 2.6 for fewer than 7
    images, index.js:1363,1426-1428, and leaves the cursor unrounded when gap > 0 and scaleDown < 1, :1432, so fractional
    edges are the normal case there and a Canvas raster anti-aliases them); OFF for the lifted MI355X default, whose
    plans have integer edges unless a gap meets a shrink, so that every output pixel is owned by exactly one image."""
    v = o.get("edgeAA")
    return (o.get("platform") is not None) if v is None else bool(v)


def _filter_of(o):
    return _FILTERS[o["filter"]] | (FILTER_EDGE_AA if edge_aa_of(o) else 0)
_PLATFORMS = {"ios": L.PLATFORM_IOS, "android": L.PLATFORM_ANDROID, "devtools": L.PLATFORM_OTHER,
              "windows": L.PLATFORM_OTHER, "mac": L.PLATFORM_OTHER, "other": L.PLATFORM_OTHER}

DEFAULT_OPTS = {
    "mode": "min",          # data.verticalStitchMode / horizontalStitchMode default (index.js:19-20)
    "gap": 0,               # data.gap default (index.js:17)
    "filter": "bilinear",   # imageSmoothingEnabled = true (index.js:1416-1418); 'nearest' = false; 'area' = opt-in box average of minified axes (IST_FILTER_AREA);
                            # 'cubic' = opt-in Catmull-Rom on axes that do not shrink, the box of 'area' on those that do (IST_FILTER_CUBIC)
    "platform": None,       # None: MI355X default = caps lifted; 'ios' / 'android' / 'devtools' reproduce the phone caps
    "maxSide": None,        # deviceMaxCanvasSize override
    "maxPixels": None,      # deviceMaxCanvasPixels override
    "superSample": None,    # None: 1 when platform is None, reference rule (index.js:1363) otherwise
    "edgeAA": None,         # anti-alias fractional rectangle edges by area coverage (IST_FILTER_EDGE_AA); None: on iff `platform` is given (edge_aa_of)
    "pngLevel": None,       # PNG export form of the *_png / stitch_files calls: 0 stored, 1 compressed on the GPU; None = DEFAULT_PNG_LEVEL
    "pngColor": None,       # PNG colour form of the same calls: 'rgba' (colour type 6) or 'rgb' (colour type 2: alpha is not read; level 1 only); None = 'rgba'
    "pngMatch": None,       # PNG matches of the same calls: 'run' (runs of equal bytes inside a 64-byte span) or 'window' (also copies from earlier spans of the chunk, found on the GPU; level 1 only); None = 'run'
    "pngFilter": None,      # PNG row filters of the same calls: 'paeth' (type 4 on every row) or 'adaptive' (a type per row, chosen on the GPU; level 1 only); None = 'paeth'
    "devices": None,        # list of GPU indices (devices[0] = root): shard the stitch over them from this one process (ist_stitch_rgba8_multi)
    "preview": None,        # (box_w, box_h): stitch_png / stitch_files also return the canvas shrunk to fit that box (the redraw into the preview
                            # node, index.js:1597-1603), as result['preview'], HxWx4 uint8.  Refused where no canvas stays in HBM behind an export.
    "colorProfile": None,   # stitch_files: 'ignore' (pixels as decoded) or 'srgb' (a file tagged with a matrix/TRC ICC profile - Display P3, Adobe RGB - is
                            # converted to sRGB on the GPU behind its decode; include/imagestitch.h "colour profiles"); None = 'ignore'
    "overlap": None,        # 'auto', or a dict of tolerance / min_rows / min_informative: a vertical strip of Bitmaps (scrolled screenshots) is stitched
                            # without the bars and the overlaps its neighbours share (find_overlaps, crop_overlaps); the result also has 'overlaps'
    "split": "auto",        # with devices: "image" (image i -> devices[i mod n], BASELINE configs[3]), "band" (equal output rows per device, cut draw
                            # by draw), "rows" (device s owns a band of canvas rows across ALL draws: full-width bands for horizontal strips and
                            # centred rects too, index.js:1540-1553), "auto" = "image" when its parts are full-width (vertical min / max), else "rows"
}

_SPLITS = {"image": L.SPLIT_IMAGE, "band": L.SPLIT_BAND, "rows": L.SPLIT_ROWS, "auto": L.SPLIT_AUTO}

DEFAULT_PNG_LEVEL = 1
PNG_COLORS = {"rgba": 0, "rgb": 1}           # IST_PNG_RGBA / IST_PNG_RGB
PNG_FILTERS = {"paeth": 0, "adaptive": 1}    # IST_PNG_FILTER_PAETH / IST_PNG_FILTER_ADAPTIVE
PNG_MATCHES = {"run": 0, "window": 1}        # IST_PNG_MATCH_RUN / IST_PNG_MATCH_WINDOW


def _png_color(color):
    """IST_PNG_* of a pngColor / color= value (None: RGBA), checked before any library call"""
    if color is None:
        return PNG_COLORS["rgba"]
    if not isinstance(color, str) or color not in PNG_COLORS:
        raise ValueError("pngColor must be 'rgba' or 'rgb', not %r" % (color,))
    return PNG_COLORS[color]


def _png_filter(row_filter):
    """IST_PNG_FILTER_* of a pngFilter / row_filter= value (None: Paeth), checked before any library call"""
    if row_filter is None:
        return PNG_FILTERS["paeth"]
    if not isinstance(row_filter, str) or row_filter not in PNG_FILTERS:
        raise ValueError("pngFilter must be 'paeth' or 'adaptive', not %r" % (row_filter,))
    return PNG_FILTERS[row_filter]


def _png_match(match):
    """IST_PNG_MATCH_* of a pngMatch / match= value (None: runs), checked before any library call"""
    if match is None:
        return PNG_MATCHES["run"]
    if not isinstance(match, str) or match not in PNG_MATCHES:
        raise TypeError("pngMatch must be 'run' or 'window', not %r" % (match,))
    return PNG_MATCHES[match]


def _png_form(level=None, color=None, row_filter=None, match=None):
    """(level, IST_PNG_*, IST_PNG_FILTER_*, IST_PNG_MATCH_*) of a call's PNG options, checked - colour, filter, match, level: in that
    order - before any library call.  level None: DEFAULT_PNG_LEVEL."""
    form = _png_color(color), _png_filter(row_filter), _png_match(match)
    return (int(DEFAULT_PNG_LEVEL if level is None else level),) + form


def _opts_png_form(o):
    return _png_form(o["pngLevel"], o["pngColor"], o["pngFilter"], o["pngMatch"])


def debug_png_grid(w, h, color="rgba"):
    """(n_chunks, rows_per_chunk (0: pieces of a row), pieces_per_row, piece_px) of the compressing encoder's chunk grid for a w x h
    canvas in a colour form (ist_debug_png_grid).  Pure CPU."""
    out = (C.c_int64 * 4)()
    L.check(L.lib.ist_debug_png_grid(int(w), int(h), _png_color(color), out))
    return tuple(int(v) for v in out)


def _limits(opts):
    lim = L.Limits()
    if opts.get("platform") is None:
        L.lib.ist_limits_unlimited(C.byref(lim))
    else:
        L.lib.ist_limits_default(_PLATFORMS[opts["platform"]], C.byref(lim))
    if opts.get("maxSide") is not None:
        lim.max_side = float(opts["maxSide"])
    if opts.get("maxPixels") is not None:
        lim.max_pixels = float(opts["maxPixels"])
    if opts.get("superSample") is not None:
        lim.max_super_sample = float(opts["superSample"])
    return lim


def _merge(opts, overlap=False, color=False):
    o = dict(DEFAULT_OPTS)
    if opts:
        unknown = set(opts) - set(o)
        if unknown:
            raise TypeError("unknown stitch option(s): %s" % sorted(unknown))
        o.update(opts)
    if o["overlap"] is not None and not overlap:
        raise TypeError(_OVERLAP_NEEDS)
    if o["colorProfile"] is not None and not color:
        raise TypeError(_COLOR_NEEDS)
    return o


_COLOR_NEEDS = ("the 'colorProfile' option applies to stitch_files: a profile comes with a file, so the conversion belongs to the decode "
                "(decode_bitmaps / decode_files_device take profile=); raw pixels carry none")
COLOR_PROFILES = {"ignore": L.COLOR_PROFILE_IGNORE, "srgb": L.COLOR_PROFILE_SRGB}
COLOR_KINDS = ("none", "identity", "convert", "unsupported")      # IST_COLOR_*


def _color_profile(profile):
    """IST_COLOR_PROFILE_* of a colorProfile / profile= value (None: ignore), checked before any library call"""
    if profile is None:
        return COLOR_PROFILES["ignore"]
    if not isinstance(profile, str) or profile not in COLOR_PROFILES:
        raise ValueError("colorProfile must be 'ignore' or 'srgb', not %r" % (profile,))
    return COLOR_PROFILES[profile]


_OVERLAP_NEEDS = ("the 'overlap' option applies to stitch / stitch_png / stitch_jpeg of a vertical strip of Bitmaps "
                  "(upload_bitmap / decode_bitmaps): the overlaps are searched where the pixels are resident")


def _overlap_opts(value):
    """the keyword arguments of find_overlaps for an 'overlap' option value ('auto' or a dict of them), checked before any library call"""
    if value == "auto":
        return {}
    if not isinstance(value, dict) or set(value) - {"tolerance", "min_rows", "min_informative"}:
        raise TypeError("overlap must be 'auto' or a dict of tolerance / min_rows / min_informative, not %r" % (value,))
    return dict(value)


def _no_preview(o, who, why):
    if o.get("preview") is not None:
        raise TypeError("%s: the 'preview' option does not apply (%s)" % (who, why))


def _preview_arg(o):
    """the ist_preview of a call whose opts ask for one, or None"""
    box = o.get("preview")
    if box is None:
        return None
    if o.get("devices"):
        raise TypeError("the 'preview' option does not apply with devices= (the canvas of a device group is assembled band by band; "
                        "previews run on one GPU)")
    try:
        bw, bh = box
        bw, bh = float(bw), float(bh)
    except (TypeError, ValueError):
        raise TypeError("preview: expected (box_w, box_h)")
    pv = L.Preview()
    pv.box_w, pv.box_h = bw, bh
    return pv


def _take_preview(pv):
    """HxWx4 uint8 view of the preview an *_png_preview call returned (a pinned block of the pool; ist_free when the last view dies)"""
    return _take_pixels(pv.pixels, int(pv.width), int(pv.height))


def preview_fit(w, h, box_w, box_h):
    """(pw, ph) of a w x h image fitted into a box (ist_preview_fit; index.js:1600-1602, each side at least 1).  Pure CPU."""
    pw, ph = C.c_int32(0), C.c_int32(0)
    L.check(L.lib.ist_preview_fit(int(w), int(h), float(box_w), float(box_h), C.byref(pw), C.byref(ph)))
    return pw.value, ph.value


def preview_device(tensor, pw, ph, out=None, stream=None, opaque=False):
    """An HxWx4 uint8 CUDA tensor (any row pitch) shrunk to ph x pw x 4 on its device (ist_preview_device): what one drawImage of it
    into a fresh pw x ph canvas reads back under filter 'area'.  Asynchronous on `stream` (default: the tensor's current stream).
    opaque: the caller's hint that every alpha byte is 255."""
    import torch
    _check_canvas(tensor, "preview_device: ")
    pw, ph = int(pw), int(ph)
    if pw < 1 or ph < 1:
        raise L.StitchError(-1, "preview_device: the preview must be at least 1 x 1")
    if out is None:
        out = torch.empty((ph, pw, 4), dtype=torch.uint8, device=tensor.device)
    elif (out.dtype != torch.uint8 or out.dim() != 3 or tuple(out.shape) != (ph, pw, 4) or out.stride(2) != 1 or out.stride(1) != 4 or
          out.device != tensor.device):
        raise TypeError("preview_device: out must be a %d x %d x 4 uint8 tensor with dense pixels on the source's device" % (ph, pw))
    st = stream if stream is not None else torch.cuda.current_stream(tensor.device)
    L.check(L.lib.ist_preview_device(_ctx(tensor.device.index or 0), C.c_void_p(tensor.data_ptr()), tensor.stride(0), int(tensor.shape[1]),
                                     int(tensor.shape[0]), 1 if opaque else 0, C.c_void_p(out.data_ptr()), out.stride(0),
                                     pw, ph, C.c_void_p(st.cuda_stream)))
    return out


_THUMB_MODES = {"fill": L.THUMB_FILL, "fit": L.THUMB_FIT}


def _thumb_spec(cell, mode, orient):
    try:
        tw, th = cell
        tw, th = int(tw), int(th)
    except (TypeError, ValueError):
        raise TypeError("thumbnails: expected cell = (width, height)")
    if mode not in _THUMB_MODES:
        raise ValueError("thumbnails: mode must be 'fill' or 'fit'")
    return L.ThumbSpec(tw, th, _THUMB_MODES[mode], 1 if orient else 0)


def _thumb_items(items, n):
    return [{"width": int(t.width), "height": int(t.height), "offset": int(t.offset), "window": (int(t.src_x), int(t.src_y), int(t.src_w), int(t.src_h)),
             "turn": int(t.turn)} for t in items[:n]]


def thumbnail_layout(descs, cell, mode, orient=True):
    """The thumbnail rule (ist_thumb_layout; pure CPU) for a list of images as stitch() takes them, Bitmaps, or (width, height[,
    orientation]) tuples: per image {'width', 'height'} of the thumbnail, its 'offset' in the output block, the 'window' (x, y, w, h) of
    the STORED pixels it shows and the 'turn' (TURN_FLIP_X | TURN_FLIP_Y mirror the shrunk window, then TURN_TRANSPOSE swaps its axes)."""
    n = len(descs)
    arr = (L.ImageDesc * max(1, n))()
    for i, d in enumerate(descs):
        if isinstance(d, Bitmap):
            arr[i] = d._desc
        elif isinstance(d, tuple):
            arr[i] = L.ImageDesc(int(d[0]), int(d[1]), int(d[2]) if len(d) > 2 else 1, 0, 0, 0, 0)
        else:
            arr[i] = _descs([d])[0]
    items = (L.ThumbItem * max(1, n))()
    spec = _thumb_spec(cell, mode, orient)
    L.check(L.lib.ist_thumb_layout(arr, n, C.byref(spec), items, None))
    return _thumb_items(items, n)


def thumbnails_device(tensors, cell, mode="fill", orientations=None, opaque=False, out=None, stream=None, orient=True):
    """HxWx4 uint8 CUDA tensors (any row pitch, one device) -> their thumbnails for a cell (width, height), on the device
    (ist_thumbs_device): a list of HxWx4 views of ONE dense uint8 tensor.  orientations: EXIF orientation per tensor (default: all 1);
    orient=False ignores them (the stored pixels, as thumbnails(..., orient=False)).
    opaque: the caller's hint that every alpha byte is 255, one bool or one per tensor.  out: a 1-D uint8 CUDA tensor that holds the
    thumbnails back to back.  Asynchronous on `stream` (default: the device's current stream) unless an image is smaller than its
    cell on an axis."""
    import torch
    n = len(tensors)
    if n == 0:
        return []
    dev = _check_canvases(tensors, "thumbnails_device: ")
    orientations = [1] * n if orientations is None else list(orientations)
    opaques = [bool(opaque)] * n if isinstance(opaque, (bool, int)) else [bool(o) for o in opaque]
    if len(orientations) != n or len(opaques) != n:
        raise ValueError("thumbnails_device: one orientation (and one opaque flag) per tensor")
    descs = (L.ImageDesc * n)(*[L.ImageDesc(int(t.shape[1]), int(t.shape[0]), int(o or 0), 0, 0, 1 if q else 0, 0)
                                for t, o, q in zip(tensors, orientations, opaques)])
    spec = _thumb_spec(cell, mode, orient)
    items = (L.ThumbItem * n)()
    total = C.c_int64(0)
    L.check(L.lib.ist_thumb_layout(descs, n, C.byref(spec), items, C.byref(total)))
    if out is None:
        out = torch.empty((max(1, total.value),), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or out.stride(0) != 1 or out.device != dev or out.numel() < total.value:
        raise TypeError("thumbnails_device: out must be a dense 1-D uint8 tensor of at least %d bytes on the sources' device" % total.value)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    pitches = (C.c_size_t * n)(*[t.stride(0) for t in tensors])
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    L.check(L.lib.ist_thumbs_device(_ctx(dev.index or 0), descs, ptrs, pitches, n, C.byref(spec), C.c_void_p(out.data_ptr()), out.numel(), items,
                                    C.c_void_p(st.cuda_stream)))
    return [out[t.offset:t.offset + 4 * t.width * t.height].view(t.height, t.width, 4) for t in items]


def thumbnails(bitmaps, cell, mode="fill", orient=True):
    """Resident bitmaps -> their thumbnails for a cell (width, height) (ist_bitmaps_thumbs): a list of HxWx4 uint8 arrays, views of ONE
    block that came down in one copy.  mode 'fill' crops to the cell's aspect ratio (aspectFill), 'fit' fits the whole image into the
    cell (aspectFit); orient=False shows the stored pixels as Bitmap.preview does."""
    n = len(bitmaps)
    if n == 0:
        return []
    if not all(isinstance(b, Bitmap) for b in bitmaps):
        raise TypeError("thumbnails: expected Bitmaps (decode_bitmaps / upload_bitmap)")
    device = bitmaps[0].device
    spec = _thumb_spec(cell, mode, orient)
    bms = (C.c_void_p * n)(*[b.handle() for b in bitmaps])
    items = (L.ThumbItem * n)()
    out = C.POINTER(C.c_uint8)()
    L.check(L.lib.ist_bitmaps_thumbs(_ctx(device), bms, n, C.byref(spec), items, C.byref(out)))
    total = int(items[n - 1].offset) + 4 * int(items[n - 1].width) * int(items[n - 1].height)
    block = _take_pixels(out, total // 4, 1).reshape(-1)
    return [block[t.offset:t.offset + 4 * t.width * t.height].reshape(t.height, t.width, 4) for t in items]


def _descs(images):
    """images: list of {'width','height','orientation'?,'fileSize'?,'opaque'?,'data'?} or HxWx4 uint8 arrays."""
    arr = (L.ImageDesc * max(1, len(images)))()
    for i, im in enumerate(images):
        if isinstance(im, dict):
            data = im.get("data")
            w = im.get("width", data.shape[1] if hasattr(data, "shape") else 0)
            h = im.get("height", data.shape[0] if hasattr(data, "shape") else 0)
            bw = im.get("bmpWidth", data.shape[1] if hasattr(data, "shape") and data.ndim == 3 else 0)
            bh = im.get("bmpHeight", data.shape[0] if hasattr(data, "shape") and data.ndim == 3 else 0)
            arr[i] = L.ImageDesc(int(w or 0), int(h or 0), int(im.get("orientation", 1) or 0), int(bw or 0), int(bh or 0),
                                 1 if im.get("opaque") else 0, int(im.get("fileSize", 0) or 0))
        else:
            arr[i] = L.ImageDesc(int(im.shape[1]), int(im.shape[0]), 1, 0, 0, 0, 0)
    return arr


class StitchPlan:
    """Result of the planner (index.js stage 2 + rect loop).  Owns the C plan; freed on garbage collection."""

    def __init__(self, cplan, descs, n_images):
        self._c = cplan
        self._descs = descs
        self.n_images = n_images
        self.out_w, self.out_h = cplan.out_w, cplan.out_h
        self.scale_down, self.super_sample = cplan.scale_down, cplan.super_sample
        self.canvas_w, self.canvas_h = int(cplan.canvas_w), int(cplan.canvas_h)
        self.big_task = bool(cplan.big_task)
        self.rects = [{"image": r.image, "orientation": r.orientation, "dx": r.dx, "dy": r.dy, "dw": r.dw, "dh": r.dh}
                      for r in cplan.rects[:cplan.n_rects]]

    def ops(self):
        """The Canvas call sequence (white fill + one drawImage per rect with its CTM) as C ops."""
        n = self._c.n_rects + 1
        arr = (L.Op * n)()
        cnt = C.c_int(0)
        L.check(L.lib.ist_plan_ops(C.byref(self._c), self._descs, self.n_images, arr, C.byref(cnt)))
        return arr, cnt.value

    def ops_as_dicts(self):
        arr, n = self.ops()
        return [{"kind": "fill" if o.kind == 0 else "draw", "image": o.image, "m": list(o.m), "s": list(o.s),
                 "d": list(o.d), "rgba": tuple(o.rgba)} for o in arr[:n]]

    def __del__(self):
        try:
            L.lib.ist_plan_free(C.byref(self._c))
        except Exception:
            pass


def _plan_args(direction, o):
    """The argument run every planning entry point of the library shares, from (direction, merged opts): direction, mode, gap,
    limits, filter.  (ctypes passes the Limits by reference and the tuple keeps it alive over the call.)"""
    return _DIRECTIONS[direction], _MODES[o["mode"]], float(o["gap"] or 0), _limits(o), _filter_of(o)


def _plan_size(rc, cplan):
    """(canvas_w, canvas_h) of the plan a stitch call filled in, with the plan freed; None when there was nothing to stitch"""
    if rc == L.IST_NOTHING_TO_DO:
        return None
    w, h = int(cplan.canvas_w), int(cplan.canvas_h)
    L.lib.ist_plan_free(C.byref(cplan))
    return w, h


def plan(images, direction, opts=None):
    """Pure-CPU planner.  Returns a StitchPlan, or None when there is nothing to stitch (index.js:1189)."""
    o = _merge(opts)
    descs = _bitmap_descs(images) if _is_bitmap_request(images, o) else _descs(images)
    cplan = L.Plan()
    rc = L.check(L.lib.ist_plan_compute(descs, len(images), *_plan_args(direction, o)[:4], C.byref(cplan)))
    if rc == L.IST_NOTHING_TO_DO:
        return None
    return StitchPlan(cplan, descs, len(images))


_ctx_cache = {}


def _drain_at_exit():
    """Interpreter exit: wait for whatever the cached contexts still have in flight and hand the idle pinned result blocks
    back, so that no DMA of the library is pending when the HIP runtime (or a profiler attached to it: rocprofv3's copy
    tracing waited 30 s for completion callbacks otherwise) shuts down.  Contexts are NOT destroyed: jobs that are garbage
    collected later still refer to them."""
    for c in list(_ctx_cache.values()):
        try:
            L.lib.ist_ctx_sync(c)
        except Exception:
            pass
    try:
        L.lib.ist_pool_trim()
    except Exception:
        pass


import atexit  # noqa: E402
atexit.register(_drain_at_exit)


def _ctx(device=0):
    c = _ctx_cache.get(device)
    if c is None:
        c = L.lib.ist_ctx_create(int(device))
        if not c:
            raise L.StitchError(-5, L.last_error())
        _ctx_cache[device] = c
    return c


def _ctx_color(device, profile):
    """The context with its colour setting set (ist_ctx_set_color_profile): per context like the PNG form, so every call that decodes
    files sets it and never inherits the one before it.  An unknown value raises ValueError before the context is asked for."""
    p = _color_profile(profile)
    c = _ctx(device)
    L.check(L.lib.ist_ctx_set_color_profile(c, p))
    return c


def _ctx_png(device, form=None):
    """The context with its PNG export form set (ist_ctx_set_png_level, ist_ctx_set_png_color, ist_ctx_set_png_filter,
    ist_ctx_set_png_match - level, colour, row filter and matches together, so a call never inherits the colour, the filter or the
    matches of the one before it): a per-context setting, so concurrent callers that want different forms on one device should
    serialise.  form: what _png_form returned (a bare level stands for _png_form(level): that level in the default form)."""
    level, color, filt, mat = form if isinstance(form, tuple) else _png_form(form)
    c = _ctx(device)
    L.check(L.lib.ist_ctx_set_png_level(c, level))
    L.check(L.lib.ist_ctx_set_png_color(c, color))
    L.check(L.lib.ist_ctx_set_png_filter(c, filt))
    L.check(L.lib.ist_ctx_set_png_match(c, mat))
    return c


def _rgba(a, who=""):
    """The type and shape rule of host pixels: an HxWx4 uint8 array (anything np.asarray makes one of)"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
        raise TypeError(who + "expected an HxWx4 uint8 RGBA array")
    return a


def _host_rows(a, desc=None, who="", align=1):
    """The size and layout rule of one image's host pixels (after _rgba) -> (array to keep alive, its address, row pitch).  The array
    covers the stored size of its desc (bitmap_w x bitmap_h of the library, which reads that much).  A view goes as it is when its
    pixels are dense and its rows at least 4 * columns (and a multiple of `align`) apart; anything else - reversed or repeated rows,
    interleaved columns - is copied once."""
    if desc is not None:
        bw, bh = desc.bmp_width if desc.bmp_width > 0 else desc.width, desc.bmp_height if desc.bmp_height > 0 else desc.height
        if a.shape[0] < bh or a.shape[1] < bw:
            raise ValueError("%sthe pixels (%dx%d) are smaller than the bitmap (%dx%d)" % (who, a.shape[1], a.shape[0], bw, bh))
    pitch = a.strides[0]
    if a.strides[2] != 1 or a.strides[1] != 4 or pitch < 4 * a.shape[1] or pitch % align:
        a, pitch = np.ascontiguousarray(a), 4 * a.shape[1]
    return a, a.ctypes.data, pitch


def _host_sources(images, who="", descs=None, holes=False):
    """The one marshal of a request's host pixels -> (descs, ptrs, pitches, keep): images as stitch() takes them, each under the rules
    of _rgba and _host_rows, with `keep` what must stay alive during the call.  who: 'request k' in a batch.  Nothing here needs a
    device, so every entry point marshals before it asks for its context.  render_ops brings its own descs and has holes (None: an
    image no op draws); everywhere else missing pixels are the reference's decode failure."""
    n = len(images)
    each = (who + ", " if who else "") + "image %d: "
    arrays = []
    for i, im in enumerate(images):
        a = im.get("data") if isinstance(im, dict) else im
        if a is None and not holes:
            raise L.StitchError(-6, "%s图片%d解码异常" % (who + ": " if who else "", i))
        arrays.append(a if a is None else _rgba(a, each % i))
    if descs is None:
        descs = _descs(images)
    keep, ptrs, pitches = [], (C.c_void_p * max(1, n))(), (C.c_size_t * max(1, n))()
    for i, a in enumerate(arrays):
        if a is not None:
            a, ptrs[i], pitches[i] = _host_rows(a, descs[i], each % i)
            keep.append(a)
    return descs, ptrs, pitches, keep


def _stitch(images, direction, o, device, kind, jpeg=()):
    """stitch / stitch_png / stitch_jpeg behind their option rules: one library call chosen by (host images | Bitmaps) x kind, kind =
    'rgba8' (pixels; with devices= the sharded ist_stitch_rgba8_multi), 'png' (+ '_preview' when opts ask for one) or 'jpeg' (jpeg =
    (quality, IST_JPEG_*)): ist_stitch_<kind>[_preview] / ist_stitch_bitmaps_<kind>[_preview]."""
    n = len(images)
    if n == 0:
        return None
    if o["overlap"] is not None:
        kw = _overlap_opts(o["overlap"])
        if direction != "vertical" or not all(isinstance(im, Bitmap) for im in images) or o.get("devices") is not None:
            raise TypeError(_OVERLAP_NEEDS)
        records = find_overlaps(images, **kw) if n > 1 else []
        views = _crop_views(images, records)
        try:
            res = _stitch(views, direction, dict(o, overlap=None), device, kind, jpeg)
        finally:
            for v in views:
                v.close()
        if res is not None:
            res["overlaps"] = records
        return res
    if _is_bitmap_request(images, o):
        name, srcs = "ist_stitch_bitmaps_" + kind, ((C.c_void_p * n)(*[None if b is None else b.handle() for b in images]),)
    else:
        descs, ptrs, pitches, keep = _host_sources(images)
        name, srcs = "ist_stitch_" + kind, (descs, ptrs, pitches)
    pv = _preview_arg(o) if kind == "png" else None
    cplan, out, ln = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    tail = [C.byref(cplan), C.byref(out)] + ([] if kind == "rgba8" else [C.byref(ln)]) + ([] if pv is None else [C.byref(pv)])
    if kind == "rgba8" and o.get("devices"):
        devs = (C.c_int * len(o["devices"]))(*[int(d) for d in o["devices"]])
        name, head, mid = name + "_multi", (devs, len(devs)), (_SPLITS[o["split"]],)
    else:
        head, mid = (_ctx_png(device, _opts_png_form(o)) if kind == "png" else _ctx(device),), jpeg
    # (rgba8, what the N-API addon binds: plan, render, and the export as ONE DMA into a pinned block of the library's pool; the numpy
    # array below is a view of that block - no host copy - and returns it to the pool when it is garbage collected)
    fn = getattr(L.lib, name + ("_preview" if pv is not None else ""))
    size = _plan_size(L.check(fn(*head, *srcs, n, *_plan_args(direction, o), *mid, *tail)), cplan)
    if size is None:
        return None
    res = {"width": size[0], "height": size[1]}
    if kind == "rgba8":
        res["data"] = _take_pixels(out, *size)
    else:
        res[kind] = _take_png(out, ln)
    if pv is not None:
        res["preview"] = _take_preview(pv)
    return res


def stitch(images, direction, opts=None, device=0):
    """stitch(images, direction, opts) -> {'width', 'height', 'data'}: host arrays through the HIP path.

    images[i] = {'width', 'height', 'data': HxWx4 uint8 (RGBA, straight alpha), 'orientation'?: 1..8, 'fileSize'?}
    or simply an HxWx4 uint8 array; or a list of Bitmaps (decode_bitmaps / upload_bitmap: nothing is uploaded).  A view with padded
    rows is read where it is (_host_rows).  Returns None when images is empty (the reference returns early).
    """
    o = _merge(opts, overlap=True)
    _no_preview(o, "stitch", "the caller gets the pixels; stitch_png / stitch_files keep the canvas in HBM and can add its preview")
    return _stitch(images, direction, o, device, "rgba8")


_BATCH_REFUSED = ("devices", "split", "pngLevel", "pngColor", "pngFilter", "pngMatch", "preview", "overlap")      # a batch runs on one GPU; stitch_png_batch picks ONE PNG form for all its files; batch previews are not built


def _batch_requests(reqs, why):
    """ctypes StitchRequest array of stitch_batch / stitch_png_batch requests (+ what must stay alive during the call)"""
    n = len(reqs)
    creqs = (L.StitchRequest * n)()
    keep = []
    for k, r in enumerate(reqs):
        if not isinstance(r, (tuple, list)) or len(r) not in (2, 3):
            raise TypeError("request %d: expected (images, direction) or (images, direction, opts)" % k)
        images, direction = r[0], r[1]
        opts = r[2] if len(r) == 3 else None
        bad = sorted(x for x in (opts or {}) if x in _BATCH_REFUSED)
        if bad:
            raise TypeError("request %d: option(s) %s do not apply to a batch (%s)" % (k, bad, why))
        o = _merge(opts)
        if direction not in _DIRECTIONS:
            raise ValueError("request %d: direction must be 'vertical' or 'horizontal'" % k)
        if any(isinstance(im, Bitmap) for im in images):
            raise TypeError("request %d: Bitmaps do not apply to a batch (host images only)" % k)
        descs, ptrs, pitches, arrays = _host_sources(images, "request %d" % k)
        d, m, gap, lim, f = _plan_args(direction, o)
        keep.append((descs, ptrs, pitches, arrays, lim))
        creqs[k] = L.StitchRequest(descs, ptrs, pitches, len(images), d, m, gap, C.pointer(lim), f, 0)
    return creqs, keep


def _run_batch(fn, ctx, creqs, extra=(), key=None):
    """One batched stitch call and its result list: per request None (no images), the canvas (key None: HxWx4 uint8) or
    {'width', 'height', key: file bytes}"""
    n = len(creqs)
    plans, outs, lens = (L.Plan * n)(), (C.POINTER(C.c_uint8) * n)(), (C.c_int64 * n)()
    L.check(fn(ctx, creqs, n, *extra, plans, outs, *([] if key is None else [lens])))
    res = []
    for k in range(n):
        if not outs[k]:
            res.append(None)
            continue
        w, h = _plan_size(L.IST_OK, plans[k])
        res.append(_take_pixels(outs[k], w, h) if key is None else {"width": w, "height": h, key: _take_png(outs[k], C.c_int64(lens[k]))})
    return res


def stitch_batch(requests, device=0):
    """Many independent stitch() calls in one go (ist_stitch_rgba8_batch): the requests' tables go up in one copy, their
    canvases are rendered by one launch per kernel form, and each comes back into a pinned block of its own.

    requests[k] = (images, direction) or (images, direction, opts), each exactly as stitch() takes them.  Returns a list of
    HxWx4 uint8 arrays, byte-identical to stitch(*requests[k])['data'], with None for a request without images."""
    reqs = list(requests)
    if not reqs:
        return []
    creqs, keep = _batch_requests(reqs, "one GPU, pixels out")
    return _run_batch(L.lib.ist_stitch_rgba8_batch, _ctx(device), creqs)


def stitch_png_batch(requests, device=0, level=None, color=None, row_filter=None, match=None):
    """Many independent stitch_png() calls in one go (ist_stitch_png_batch): stitch_batch with a PNG file in place of each
    canvas.  Every sub-batch is rendered by one launch per kernel form and encoded by ONE compression launch; only the files
    cross PCIe.  requests as for stitch_batch (no per-request pngLevel or pngColor: `level` chooses the form for the whole batch, 0
    stored, 1 compressed, None = DEFAULT_PNG_LEVEL, `color` its colour form, 'rgba' or 'rgb' as opts['pngColor'], `row_filter` its row filters, 'paeth' or 'adaptive' as opts['pngFilter'], and `match` its matches, 'run' or 'window' as opts['pngMatch']).  Returns a list of {'width', 'height', 'png': bytes}, with None for a request
    without images; each file's zlib stream is stitch_png(*requests[k])['png']'s, byte for byte."""
    reqs = list(requests)
    if not reqs:
        return []
    form = _png_form(level, color, row_filter, match)
    creqs, keep = _batch_requests(reqs, "one GPU, one PNG form for the whole batch: level=, color=, row_filter=, match=")
    return _run_batch(L.lib.ist_stitch_png_batch, _ctx_png(device, form), creqs, key="png")


def launch_jobs(jobs, srcs, outs, stream=None):
    """Run compiled StitchJobs (Stitcher.compile) as ONE batch (ist_jobs_launch): one launch per kernel form on `stream`.
    srcs[k]: job k's source tensors (None for images it does not sample); outs[k]: its canvas tensor.  Asynchronous."""
    import torch
    n = len(jobs)
    if len(srcs) != n or len(outs) != n:
        raise ValueError("launch_jobs: jobs, srcs and outs must have the same length")
    if n == 0:
        return
    st = stream if stream is not None else torch.cuda.current_stream(outs[0].device)
    handles = (C.c_void_p * n)(*[j._h for j in jobs])
    counts = (C.c_int * n)(*[j.n_images for j in jobs])
    total = max(1, sum(j.n_images for j in jobs))
    ptrs, pitches = (C.c_void_p * total)(), (C.c_size_t * total)()
    at = 0
    for j, ss in zip(jobs, srcs):
        if len(ss) > j.n_images:
            raise ValueError("launch_jobs: more sources than the job has images")
        for i, t in enumerate(ss):
            ptrs[at + i] = 0 if t is None else t.data_ptr()
            pitches[at + i] = 0 if t is None else t.stride(0)
        at += j.n_images
    dst = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    dpitch = (C.c_size_t * n)(*[o.stride(0) for o in outs])
    L.check(L.lib.ist_jobs_launch(handles, n, ptrs, pitches, counts, dst, dpitch, C.c_void_p(st.cuda_stream)))


def _take_pixels(out, w, h):
    """HxWx4 uint8 view of a library-owned result; ist_free runs when the last view dies."""
    import weakref
    raw = (C.c_uint8 * (w * h * 4)).from_address(C.addressof(out.contents))
    weakref.finalize(raw, L.lib.ist_free, C.cast(out, C.c_void_p))
    return np.frombuffer(raw, np.uint8).reshape(h, w, 4)


def render_ops(canvas_w, canvas_h, ops, n_ops, descs, srcs, filter="bilinear", clear=(0, 0, 0, 0), region=None, device=0):
    """A recorded Canvas op list -> HxWx4 uint8 (ist_render_rgba8: what the Canvas-2D shim's export / getImageData binds).
    srcs: list of HxWx4 uint8 arrays (None for images no op draws)."""
    n = len(srcs)
    descs, ptrs, pitches, keep = _host_sources(srcs, descs=descs, holes=True)
    reg, rw, rh = None, int(canvas_w), int(canvas_h)
    if region is not None:
        x, y, w, h = [int(v) for v in region]
        reg = C.byref(L.Region(x, y, w, h))
        rw, rh = min(canvas_w, x + w) - max(0, x), min(canvas_h, y + h) - max(0, y)
    data = np.empty((rh, rw, 4), np.uint8)
    clr = (C.c_uint8 * 4)(*clear)
    f = (_FILTERS[filter] if isinstance(filter, str) else int(filter))
    L.check(L.lib.ist_render_rgba8(_ctx(device), int(canvas_w), int(canvas_h), clr, ops, int(n_ops), descs, ptrs, pitches, n,
                                   f, reg, data.ctypes.data, data.strides[0]))
    return data


def stitch_via_c_abi(images, direction, opts=None, device=0):
    """stitch() with the result copied into ordinary Python-owned memory (the pinned block goes straight back to the pool)."""
    r = stitch(images, direction, opts, device)
    if r is not None:
        r["data"] = r["data"].copy()
    return r


def _take_png(out, n, copy=True):
    """The library's malloc'ed file - a PNG or, despite the name, a JPEG - as Python bytes (one copy), or with copy=False as a
    memoryview over the C buffer itself, released through ist_free when the view is garbage collected (a 146 MB file costs ~20 ms
    to copy)."""
    if copy:
        try:
            return C.string_at(out, n.value)
        finally:
            L.lib.ist_free(out)
    import weakref
    arr = (C.c_uint8 * n.value).from_address(C.addressof(out.contents))
    weakref.finalize(arr, L.lib.ist_free, C.cast(out, C.c_void_p))
    return memoryview(arr).cast("B")


def decode_png(data):
    """PNG file bytes -> HxWx4 uint8 RGBA (straight alpha).  Host decode (zlib + the PNG predictors); no GPU needed."""
    buf = bytes(data)
    w, h = C.c_int32(0), C.c_int32(0)
    L.check(L.lib.ist_png_info(buf, len(buf), C.byref(w), C.byref(h)))
    out = np.empty((h.value, w.value, 4), np.uint8)
    L.check(L.lib.ist_png_decode_rgba8(buf, len(buf), out.ctypes.data, out.strides[0], out.shape[0]))
    return out


def image_info(data):
    """(width, height, orientation) of a PNG or JPEG file; orientation = EXIF tag 0x0112 (0 when absent)."""
    buf = bytes(data)
    w, h, o = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L.check(L.lib.ist_image_info(buf, len(buf), C.byref(w), C.byref(h), C.byref(o)))
    return w.value, h.value, o.value


_SCALES = (1, 2, 4, 8)


def scaled_size(w, h, scale):
    """(sw, sh) of a w x h JPEG decoded at 1 / scale, scale in {1, 2, 4, 8}: ceil(w / scale), ceil(h / scale) (ist_jpeg_scaled_size).
    Pure CPU."""
    sw, sh = C.c_int32(0), C.c_int32(0)
    L.check(L.lib.ist_jpeg_scaled_size(int(w), int(h), int(scale), C.byref(sw), C.byref(sh)))
    return sw.value, sh.value


def decode_scale_fit(w, h, min_w, min_h):
    """The largest scale in {1, 2, 4, 8} at which a w x h file still decodes to at least min_w x min_h pixels, 1 if none does
    (ist_decode_scale_fit).  Pure CPU."""
    d = L.lib.ist_decode_scale_fit(int(w), int(h), int(min_w), int(min_h))
    L.check(d if d < 0 else 0)
    return d


def _scales(scale, blobs, who):
    """scale= of a decode call -> (one denominator per file, the C array or None for all 1).  JPEG files take the denominator, every
    other type decodes at 1 / 1."""
    n = len(blobs)
    ds = [int(d) for d in _per_file(scale, n, who + ": scale")]
    for i, d in enumerate(ds):
        if d not in _SCALES:
            raise L.StitchError(-1, "%s: the scale of image %d is %d, not 1, 2, 4 or 8" % (who, i, d))
    return ds, (None if all(d == 1 for d in ds) else (C.c_int32 * max(1, n))(*ds))


def _is_jpeg(buf):
    return buf[:2] == b"\xff\xd8"


def decode_image(data, device=0, scale=1, profile="ignore"):
    """PNG or JPEG file bytes -> HxWx4 uint8 RGBA.  JPEG: Huffman decoding on the host, IDCT / upsampling / colour
    conversion on the GPU.  The bitmap is returned as stored (EXIF orientation is applied by the stitch, like the
    reference's drawWithOrientation).  scale: 1, 2, 4 or 8 - a JPEG decodes at 1 / scale of its size (scaled_size), as
    libjpeg-turbo's decode-to-scale does, byte for byte; other file types decode at 1 / 1.
    profile: 'ignore' or 'srgb' - a JPEG tagged with an ICC profile the colour contract takes is converted to sRGB on the GPU.  PNG,
    WebP, BMP and GIF files are decoded on the host here and never reach the device: they are NOT converted by this call
    (decode_bitmaps and decode_files_device convert every file type)."""
    buf = bytes(data)
    _color_profile(profile)
    (d,), _ = _scales(scale, [buf], "decode_image")
    w, h, _ = image_info(buf)
    jpeg = _is_jpeg(buf)
    if jpeg and d > 1:
        w, h = scaled_size(w, h, d)
    out = np.empty((h, w, 4), np.uint8)
    ctx = _ctx_color(device, profile) if jpeg else None          # only JPEG needs the GPU
    if d == 1:
        L.check(L.lib.ist_image_decode_rgba8(ctx, buf, len(buf), out.ctypes.data, out.strides[0], out.shape[0]))
    else:
        L.check(L.lib.ist_image_decode_rgba8_scaled(ctx, buf, len(buf), d, out.ctypes.data, out.strides[0], out.shape[0]))
    return out


def decode_files_device(blobs, device=0, out=None, scale=1, profile="ignore"):
    """File bytes -> bitmaps in HBM (ist_decode_files_device): returns ([HxWx4 uint8 CUDA tensors], [image dicts for
    plan/compile]).  Baseline JPEG: Huffman decoding + reconstruction on the GPU; only the file bytes cross PCIe.
    out: optional list of preallocated tensors (one spare row behind each is the caller's business).
    scale: 1, 2, 4 or 8, one for all files or one per file: a JPEG decodes at 1 / scale (scaled_size); its dict then carries
    'bmpWidth' / 'bmpHeight' = the tensor's size beside the natural 'width' / 'height', which is what plan and compile expect.
    profile: 'ignore' or 'srgb' - a file tagged with an ICC profile the colour contract takes lands converted to sRGB."""
    import torch
    n = len(blobs)
    _color_profile(profile)
    ds, cden = _scales(scale, blobs, "decode_files_device")
    sizes = [image_info(b) for b in blobs]
    sizes = [scaled_size(w, h, d) + (o,) if d > 1 and _is_jpeg(b) else (w, h, o) for (w, h, o), d, b in zip(sizes, ds, blobs)]
    dev = torch.device("cuda", device)
    if out is None:
        out = [torch.empty((h + 1, w, 4), dtype=torch.uint8, device=dev)[:h] for (w, h, _) in sizes]
    else:
        # the library writes `out` from its own streams: what the caller queued on these tensors (a launch still reading the
        # previous bitmaps) must be done first (include/imagestitch.h, ist_decode_files_device "Ordering")
        for d in {t.device for t in out}:
            torch.cuda.current_stream(d).synchronize()
    files = (C.c_char_p * n)(*blobs)
    lens = (C.c_int64 * n)(*[len(b) for b in blobs])
    dst, pitch, rows = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int64 * n)()
    for i, t in enumerate(out):
        dst[i], pitch[i], rows[i] = t.data_ptr(), t.stride(0), t.shape[0]
    descs = (L.ImageDesc * n)()
    ctx = _ctx_color(device, profile)
    if cden is None:
        L.check(L.lib.ist_decode_files_device(ctx, files, lens, n, dst, pitch, rows, descs))
    else:
        L.check(L.lib.ist_decode_files_device_scaled(ctx, files, lens, n, cden, dst, pitch, rows, descs))
    imgs = [{"width": d.width, "height": d.height, "orientation": d.orientation, "opaque": bool(d.opaque), "fileSize": d.file_size} for d in descs]
    for im, d in zip(imgs, descs):
        if d.bmp_width or d.bmp_height:
            im["bmpWidth"], im["bmpHeight"] = int(d.bmp_width), int(d.bmp_height)
    return out, imgs


def debug_jpeg_gpu_coefficients(blob, device=0):
    """The GPU Huffman decoder's coefficients of one file (ist_debug_jpeg_gpu_coefficients): {'ok', 'launches', 'planes'}, planes =
    one blocks_y x blocks_x x 64 int16 array per component (natural order, DC integrated, not dequantised), None when the decoder
    handed the file back (ok False).  Raises StitchError(-7) for a file the GPU decoder does not take."""
    info = L.JpegCoefInfo()
    L.check(L.lib.ist_debug_jpeg_gpu_coefficients(None, blob, len(blob), None, None, C.byref(info)))
    planes = [np.zeros((info.blocks_y[c], info.blocks_x[c], 64), np.int16) for c in range(info.ncomp)]
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    elems = (C.c_int64 * 3)(*[p.size for p in planes])
    L.check(L.lib.ist_debug_jpeg_gpu_coefficients(_ctx(device), blob, len(blob), ptrs, elems, C.byref(info)))
    return {"ok": bool(info.ok), "launches": int(info.launches), "planes": planes if info.ok else None}


PHASES = ("host_decode", "plan_arena", "entropy_gpu", "reconstruct", "stitch", "png", "d2h")


def last_phase_times(device=0):
    """{phase: ms} of the last file-pipeline call on the device's context (enable with set_phase_timing)."""
    ms = (C.c_double * 8)()
    L.check(L.lib.ist_ctx_last_timing(_ctx(device), ms, 8))
    return {k: ms[i] for i, k in enumerate(PHASES)}


def set_phase_timing(on, device=0):
    L.check(L.lib.ist_ctx_set_timing(_ctx(device), 1 if on else 0))


def stitch_files(paths, direction, opts=None, out_path=None, device=0, copy=True):
    """File to file, device-resident (ist_stitch_files_png): decode (Huffman / inflate on host threads, JPEG
    reconstruction on the GPU) -> plan (EXIF orientation from the file, like getImageInfo, index.js:734) -> one fused
    stitch launch -> PNG export on the GPU.  Only file bytes go in and PNG bytes come out over PCIe.
    Returns {'width','height','png'} and writes out_path when given.  The mini-program's whole onStitch: index.js:1441-1581."""
    o = _merge(opts, color=True)
    form = _opts_png_form(o)
    _color_profile(o["colorProfile"])
    n = len(paths)
    if n == 0:
        return None
    # the library reads the files itself (ist_stitch_paths_png: one parked worker per file, into blocks its context keeps).
    # (Reading nine 12 MP JPEGs into Python bytes cost ~1 ms of the call; opening and mapping them from Python still 0.2 ms.)
    cpaths = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    cplan, out, ln = L.Plan(), C.POINTER(C.c_uint8)(), C.c_int64(0)
    pv = _preview_arg(o)
    fn = L.lib.ist_stitch_paths_png if pv is None else L.lib.ist_stitch_paths_png_preview
    _ctx_color(device, o["colorProfile"])
    size = _plan_size(L.check(fn(_ctx_png(device, form), cpaths, n, *_plan_args(direction, o), C.byref(cplan), C.byref(out), C.byref(ln),
                                 *([] if pv is None else [C.byref(pv)]))), cplan)
    if size is None:
        return None
    w, h = size
    res = {"width": w, "height": h, "png": _take_png(out, ln, copy)}
    if pv is not None:
        res["preview"] = _take_preview(pv)
    if out_path:
        with open(out_path, "wb") as f:
            f.write(res["png"])
    return res


def encode_png(pixels, device=0, level=None, color=None, row_filter=None, match=None):
    """Lossless PNG of an HxWx4 uint8 array, encoded on the GPU (export step, utils/canvas.js:205-242).
    level 0: stored deflate blocks; 1: Paeth + run-length + Huffman (ist_ctx_set_png_level).  color 'rgba' (default, colour type 6) or
    'rgb' (colour type 2: alpha is not read; level 1 only - ist_ctx_set_png_color).  row_filter 'paeth' (default: filter type 4 on
    every row) or 'adaptive' (a type per row, chosen on the GPU by the least sum of absolute residuals; level 1 only -
    ist_ctx_set_png_filter; `filter` is the resampling filter, hence the name).  match 'run' (default: runs of equal bytes inside a
    64-byte span) or 'window' (a chunk also copies from its earlier spans, found on the GPU; never a larger file, half the bytes
    on rendered text (profiles/r17_png_match.json), a slower encoder; level 1 only - ist_ctx_set_png_match)."""
    form = _png_form(level, color, row_filter, match)
    a, ptr, pitch = _host_rows(_rgba(pixels))
    out, n = C.POINTER(C.c_uint8)(), C.c_int64(0)
    L.check(L.lib.ist_png_encode_rgba8(_ctx_png(device, form), ptr, pitch, a.shape[1], a.shape[0], C.byref(out), C.byref(n)))
    return _take_png(out, n)


def stitch_png(images, direction, opts=None, device=0):
    """stitch(images, direction, opts) with the reference's export: returns {'width','height','png': bytes}.  The
    canvas stays on the device; only the PNG crosses PCIe.  images are marshalled as stitch() marshals them (padded views are read
    where they are); they may be a list of Bitmaps."""
    o = _merge(opts, overlap=True)
    _opts_png_form(o)
    return _stitch(images, direction, o, device, "png")


def encode_png_device(canvas, out=None, stream=None, device=None, level=None, color=None, row_filter=None, match=None):
    """PNG of a canvas that is resident in HBM (HxWx4 uint8 CUDA tensor) into a CUDA uint8 tensor; returns (tensor, length).
    level, color, row_filter, match: as encode_png."""
    form = _png_form(level, color, row_filter, match)
    import torch
    _check_canvas(canvas, "encode_png_device: ")
    h, w = int(canvas.shape[0]), int(canvas.shape[1])
    out, off, dst, cap = _file_out(out, L.lib.ist_png_bound(w, h), canvas.device)
    st = stream if stream is not None else torch.cuda.current_stream(canvas.device)
    n = C.c_int64(0)
    dev = canvas.device.index if device is None else device
    L.check(L.lib.ist_png_encode_device(_ctx_png(dev or 0, form), C.c_void_p(canvas.data_ptr()), canvas.stride(0), w, h,
                                        C.c_void_p(dst), cap, C.byref(n), C.c_void_p(st.cuda_stream)))
    return out[off:off + n.value], n.value


JPEG_SUBSAMPLING = {"444": 0, "420": 1}      # IST_JPEG_444 / IST_JPEG_420
JPEG_OPTIMIZE = 0x100                        # IST_JPEG_OPTIMIZE, OR-ed into the subsampling


def _jpeg_args(quality, subsampling, optimize=False):
    """(quality, IST_JPEG_* [| IST_JPEG_OPTIMIZE]) of a JPEG export, checked: an integer quality 1..100, subsampling '420' or '444',
    optimize a bool (the file's own Huffman tables)"""
    if not isinstance(optimize, bool):
        raise TypeError("optimize: expected a bool")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)):
        raise TypeError("quality: expected an integer 1..100")
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality must be 1..100")
    if str(subsampling) not in JPEG_SUBSAMPLING:
        raise ValueError("subsampling must be '420' or '444'")
    return int(quality), JPEG_SUBSAMPLING[str(subsampling)] | (JPEG_OPTIMIZE if optimize else 0)


def encode_jpeg(pixels, quality=90, subsampling="420", device=0, optimize=False):
    """Baseline JFIF file (bytes) of an HxWx4 uint8 array, encoded on the GPU (ist_jpeg_encode_rgba8; the export with fileType 'jpg',
    utils/canvas.js:205-221).  Alpha is not read.  The file is pinned byte for byte by include/imagestitch.h.  optimize=True: the
    file carries the Huffman tables that are optimal for its own symbols (IST_JPEG_OPTIMIZE) - the same pixels in fewer bytes."""
    q, ss = _jpeg_args(quality, subsampling, optimize)
    a = _rgba(pixels)
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise TypeError("expected an HxWx4 uint8 RGBA array")
    a, ptr, pitch = _host_rows(a, align=4)
    out, n = C.POINTER(C.c_uint8)(), C.c_int64(0)
    L.check(L.lib.ist_jpeg_encode_rgba8(_ctx(device), ptr, pitch, a.shape[1], a.shape[0], q, ss, C.byref(out), C.byref(n)))
    return _take_png(out, n)


def encode_jpeg_device(canvas, quality=90, subsampling="420", out=None, stream=None, optimize=False):
    """JPEG of a canvas that is resident in HBM (HxWx4 uint8 CUDA tensor, any row pitch that is a multiple of 4) into a CUDA uint8
    tensor (ist_jpeg_encode_device); returns (tensor, length) like encode_png_device.  out: optional, ist_jpeg_bound + 16 bytes (the
    bound of the optimised file when optimize=True: it is the larger one)."""
    import torch
    q, ss = _jpeg_args(quality, subsampling, optimize)
    _check_canvas(canvas, "encode_jpeg_device: ")
    h, w = int(canvas.shape[0]), int(canvas.shape[1])
    out, off, dst, cap = _file_out(out, L.lib.ist_jpeg_bound(w, h, ss), canvas.device)
    st = stream if stream is not None else torch.cuda.current_stream(canvas.device)
    n = C.c_int64(0)
    L.check(L.lib.ist_jpeg_encode_device(_ctx(canvas.device.index or 0), C.c_void_p(canvas.data_ptr()), canvas.stride(0), w, h, q, ss,
                                         C.c_void_p(dst), cap, C.byref(n), C.c_void_p(st.cuda_stream)))
    return out[off:off + n.value], n.value


def stitch_jpeg(images, direction, opts=None, device=0):
    """stitch(images, direction, opts) with the JPEG export: returns {'width', 'height', 'jpeg': bytes} (ist_stitch_jpeg /
    ist_stitch_bitmaps_jpeg).  opts['quality'] (1..100, default 90), opts['subsampling'] ('420' default, or '444') and
    opts['optimize'] (a bool, default False: the file's own Huffman tables) choose the file; the canvas stays on the device and only the file crosses PCIe.  images as for stitch_png(): marshalled as stitch() marshals them,
    or a list of Bitmaps."""
    opts = dict(opts or {})
    jpeg = _jpeg_args(opts.pop("quality", 90), opts.pop("subsampling", "420"), opts.pop("optimize", False))
    o = _merge(opts, overlap=True)
    _no_preview(o, "stitch_jpeg", "previews are built beside the PNG export")
    if o.get("devices") is not None:
        raise TypeError("stitch_jpeg: devices= does not apply (the JPEG export runs on one GPU)")
    return _stitch(images, direction, o, device, "jpeg", jpeg)


def _per_file(value, n, name):
    """one value for all n files, or a sequence of length n"""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError("%s: expected one value or a sequence of length %d, got %d" % (name, n, len(value)))
        return list(value)
    return [value] * n


def encode_jpeg_batch_device(canvases, quality=90, subsampling="420", outs=None, stream=None, optimize=False):
    """JPEG files of many canvases resident in HBM (HxWx4 uint8 CUDA tensors of one device, any row pitch that is a multiple of 4) in
    one transform, one entropy and one gather launch per round (ist_jpeg_encode_batch_device).  quality and subsampling: one value for
    all files or a sequence of length n, and so is optimize (a batch may mix optimised and standard files).  outs: optional CUDA uint8 tensors of at least ist_jpeg_bound + 16 bytes each.  Returns
    [(tensor, length)], each file byte for byte what encode_jpeg_device gives for that canvas."""
    canvases = list(canvases)
    n = len(canvases)
    if n == 0:
        return []
    args = []
    for k, (q, s, o) in enumerate(zip(_per_file(quality, n, "quality"), _per_file(subsampling, n, "subsampling"), _per_file(optimize, n, "optimize"))):
        try:
            args.append(_jpeg_args(q, s, o))
        except (TypeError, ValueError) as e:
            raise type(e)("file %d: %s" % (k, e)) from None
    qs, ss = (C.c_int * n)(*[a[0] for a in args]), (C.c_int * n)(*[a[1] for a in args])
    return _encode_batch_device(L.lib.ist_jpeg_encode_batch_device, _ctx, "encode_jpeg_batch_device", canvases,
                                lambda k, w, h: L.lib.ist_jpeg_bound(w, h, ss[k]), outs, stream, (qs, ss))


def stitch_jpeg_batch(requests, device=0):
    """Many independent stitch_jpeg() calls in one go (ist_stitch_jpeg_batch): stitch_png_batch with a JPEG file in place of each
    PNG.  requests as for stitch_batch; each request's opts may carry 'quality' (1..100, default 90), 'subsampling' ('420'
    default, or '444') and 'optimize' (a bool, default False).  Returns a list of {'width', 'height', 'jpeg': bytes}, with None for a request without images; each file is
    stitch_jpeg(*requests[k])['jpeg'], byte for byte."""
    reqs = list(requests)
    if not reqs:
        return []
    n = len(reqs)
    plain, qs, ss = [], (C.c_int * n)(), (C.c_int * n)()
    for k, r in enumerate(reqs):
        if not isinstance(r, (tuple, list)) or len(r) not in (2, 3):
            raise TypeError("request %d: expected (images, direction) or (images, direction, opts)" % k)
        opts = dict(r[2] or {}) if len(r) == 3 else {}
        try:
            qs[k], ss[k] = _jpeg_args(opts.pop("quality", 90), opts.pop("subsampling", "420"), opts.pop("optimize", False))
        except (TypeError, ValueError) as e:
            raise type(e)("request %d: %s" % (k, e)) from None
        plain.append((r[0], r[1], opts))
    creqs, keep = _batch_requests(plain, "one GPU, JPEG files out")
    return _run_batch(L.lib.ist_stitch_jpeg_batch, _ctx(device), creqs, (qs, ss), "jpeg")


def encode_png_batch_device(canvases, outs=None, stream=None, level=None, color=None, row_filter=None, match=None):
    """PNG files of many canvases resident in HBM (HxWx4 uint8 CUDA tensors of one device, any row pitch) in ONE compression
    launch (ist_png_encode_batch_device).  outs: optional CUDA uint8 tensors of at least ist_png_bound + 16 bytes each.  Returns
    [(tensor, length)], each file byte for byte what encode_png_device gives for that canvas at the same level, color, row_filter and match."""
    form = _png_form(level, color, row_filter, match)
    return _encode_batch_device(L.lib.ist_png_encode_batch_device, lambda d: _ctx_png(d, form), "encode_png_batch_device", list(canvases),
                                lambda k, w, h: L.lib.ist_png_bound(w, h), outs, stream)


def _encode_batch_device(fn, ctx_of, who, canvases, bound, outs, stream, extra=()):
    """encode_png_batch_device / encode_jpeg_batch_device behind their own arguments: canvases under _check_canvases, one _file_out per
    file (bound(k, w, h): the size to allocate where the caller brought none), one call, [(tensor, length)]"""
    import torch
    n = len(canvases)
    if n == 0:
        return []
    if outs is not None and len(outs) != n:
        raise ValueError(who + ": canvases and outs must have the same length")
    dev = _check_canvases(canvases)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    src, pitch = (C.c_void_p * n)(), (C.c_size_t * n)()
    w, h = (C.c_int64 * n)(), (C.c_int64 * n)()
    dst, cap, ln = (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
    files = []
    for k, c in enumerate(canvases):
        src[k], pitch[k], h[k], w[k] = c.data_ptr(), c.stride(0), int(c.shape[0]), int(c.shape[1])
        o, off, dst[k], cap[k] = _file_out(None if outs is None else outs[k], bound(k, w[k], h[k]), dev, "file %d: " % k)
        files.append((o, off))
    L.check(fn(ctx_of(dev.index or 0), src, pitch, w, h, *extra, n, dst, cap, ln, C.c_void_p(st.cuda_stream)))
    return [(o[off:off + ln[k]], int(ln[k])) for k, (o, off) in enumerate(files)]


def _canvas_form(t, who=""):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 4 or t.stride(2) != 1 or t.stride(1) != 4:
        raise TypeError(who + "expected an HxWx4 uint8 CUDA tensor with dense pixels")


def _check_canvas(t, who="", device=None):
    """The rule of a canvas in HBM: a torch tensor, HxWx4 uint8 with dense pixels (any row pitch), on a GPU - on `device` where it
    shares a call with others.  Handing the library anything else as a device pointer is a GPU fault, not an error code."""
    _canvas_form(t, who)
    if not t.is_cuda:
        raise TypeError(who + "canvases must be CUDA tensors (host pixels: upload_bitmap, or the entry points that take arrays)")
    if device is not None and t.device != device:
        raise TypeError(who + "the canvases of one call must live on one device (%s, not %s)" % (device, t.device))


def _check_canvases(tensors, who=""):
    """_check_canvas for the canvases of one call, which share a device: the one returned.  The form of every canvas is judged
    before where any of them lives, so 'canvas k: ...' names a malformed one whatever the others are."""
    for k, t in enumerate(tensors):
        _canvas_form(t, "%scanvas %d: " % (who, k))
    for k, t in enumerate(tensors):
        _check_canvas(t, "%scanvas %d: " % (who, k), tensors[0].device)
    return tensors[0].device


def _file_out(out, cap, device, who=""):
    """Where an encoder writes its file -> (tensor, offset, pointer, capacity): `out`, a dense 1-D uint8 CUDA tensor on the canvas's
    device, or cap + 16 fresh bytes; the file starts at the first 16-byte boundary.  (Whether the capacity is enough is the library's
    to say: it names the bound.)"""
    import torch
    device = torch.device(device)
    if out is None:
        out = torch.empty(max(int(cap), 0) + 16, dtype=torch.uint8, device=device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or out.stride(0) != 1 or out.device != device:
        raise TypeError(who + "out must be a dense 1-D uint8 CUDA tensor on the canvas's device")
    base = out.data_ptr()
    aligned = (base + 15) & ~15
    return out, aligned - base, aligned, out.numel() - (aligned - base)


class Bitmap:
    """One decoded RGBA8 image resident in HBM and owned by the library (ist_bitmap_*), with what the planner reads of it: width,
    height (natural size), orientation (EXIF 1..8), opaque, file_size.  Made by decode_bitmaps / upload_bitmap; plan, stitch and
    stitch_png take a list of them in place of host images and read the pixels where they are (the page's bitmap cache,
    index.js:534-627).  close() - or garbage collection - drops this reference; a call that is using the bitmap keeps its own until it
    returns.  48 MB of HBM per 12 MP photo, for as long as the host keeps it."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = int(device)
        self._desc = L.ImageDesc()
        L.check(L.lib.ist_bitmap_desc(C.c_void_p(handle), C.byref(self._desc)))

    width = property(lambda self: int(self._desc.width))
    height = property(lambda self: int(self._desc.height))
    orientation = property(lambda self: int(self._desc.orientation))
    opaque = property(lambda self: bool(self._desc.opaque))
    file_size = property(lambda self: int(self._desc.file_size))

    @property
    def shape(self):
        """(rows, columns, 4) of the stored pixels (the decoded bitmap, before any EXIF orientation)"""
        d = self._desc
        return (int(d.bmp_height or d.height), int(d.bmp_width or d.width), 4)

    def handle(self):
        if not self._h:
            raise ValueError("the bitmap has been closed")
        return self._h

    def download(self):
        """the pixels as an HxWx4 uint8 array (one copy from HBM)"""
        out = np.empty(self.shape, np.uint8)
        L.check(L.lib.ist_bitmap_download(C.c_void_p(self.handle()), out.ctypes.data, out.strides[0], out.shape[0]))
        return out

    def preview(self, box_w, box_h):
        """the stored pixels shrunk to fit a box (preview_fit of shape; ist_bitmap_preview): an HxWx4 uint8 thumbnail reduced in HBM,
        without the download.  EXIF orientation is not applied, as in download()."""
        rows, cols, _ = self.shape
        pw, ph = preview_fit(cols, rows, box_w, box_h)
        out = np.empty((ph, pw, 4), np.uint8)
        L.check(L.lib.ist_bitmap_preview(_ctx(self.device), C.c_void_p(self.handle()), pw, ph, out.ctypes.data, out.strides[0]))
        return out

    def rows(self, y0, n):
        """rows [y0, y0 + n) of the stored pixels as a Bitmap of their own (ist_bitmap_rows): a view that shares this bitmap's block and
        keeps it alive, copies nothing, and goes wherever a Bitmap goes.  Refused for EXIF orientation > 1 and reduced-scale decodes."""
        h = L.lib.ist_bitmap_rows(C.c_void_p(self.handle()), int(y0), int(n))
        if not h:
            msg = L.last_error()
            raise L.StitchError(-7 if "orientation" in msg or "reduced scale" in msg else -1, msg)
        return Bitmap(h, self.device)

    def close(self):
        if self._h:
            L.lib.ist_bitmap_release(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __repr__(self):
        return "Bitmap(%dx%d, orientation %d, device %d%s)" % (self.width, self.height, self.orientation, self.device, "" if self._h else ", closed")


def _is_bitmap_request(images, o):
    """True for a request made of Bitmaps (None entries allowed: the library rejects them as a missing image), False for one of host
    images.  A request is one or the other."""
    if not any(isinstance(im, Bitmap) for im in images):
        return False
    if not all(im is None or isinstance(im, Bitmap) for im in images):
        raise TypeError("a request is either all Bitmaps or all host images, not a mix")
    if o.get("devices") is not None:
        raise TypeError("devices= does not apply to Bitmaps: a bitmap lives on one GPU")
    return True


def _bitmap_descs(images):
    arr = (L.ImageDesc * max(1, len(images)))()
    for i, b in enumerate(images):
        if b is not None:
            arr[i] = b._desc
    return arr


def _overlap_call_opts(tolerance, min_rows, min_informative):
    return L.OverlapOpts(int(tolerance), int(min_rows), int(min_informative), 0)


def _overlap_records(out, n):
    return [{"header": int(out[i].header), "footer": int(out[i].footer), "overlap": int(out[i].overlap), "cost": int(out[i].cost)} for i in range(n)]


def find_overlaps(bitmaps, tolerance=8, min_rows=16, min_informative=8):
    """Per neighbouring pair of a vertical strip of Bitmaps (scrolled screenshots, top to bottom): {'header', 'footer', 'overlap', 'cost'} -
    the rows of a bar both shots repeat at the top and at the bottom, the rows of the upper shot's body that the lower one shows again,
    and the summed row difference at that overlap (ist_bitmaps_overlap; the rule is in include/imagestitch.h).  Found on the GPU from
    the resident pixels: three launches per call.  The defaults are the contract's, not measured optima: tolerance 8 is two 8-bit
    levels per pixel.  Periodic content is ambiguous by nature; content that changes inside the overlap may give overlap 0."""
    bitmaps = list(bitmaps)
    if not all(isinstance(b, Bitmap) for b in bitmaps):
        raise TypeError("find_overlaps: expected Bitmaps (upload_bitmap / decode_bitmaps)")
    n = len(bitmaps)
    out = (L.Overlap * max(1, n - 1))()
    opts = _overlap_call_opts(tolerance, min_rows, min_informative)
    handles = (C.c_void_p * max(1, n))(*[b.handle() for b in bitmaps])
    L.check(L.lib.ist_bitmaps_overlap(_ctx(bitmaps[0].device if n else 0), handles, n, C.byref(opts), out))
    return _overlap_records(out, n - 1)


def find_overlaps_device(tensors, tolerance=8, min_rows=16, min_informative=8):
    """find_overlaps for HxWx4 uint8 CUDA tensors (any row pitch, dense pixels) on one device (ist_overlap_device).  The current
    stream is synchronised first: the call reads the tensors on the library's stream and returns the records."""
    import torch
    tensors = list(tensors)
    n = len(tensors)
    if n:
        _check_canvases(tensors, "find_overlaps_device: ")
    descs = (L.ImageDesc * max(1, n))()
    ptrs, pitches = (C.c_void_p * max(1, n))(), (C.c_size_t * max(1, n))()
    for i, t in enumerate(tensors):
        descs[i].width, descs[i].height, descs[i].orientation = int(t.shape[1]), int(t.shape[0]), 1
        ptrs[i], pitches[i] = t.data_ptr(), t.stride(0)
    out = (L.Overlap * max(1, n - 1))()
    opts = _overlap_call_opts(tolerance, min_rows, min_informative)
    dev = (tensors[0].device.index or 0) if n else 0
    if n:
        torch.cuda.current_stream(dev).synchronize()
    L.check(L.lib.ist_overlap_device(_ctx(dev), ptrs, pitches, descs, n, C.byref(opts), out))
    return _overlap_records(out, n - 1)


def overlap_rows(pairs, heights):
    """The crop rule (ist_overlap_rows; pure CPU): [(top, bot)] per image - image i keeps rows [top, bot) - for the records of
    find_overlaps and the images' heights.  A pair with overlap 0 crops nothing; an image that would keep no row voids its pair."""
    n = len(heights)
    if len(pairs) != max(0, n - 1):
        raise ValueError("overlap_rows: %d images need %d pairs, not %d" % (n, max(0, n - 1), len(pairs)))
    cp = (L.Overlap * max(1, n - 1))()
    for i, p in enumerate(pairs):
        cp[i].header, cp[i].footer, cp[i].overlap, cp[i].cost = int(p["header"]), int(p["footer"]), int(p["overlap"]), int(p.get("cost", 0))
    ch = (C.c_int32 * max(1, n))(*[int(h) for h in heights])
    top, bot = (C.c_int32 * max(1, n))(), (C.c_int32 * max(1, n))()
    L.check(L.lib.ist_overlap_rows(cp, ch, n, top, bot))
    return [(int(top[i]), int(bot[i])) for i in range(n)]


def _crop_views(bitmaps, records):
    rows = overlap_rows(records, [b.shape[0] for b in bitmaps])
    views = []
    try:
        for b, (t, e) in zip(bitmaps, rows):
            views.append(b.rows(t, e - t))
    except Exception:
        for v in views:
            v.close()
        raise
    return views


def crop_overlaps(bitmaps, **opts):
    """The strip without what its neighbours share: one row view per Bitmap (Bitmap.rows over overlap_rows of find_overlaps(bitmaps,
    **opts)); nothing is copied, and the views stitch, preview and export like any Bitmap."""
    bitmaps = list(bitmaps)
    return _crop_views(bitmaps, find_overlaps(bitmaps, **opts) if len(bitmaps) > 1 else [])


def _read_files(files):
    blobs = []
    for f in files:
        if isinstance(f, (str, os.PathLike)):
            with open(f, "rb") as fh:
                f = fh.read()
        blobs.append(bytes(f))
    return blobs


def decode_bitmaps(files, device=0, scale=1, profile="ignore"):
    """Image files (bytes, or paths that are read here) -> [Bitmap], decoded straight into HBM by the decoder of stitch_files (baseline
    JPEG: Huffman decoding + reconstruction on the GPU).  Each bitmap's desc is what stitch_files plans with: size, EXIF orientation,
    opaque for JPEG, file_size = the file's length.  All or nothing: a file that does not decode raises StitchError('图片k解码异常: ...')
    and no bitmap is kept.
    scale: 1, 2, 4 or 8, one for all files or one per file: a JPEG is decoded at 1 / scale of its size (scaled_size; libjpeg-turbo's
    decode-to-scale, byte for byte) and held at that size - width / height stay the natural size, shape is the stored one - so a
    12 MP photo at scale 4 holds 3 MB instead of 48 MB and plans, stitches, previews and thumbnails like the full-size bitmap.  Other
    file types decode at 1 / 1.
    profile: 'ignore' (the pixels as decoded) or 'srgb': a file tagged with an ICC profile the colour contract takes (matrix/TRC RGB:
    Display P3, Adobe RGB, ...) is converted to sRGB in place by one launch behind its decode; untagged, sRGB-tagged and unsupported
    files stay as decoded (image_color says which a file is)."""
    ctx = _ctx_color(device, profile)
    blobs = _read_files(files)
    n = len(blobs)
    if n == 0:
        return []
    _, cden = _scales(scale, blobs, "decode_bitmaps")
    cfiles = (C.c_char_p * n)(*blobs)
    lens = (C.c_int64 * n)(*[len(b) for b in blobs])
    out = (C.c_void_p * n)()
    if cden is None:
        L.check(L.lib.ist_bitmaps_decode(ctx, cfiles, lens, n, out))
    else:
        L.check(L.lib.ist_bitmaps_decode_scaled(ctx, cfiles, lens, n, cden, out))
    return [Bitmap(out[i], device) for i in range(n)]


def _join_args(files, direction, who):
    if direction not in _DIRECTIONS:
        raise ValueError("%s: direction must be 'vertical' or 'horizontal'" % who)
    blobs = _read_files(files)
    n = len(blobs)
    if n == 0:
        raise ValueError("%s: no files" % who)
    return blobs, (C.c_char_p * n)(*blobs), (C.c_int64 * n)(*[len(b) for b in blobs]), n


def _join_record(info):
    return {"ok": info.reason == 0, "reason": L.JOIN_REASONS[info.reason], "image": int(info.image), "width": int(info.width),
            "height": int(info.height), "subsampling": {0: "444", 1: "420"}.get(info.subsampling)}


def jpeg_join_check(files, direction):
    """Can these JPEG files (bytes, or paths that are read here) be joined losslessly (ist_jpeg_join_check: headers only, no GPU)?
    Returns {'ok', 'reason', 'image', 'width', 'height', 'subsampling'}: reason is 'ok' or the lower-case name of the first refusal
    ('not_jpeg', 'layout', 'mixed', 'tables', 'size', 'align', 'orient', 'limit'), image the first image it applies to (-1: none),
    width / height the joined file's size when ok (else 0), subsampling '444' / '420' of image 0 once known (else None).  The
    library's message of a refusal is last_error()."""
    _, cfiles, lens, n = _join_args(files, direction, "jpeg_join_check")
    info = L.JpegJoinInfo()
    rc = L.lib.ist_jpeg_join_check(cfiles, lens, n, _DIRECTIONS[direction], C.byref(info))
    if rc < 0 and rc != -7:      # (IST_E_UNSUPPORTED is the refusal the record describes)
        L.check(rc)
    return _join_record(info)


def join_jpeg(files, direction, optimize=False, device=0):
    """JPEG files (bytes or paths, as decode_bitmaps takes them) -> ONE JPEG file (bytes) that carries exactly the sources' quantised
    coefficients and quantisation tables (ist_jpeg_join_files): what jpegtran does for one file, done for a strip.  No pixel is made:
    the files are entropy-decoded to their coefficient planes on the GPU, one kernel moves the blocks into the export's scratch, and
    the export's entropy coder writes the file - no generation loss, no quality to choose.  The sources must share a width
    (vertical) or height (horizontal), a sampling layout (4:4:4 or 4:2:0) and their quantisation tables; every image but the last
    must be a whole number of MCUs along the join (jpeg_join_check says whether a set qualifies, and why not).  optimize=True: the
    file's own Huffman tables (IST_JPEG_OPTIMIZE).  An ineligible set raises StitchError (IST_E_UNSUPPORTED) whose message names the
    image and the reason; nothing falls back to the pixel route - the caller asks jpeg_join_check and decides."""
    if not isinstance(optimize, bool):
        raise TypeError("optimize: expected a bool")
    _, cfiles, lens, n = _join_args(files, direction, "join_jpeg")
    out, m = C.POINTER(C.c_uint8)(), C.c_int64(0)
    L.check(L.lib.ist_jpeg_join_files(_ctx(device), cfiles, lens, n, _DIRECTIONS[direction], JPEG_OPTIMIZE if optimize else 0, None,
                                      C.byref(out), C.byref(m)))
    return _take_png(out, m)


def thumbnails_from_files(files, cell, mode="fill", orient=True, device=0, profile="ignore"):
    """Image files (bytes or paths) -> their thumbnails for a cell (width, height), as thumbnails() returns them, without ever holding
    a full-size bitmap: every JPEG is decoded at the largest scale (decode_scale_fit) at which its stored pixels still cover its
    thumbnail, so the grid of nine 12 MP photos (index.wxml:4-22) reads a sixty-fourth of their pixels.  The bitmaps are released
    before the call returns.  profile: as decode_bitmaps."""
    _color_profile(profile)
    blobs = _read_files(files)
    if not blobs:
        return []
    infos = [image_info(b) for b in blobs]
    items = thumbnail_layout([(w, h, o or 1) for (w, h, o) in infos], cell, mode, orient)
    scales = []
    for (w, h, o), t in zip(infos, items):
        tw, th = (t["height"], t["width"]) if orient and o >= 5 else (t["width"], t["height"])      # the thumbnail on the STORED axes
        scales.append(decode_scale_fit(w, h, max(1, tw), max(1, th)))
    bitmaps = decode_bitmaps(blobs, device, scale=scales, profile=profile)
    try:
        return thumbnails(bitmaps, cell, mode, orient)
    finally:
        for b in bitmaps:
            b.close()


def image_color(data):
    """The colour kind of an image file (ist_image_color): 'none' (untagged), 'identity' (tagged sRGB: nothing to do), 'convert' (a
    profile that profile='srgb' converts) or 'unsupported' (a profile the contract does not take: LUT-only, GRAY, CMYK, damaged).
    Pure CPU."""
    buf = bytes(data)
    kind = C.c_int32(0)
    L.check(L.lib.ist_image_color(buf, len(buf), C.byref(kind)))
    return COLOR_KINDS[kind.value]


def _icc_tables(icc):
    buf = bytes(icc)
    t = L.ColorTables()
    L.check(L.lib.ist_icc_tables(buf, len(buf), C.byref(t)))
    return t


def icc_tables(icc):
    """The integer tables of an ICC profile (ist_icc_tables): {'kind', 'dec': 3x256 uint16, 'mq': 3x3 int32}; dec and mq are None
    for 'unsupported'.  Pure CPU."""
    t = _icc_tables(icc)
    kind = COLOR_KINDS[t.kind]
    if kind not in ("convert", "identity"):
        return {"kind": kind, "dec": None, "mq": None}
    return {"kind": kind, "dec": np.ctypeslib.as_array(t.dec).astype(np.uint16), "mq": np.ctypeslib.as_array(t.mq).astype(np.int32)}


def convert_color_device(tensor, icc, stream=None):
    """An HxWx4 uint8 CUDA tensor (any row stride that is a multiple of 4 bytes, pixels contiguous) through the tables of the ICC
    profile `icc` to sRGB, in place (ist_color_convert_device), asynchronous on `stream` (None: the current torch stream).  Identity
    tables change nothing; a profile the contract does not take raises StitchError(IST_E_INVALID).  Returns the tensor."""
    import torch
    t = tensor
    _check_canvas(t, "convert_color_device: ")
    tables = _icc_tables(icc)
    s = torch.cuda.current_stream(t.device).cuda_stream if stream is None else int(stream)
    L.check(L.lib.ist_color_convert_device(_ctx(t.device.index), t.data_ptr(), t.stride(0), t.shape[1], t.shape[0], C.byref(tables), s))
    return tensor


def upload_bitmap(image, device=0):
    """A host image -> Bitmap: an HxWx4 uint8 RGBA array, or a dict as stitch() takes ({'width', 'height', 'data', 'orientation'?,
    'fileSize'?, 'opaque'?}); the desc is kept as given."""
    a = image.get("data") if isinstance(image, dict) else image
    if a is None:
        raise L.StitchError(-6, "图片0解码异常")
    a = _rgba(a)
    desc = _descs([image])
    a, ptr, pitch = _host_rows(a, desc[0])
    h = L.lib.ist_bitmap_upload(_ctx(device), desc, ptr, pitch)
    if not h:                                    # (NULL: the message says which rule failed)
        msg = L.last_error()
        raise L.StitchError(-6 if msg.startswith("图片") else -1 if msg.startswith("src_pitch") else -8 if msg.startswith("out of device memory") else -9, msg)
    return Bitmap(h, device)


class StitchJob:
    """A compiled op list on one device: re-launchable on new source / destination buffers with no upload."""

    def __init__(self, ctx, handle, n_images, device=0):
        self._ctx, self._h, self.n_images, self._device = ctx, handle, n_images, int(device)
        info = L.JobInfo()
        L.check(L.lib.ist_job_info_get(handle, C.byref(info)))
        self.info = {k: getattr(info, k) for k, _ in L.JobInfo._fields_}
        self.canvas_w, self.canvas_h = int(info.canvas_w), int(info.canvas_h)
        self._src = (C.c_void_p * max(1, n_images))()
        self._pitch = (C.c_size_t * max(1, n_images))()

    @property
    def preferred_pitch(self):
        """bytes per canvas row this job runs fastest on (ist_job_preferred_dst_pitch): dense rows for a strip the library walks in its
        flat form, otherwise rows padded to a multiple of 4 KiB"""
        return int(L.lib.ist_job_preferred_dst_pitch(self._h))

    def empty_canvas(self, device=None):
        """an uninitialised canvas tensor (canvas_h x canvas_w x 4, uint8) on the job's device whose row pitch is preferred_pitch"""
        import torch
        dev = torch.device("cuda", self._device if device is None else device)
        pitch = self.preferred_pitch
        raw = torch.empty((self.canvas_h * pitch + 4096,), dtype=torch.uint8, device=dev)
        off = (-raw.data_ptr()) % 4096
        return raw[off:off + self.canvas_h * pitch].view(self.canvas_h, pitch // 4, 4)[:, :self.canvas_w]

    def launch_ptrs(self, src_ptrs, src_pitches, dst_ptr, dst_pitch, stream=0):
        for i, (p, q) in enumerate(zip(src_ptrs, src_pitches)):
            self._src[i] = p
            self._pitch[i] = q
        L.check(L.lib.ist_job_launch(self._h, self._src, self._pitch, self.n_images, C.c_void_p(dst_ptr), dst_pitch,
                                     C.c_void_p(stream)))

    def launch(self, srcs, out, stream=None):
        """srcs: list of HxWx4 uint8 CUDA tensors (None for images the job does not sample); out: canvas tensor."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(out.device)
        ptrs = [0 if t is None else t.data_ptr() for t in srcs]
        pitches = [0 if t is None else t.stride(0) for t in srcs]
        self.launch_ptrs(ptrs, pitches, out.data_ptr(), out.stride(0), st.cuda_stream)

    def close(self):
        if self._h:
            L.lib.ist_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_cells(canvas_w, canvas_h, ops, n_ops, descs, n_images, filter="bilinear", clear=(0, 0, 0, 0), clip=None):
    """The cells Stitcher.compile_ops would compile for the same arguments (ist_debug_cells: pure CPU, no device): returns
    (cells, kernel_kind, tile_table) with one dict per cell - path (_lib.PATH_*), tile_w, tile_h, sub_h, X0, Y0, X1, Y1, tiles."""
    clr = (C.c_uint8 * 4)(*clear)
    region = C.byref(L.Region(*[int(v) for v in clip])) if clip is not None else None
    f = _FILTERS[filter] if isinstance(filter, str) else int(filter)
    n, kind, table = C.c_int(0), C.c_int(0), C.c_int(0)
    L.check(L.lib.ist_debug_cells(int(canvas_w), int(canvas_h), clr, ops, int(n_ops), descs, int(n_images), f, region, None, 0, C.byref(n), None, None))
    arr = (L.DebugCell * max(1, n.value))()
    L.check(L.lib.ist_debug_cells(int(canvas_w), int(canvas_h), clr, ops, int(n_ops), descs, int(n_images), f, region, arr, n.value, C.byref(n),
                                  C.byref(kind), C.byref(table)))
    return [{k: getattr(arr[i], k) for k, _ in L.DebugCell._fields_} for i in range(n.value)], kind.value, bool(table.value)


class Stitcher:
    """Device-resident stitcher: one per GPU (one process per GPU in the multi-GPU layout)."""

    def __init__(self, device=0):
        self.device = int(device)
        self._ctx = _ctx(self.device)

    def compile_ops(self, canvas_w, canvas_h, ops, n_ops, descs, n_images, filter="bilinear", clear=(0, 0, 0, 0), clip=None):
        clr = (C.c_uint8 * 4)(*clear)
        region = None
        if clip is not None:
            region = C.byref(L.Region(*[int(v) for v in clip]))
        h = L.lib.ist_job_create(self._ctx, int(canvas_w), int(canvas_h), clr, ops, int(n_ops), descs, int(n_images),
                                 _FILTERS[filter] if isinstance(filter, str) else int(filter), region)
        if not h:
            raise L.StitchError(-1, L.last_error())
        return StitchJob(self._ctx, h, n_images, self.device)

    def compile(self, images, direction, opts=None, only_images=None):
        """Plan + compile.  only_images: iterable of image indices this device renders (multi-GPU sharding);
        the other rects are dropped from the op list (their canvas area is left to whoever owns them)."""
        o = _merge(opts)
        p = plan(images, direction, o)
        if p is None:
            return None, None
        ops, n_ops = p.ops()
        if only_images is not None:
            keep = set(int(i) for i in only_images)
            sel = [ops[0]] + [ops[k] for k in range(1, n_ops) if ops[k].image in keep]
            ops = (L.Op * len(sel))(*sel)
            n_ops = len(sel)
        job = self.compile_ops(p.canvas_w, p.canvas_h, ops, n_ops, p._descs, len(images), _filter_of(o))
        return p, job


class GroupJob:
    """A stitch compiled for a device group (ist_group_job_*): parts[k] = {image, slot, device, box, rows} and one source
    pointer per part at launch."""

    def __init__(self, group, handle, plan):
        self._g, self._h, self.plan = group, handle, plan
        n = C.c_int(0)
        L.check(L.lib.ist_group_job_parts(handle, None, 0, C.byref(n)))
        arr = (L.Part * max(1, n.value))()
        L.check(L.lib.ist_group_job_parts(handle, arr, n.value, C.byref(n)))
        self.parts = [{"image": p.image, "slot": p.slot, "device": group.devices[p.slot], "box": (p.X0, p.Y0, p.X1, p.Y1),
                       "rows": (p.sy0, p.sy1), "in_place": bool(p.in_place)} for p in arr[:n.value]]

    def launch(self, part_srcs, out):
        """part_srcs[k]: HxWx4 uint8 CUDA tensor on parts[k]['device'] holding the WHOLE image, or (tensor, first_row) for a
        partial holding (rows first_row ... ; one spare row behind the last must be readable).  out: canvas on the root.
        The group's streams do not synchronise with the caller's: work the caller queued on these buffers (uploads, fills) is
        waited for here, on each tensor's current torch stream."""
        import torch
        for dev in {(s[0] if isinstance(s, tuple) else s).device for s in part_srcs} | {out.device}:
            torch.cuda.current_stream(dev).synchronize()
        n = len(self.parts)
        ptrs, pitches = (C.c_void_p * n)(), (C.c_size_t * n)()
        for k, s in enumerate(part_srcs):
            t, first = (s if isinstance(s, tuple) else (s, 0))
            ptrs[k] = t.data_ptr() - first * t.stride(0)
            pitches[k] = t.stride(0)
        L.check(L.lib.ist_group_job_launch(self._h, ptrs, pitches, n, C.c_void_p(out.data_ptr()), out.stride(0)))

    def close(self):
        if self._h:
            L.lib.ist_group_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StitchGroup:
    """Several GPUs driven from this one process (the N-API host's layout; ist_group_*).  devices[0] is the root."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * len(self.devices))(*self.devices)
        self._h = L.lib.ist_group_create(arr, len(self.devices))
        if not self._h:
            raise L.StitchError(-5, L.last_error())

    def compile(self, images, direction, opts=None):
        o = _merge(opts)
        p = plan(images, direction, o)
        if p is None:
            return None
        ops, n_ops = p.ops()
        clr = (C.c_uint8 * 4)(0, 0, 0, 0)
        h = L.lib.ist_group_job_create(self._h, p.canvas_w, p.canvas_h, clr, ops, n_ops, p._descs, len(images), _filter_of(o), _SPLITS[o["split"]])
        if not h:
            raise L.StitchError(-1, L.last_error())
        return GroupJob(self, h, p)

    def sync(self):
        L.check(L.lib.ist_group_sync(self._h))

    def close(self):
        if self._h:
            L.lib.ist_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
