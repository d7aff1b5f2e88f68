/*
 * imagestitch.h — C-ABI of the MI355X-native strip stitcher (libimagestitch.so).
 *
 * This is the drop-in boundary for ONE path of Iamctb/ImageStitching: the Canvas-2D strip concatenation in
 * Page.onStitch (plan -> per-image resample -> row/column blit into one buffer -> readback).  The reference has
 * no FFI of its own (it is a WeChat mini-program: JavaScript calling the platform Canvas); the seam is the set
 * of Canvas calls onStitch issues.  Every entry point below names the reference code it replaces; paths are
 * relative to miniprogram-stitch/miniprogram/ in the reference repository.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures (a stream is passed as void* = hipStream_t);
 *   - return 0 on success, a negative IST_E_* code on failure; ist_last_error() gives the thread-local message
 *     (the reference throws Error(msg) into one catch that toasts '拼图失败：'+msg, pages/index/index.js:1618-1624);
 *   - the caller owns every pixel buffer; the library owns only what it returns through ist_*_create /
 *     ist_plan_compute and frees through the matching destroy/free call;
 *   - pixels are RGBA8, row-major, straight (non-premultiplied) alpha, top row first, as ImageData is;
 *   - no CPU fallback exists: rendering entry points fail with IST_E_NO_DEVICE when no HIP device is present.
 */
#ifndef IMAGESTITCH_H_
#define IMAGESTITCH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IST_API __attribute__((visibility("default")))

#define IST_ABI_VERSION 2     /* 2: output capacity on the decode calls, pooled pinned results, device groups */

/* error codes */
enum {
  IST_OK = 0,
  IST_NOTHING_TO_DO = 1,        /* onStitch returns early when images is empty (pages/index/index.js:1189) */
  IST_E_INVALID = -1,           /* bad argument */
  IST_E_SIZE_UNAVAILABLE = -2,  /* '图片尺寸不可用'   (pages/index/index.js:1254) */
  IST_E_OUTPUT_SIZE = -3,       /* '输出尺寸计算失败' (pages/index/index.js:1320) */
  IST_E_NO_CONTEXT = -4,        /* '无法获取绘图上下文' (pages/index/index.js:1412) */
  IST_E_NO_DEVICE = -5,         /* 'OffscreenCanvas 不可用' analogue (utils/canvas.js:149): no HIP device / HIP failure */
  IST_E_DECODE = -6,            /* '图片N解码异常' (pages/index/index.js:1513): a source bitmap is missing or 0-sized */
  IST_E_UNSUPPORTED = -7,       /* a Canvas feature outside the path (non axis-aligned transform, translucent fill) */
  IST_E_NOMEM = -8,
  IST_E_HIP = -9
};

enum { IST_VERTICAL = 0, IST_HORIZONTAL = 1 };                    /* data.direction  (index.js:16)    */
enum { IST_MODE_MIN = 0, IST_MODE_MAX = 1, IST_MODE_ORIGINAL = 2 };/* data.*StitchMode (index.js:19-20) */
enum { IST_PLATFORM_OTHER = 0, IST_PLATFORM_IOS = 1, IST_PLATFORM_ANDROID = 2 }; /* sys.platform       */
enum { IST_OP_FILL = 0, IST_OP_DRAW = 1, IST_OP_HOLE = 2 };
enum { IST_FILTER_NEAREST = 0, IST_FILTER_BILINEAR = 1, IST_FILTER_AREA = 2, IST_FILTER_CUBIC = 3 };   /* imageSmoothingEnabled false / true (index.js:1416-1418) */
/* IST_FILTER_AREA (an option; the contract's default for imageSmoothingQuality = 'high', index.js:1419, stays bilinear): on
 * every source axis that is MINIFIED (|scale| > 1 source pixel per canvas pixel) the sample is the average of the source
 * over the canvas pixel's footprint (a box of that width, pixels weighted by overlap); other axes, and any draw that
 * does not shrink, are bilinear - at |scale| = 1 the box IS the bilinear pair, so the two meet continuously.  The
 * phone-capped plans shrink 12 MP photos 2.2x (iOS) to 6.6x (Android), where point-sampled bilinear aliases. */
/* IST_FILTER_CUBIC (an option, the counterpart of IST_FILTER_AREA for draws that GROW: the super-sampled small-job plan,
 * index.js:1363, enlarges 2.2-2.6x; mode 'max' enlarges every image narrower than the widest): decided per source axis of a
 * draw.  On an axis with |scale| <= 1 (enlarged or 1:1) the sample is the Catmull-Rom cubic convolution (Keys, a = -0.5) at
 * half-pixel centres: f = s - 0.5, i = floor(f), t = f - i, taps i-1 .. i+2, each clamped to the draw's clamp box, weights
 *     w(-1) = ((-0.5 t + 1.0) t - 0.5) t      w(0) = (1.5 t - 2.5) t t + 1.0
 *     w(+1) = ((-1.5 t + 2.0) t + 0.5) t      w(+2) = (0.5 t - 0.5) t t
 * (they sum to 1; at t = 0 they are (0, 1, 0, 0), so a 1:1 draw at an integer offset is the identity and stays a copy).  On an
 * axis with |scale| > 1 the sample is the box of IST_FILTER_AREA, unchanged.  The separable sum runs over premultiplied,
 * unrounded components; the kernel's negative lobes overshoot, so alpha is clamped to [0, 255] and each premultiplied colour
 * to [0, alpha] before compositing.  Coverage, source-over and the single rounding are those of the bilinear filter. */
/* OR-ed into a `filter` argument: anti-alias FRACTIONAL rectangle edges by area coverage, as Canvas rasters do (they
 * arise from ctx.scale(superSample), index.js:1426-1428, and from the unrounded cursor, :1432).  Off: a pixel belongs
 * to a draw iff its centre is inside the rectangle.  Integer-edged plans are unaffected either way. */
enum { IST_FILTER_EDGE_AA = 0x100 };

/* per-image record: the five fields the planner reads (index.js:724-739, 1194, 1211, 1252-1253, 1522-1523, 1532) */
typedef struct ist_image_desc {
  int32_t width, height;      /* naturalWidth, naturalHeight */
  int32_t orientation;        /* EXIF 1..8; 0 = unset (treated as 1, utils/canvas.js:155) */
  int32_t bmp_width, bmp_height; /* decoded bitmap size (bmp.width/height); 0 = same as natural */
  int32_t opaque;             /* caller's hint: every alpha byte is 255 (JPEG-decoded photos). Never changes results. */
  int64_t file_size;          /* bytes; feeds bigTask (index.js:1211-1212); 0 if unknown */
} ist_image_desc;

/* device caps: this.deviceMaxCanvasSize / deviceMaxCanvasPixels + sys.platform (index.js:126-156, 1323-1336) */
typedef struct ist_limits {
  int32_t platform;
  int32_t reserved;
  double max_side;            /* 0 = unset -> reference fallback (android 4096, else 12288) */
  double max_pixels;          /* 0 = unset -> reference fallback */
  double max_super_sample;    /* <=0: reference rule (bigTask 1, ios 2.2, else 2.6; index.js:1363); >0 replaces it */
} ist_limits;

/* one drawWithOrientation call (utils/canvas.js:153): destination rectangle in user space */
typedef struct ist_rect {
  int32_t image, orientation;
  double dx, dy, dw, dh;
} ist_rect;

/* result of the planner: index.js stage 2 (1251-1386) + the rect/cursor loop (1432-1433, 1522-1554) */
typedef struct ist_plan {
  double out_w, out_h;        /* targetW/H after caps (1360-1361) */
  double scale_down;          /* 1337-1357 */
  double super_sample;        /* 1360-1386 */
  int64_t canvas_w, canvas_h; /* canvasOutW/H: offscreen canvas + export size (1373-1383, 1391, 1577-1579) */
  int32_t big_task;           /* 1212 */
  int32_t n_rects;
  ist_rect* rects;            /* library-owned; ist_plan_free */
} ist_plan;

/* One recorded Canvas call, in canvas order.  kind 0: fillRect(d) with fillStyle rgba (index.js:1423-1424);
 * kind 1: 9-argument drawImage(image, s, d) (utils/canvas.js:156); kind 2 (no Canvas analogue): rectangle d is
 * left untouched by the launch because another producer delivers those pixels (a band received in place over
 * xGMI in the multi-GPU layout).  m = CTM at the time of the call:
 * X = m0*u + m2*v + m4,  Y = m1*u + m3*v + m5  (same order as ctx.setTransform(a,b,c,d,e,f), index.js:1404). */
typedef struct ist_op {
  int32_t kind, image;
  double m[6];
  double s[4];                /* sx, sy, sw, sh */
  double d[4];                /* dx, dy, dw, dh */
  uint8_t rgba[4];
  int32_t reserved;
} ist_op;

typedef struct ist_region { int32_t x, y, w, h; } ist_region;    /* getImageData / export region (index.js:1564, 1577) */

typedef struct ist_job_info {
  int64_t canvas_w, canvas_h;
  int32_t n_ops, n_cells;
  int64_t n_tiles;
  int64_t out_pixels;         /* pixels written per launch */
  int64_t src_pixels_touched; /* distinct source pixels inside the sampling footprints */
  int64_t algorithmic_bytes;  /* 4*src_pixels_touched + 4*out_pixels */
  int64_t tiles_fill, tiles_copy, tiles_sample, tiles_general;
} ist_job_info;

typedef struct ist_ctx ist_ctx;   /* one HIP device + scratch */
typedef struct ist_job ist_job;   /* one compiled op list (device-side cell/op tables) */

/* ---- diagnostics ------------------------------------------------------------------------------------------ */
IST_API int ist_abi_version(void);
IST_API const char* ist_last_error(void);
IST_API int ist_device_count(void);                                   /* 0 when no HIP device is usable */
/* device allocations (hipMalloc calls) the library has made in this process so far.  A measurement aid for hosts and tests:
 * the steady state of every entry point allocates nothing (scratch, arenas and table blocks are kept and re-used). */
IST_API int64_t ist_debug_device_allocs(void);
/* What the library has asked the HIP runtime for in this process and not yet given back: out[0] device blocks, out[1] pinned host
 * blocks (the pool of result buffers that ist_free / ist_pool_trim manage is not counted), out[2] streams, out[3] events.  A test aid:
 * the steady state of every entry point leaves all four where they were, and destroying a context (group, bitmap, job) returns
 * everything it made.  IST_E_INVALID when out is NULL; four zeros in a process that has not used a device. */
IST_API int ist_debug_live_handles(int64_t out[4]);
/* JPEG files whose entropy-coded scan the GPU Huffman decoder has decoded AND validated in this process so far (files it
 * handed back to the host decoder do not count).  Tests use it to tell the GPU path from the silent host fall-back. */
IST_API int64_t ist_debug_gpu_entropy_files(void);
/* synchronisation launches the GPU Huffman decoder has made in this process so far, summed over its calls (one call decodes a whole
 * batch of files: its launches are those of the file that settles last).  Two per call is the floor; a file whose MCU slots all share
 * both Huffman tables takes about one per 48 subsequences of 1024 bits, 64 at the most. */
IST_API int64_t ist_debug_gpu_entropy_sync_launches(void);
/* The GPU Huffman decoder's coefficients of ONE file, read back (a test aid: pixels cannot tell a wrong coefficient that the IDCT's
 * clamp hides).  The file is parsed and decoded alone, exactly as the file pipeline would, and the dense planes the reconstruction
 * kernels read - blocks_y * blocks_x * 64 int16 per component, natural order, DC integrated, not dequantised - are copied to
 * planes[c] (plane_elems[c] = the int16 each can hold).  info: ok = 1 when the decoder validated the file (0: it would be handed to
 * the host decoder; the planes are left untouched), launches = its synchronisation launches, and the plane geometry.  planes = NULL
 * fills the geometry only and needs neither a context nor a device.  IST_E_UNSUPPORTED: not a file the GPU decoder takes
 * (progressive, several scans, more than two tables of a class, too many restart intervals). */
typedef struct ist_jpeg_coef_info {
  int32_t ok, launches, ncomp, reserved;
  int32_t blocks_x[3], blocks_y[3];
} ist_jpeg_coef_info;
IST_API int ist_debug_jpeg_gpu_coefficients(ist_ctx* ctx, const uint8_t* file, int64_t len, int16_t* const* planes, const int64_t* plane_elems,
                                            ist_jpeg_coef_info* info);
/* images the file pipeline has reconstructed STRAIGHT INTO the canvas so far (a draw that only moves an opaque image: no bitmap of
 * its own, no stitch launch for it).  Tests use it to tell that path from the general one, which makes the same pixels. */
IST_API int64_t ist_debug_direct_images(void);
/* diagnostics: ist_group_stitch_rgba8 / ist_stitch_rgba8_multi calls of this process whose result was delivered by the HOST
 * SINK (every device DMAs its bands into the pinned result; no gather, no root readback) */
IST_API int64_t ist_debug_host_sink_stitches(void);
/* launches (ist_job_launch, any caller; every entry of an ist_jobs_launch batch counts as one) that took a job's flat form: every op covers whole canvas rows at unit scale and the caller's
 * rows were dense on both sides, so the same bytes were moved as rows of 32 KiB */
IST_API int64_t ist_debug_flat_launches(void);
/* ist_stitch_rgba8 calls delivered band by band with uploads and downloads overlapped (a strip of disjoint row bands >= 32 MB; DESIGN.md
 * section 4 "Host <-> device"); the others took upload-all, launch, download-all */
IST_API int64_t ist_debug_duplex_stitches(void);
/* kernel launches made by ist_jobs_launch (and so by ist_stitch_rgba8_batch) in this process: one per kernel form present in a batch */
IST_API int64_t ist_debug_batch_launches(void);

/* ---- planner: pure CPU, bit-exact to index.js:1211-1216, 1251-1386, 1432-1433, 1522-1554 -------------------- */
IST_API void ist_limits_default(int platform, ist_limits* out);        /* index.js:126-156 fallback branch */
IST_API void ist_limits_unlimited(ist_limits* out);                    /* MI355X default: caps lifted, superSample 1 */
IST_API int ist_plan_compute(const ist_image_desc* images, int n_images, int direction, int mode, double gap,
                             const ist_limits* limits, ist_plan* out);
IST_API void ist_plan_free(ist_plan* plan);
/* the Canvas call sequence stage 3-4 issues for a plan: white fillRect over the canvas (index.js:1423-1424),
 * ctx.scale(ss,ss) folded into every CTM (1426-1428), one drawWithOrientation per rect (utils/canvas.js:153-202).
 * ops must hold n_rects + 1 entries. */
IST_API int ist_plan_ops(const ist_plan* plan, const ist_image_desc* images, int n_images, ist_op* ops, int* n_ops);
/* canvas pixels one op touches: box = {X0, Y0, X1, Y1} (half open, clipped to the canvas) under the coverage rule of
 * `filter` (pixel centre, or every touched pixel with IST_FILTER_EDGE_AA).  Returns 1 when the op draws nothing.
 * Pure CPU; what the multi-GPU layer uses to cut a stitch into per-image bands. */
IST_API int ist_op_box(const ist_op* op, int64_t canvas_w, int64_t canvas_h, int filter, int32_t box[4]);
/* The flat form of an op list as the kernel will walk it (pure CPU, no GPU needed; a test aid): when every op covers whole canvas
 * rows at unit scale, ist_job_launch on dense rows moves the same bytes as rows of *pitch bytes starting *dst_offset bytes into the
 * destination.  One record per cell: rows Y0..Y1-1, pixels X0..X1-1 of that wide canvas; path 0 = fill with bg (packed R,G,B,A),
 * 1 = copy from src[image] starting src_offset bytes into it (+ *pitch per row), source-over bg unless opaque.  *n_cells = 0 when
 * the op list has no flat form.  tests/test_flat_form.py replays the records in numpy against the op list. */
typedef struct ist_flat_cell {
  int32_t path, image;
  int32_t X0, Y0, X1, Y1;
  int64_t src_offset;
  uint32_t bg;
  int32_t opaque;
} ist_flat_cell;
IST_API int ist_debug_flat_form(int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
                                const ist_image_desc* images, int n_images, int filter, const ist_region* clip, int64_t* pitch,
                                int64_t* dst_offset, ist_flat_cell* cells, int max_cells, int* n_cells);
/* The tile path of a compiled cell: ist_flat_cell.path and ist_debug_cell.path.  Which one a cell gets depends on its paint stack, on the
 * filter and on the draw's scales (|kx|, |ky|: source pixels per canvas pixel) alone - never on the pixels.
 *   0 FILL           a constant colour
 *   1 COPY           one 1:1 draw at an integer offset over an opaque colour (or an opaque draw): rows are moved, flips included
 *   2 SAMPLE         one axis-aligned draw, gathered tap by tap straight from HBM (nearest; bilinear where no staged form fits)
 *   3 GENERAL        anything else: the paint stack evaluated per pixel (overlaps, fractional edge strips, strong quarter-turned shrinks)
 *   4 SAMPLE_LDS     SAMPLE, bilinear, |kx| <= 4 and |ky| < 2: a stage of sub_h rows' footprint in LDS, tile_h / sub_h stages per tile
 *   5 SWAP_LDS       one quarter-turned bilinear draw: the footprint staged transposed in LDS; tiles 64 wide and 64 / 32 / 16 high
 *   6 SAMPLE_STREAM  SAMPLE, bilinear, |ky| >= 2: every wave streams its rows' source row pairs through a ring of sub_h pairs
 *   7 AREA_STREAM    one axis-aligned shrinking draw under IST_FILTER_AREA: streamed box sums
 *   8 CUBIC_STREAM   one axis-aligned draw that shrinks on neither axis under IST_FILTER_CUBIC */
enum { IST_PATH_FILL = 0, IST_PATH_COPY = 1, IST_PATH_SAMPLE = 2, IST_PATH_GENERAL = 3, IST_PATH_SAMPLE_LDS = 4, IST_PATH_SWAP_LDS = 5,
       IST_PATH_SAMPLE_STREAM = 6, IST_PATH_AREA_STREAM = 7, IST_PATH_CUBIC_STREAM = 8 };
/* The cells of an op list as ist_job_create compiles them (pure CPU: no context, no device; a test aid).  One record per cell, in
 * canvas order: its path (above), the tile shape the kernel walks it in (tile_w x tile_h canvas pixels; sub_h = rows per LDS stage
 * on path 4, ring depth on path 6, else 0), its canvas box (half open) and its number of tiles.  *kernel_kind (optional) = the kernel
 * form the job launches (0: fill / copy only; 1: + the axis-aligned resampling paths; 2: + SWAP_LDS / GENERAL; 3-4: with AREA_STREAM;
 * 5-6: with CUBIC_STREAM); *tile_table (optional) = 1 when the job carries a per-tile table, 0 when the kernel finds a tile's cell by
 * searching the band and cell prefixes (fill / copy jobs, jobs of more than 4 Mi tiles).  max_cells = 0 only counts. */
typedef struct ist_debug_cell {
  int32_t path;
  int32_t tile_w, tile_h, sub_h;
  int32_t X0, Y0, X1, Y1;
  int64_t tiles;
} ist_debug_cell;
IST_API int ist_debug_cells(int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4], const ist_op* ops, int n_ops,
                            const ist_image_desc* images, int n_images, int filter, const ist_region* clip, ist_debug_cell* cells,
                            int max_cells, int* n_cells, int* kernel_kind, int* tile_table);

/* ---- sharding: one stitch cut into parts for a group of GPUs (pure CPU) ----------------------------------------- */
/* The per-image iterations of onStitch are independent once the cursor is planned (index.js:1439-1554).  A PART is a
 * canvas box of ONE draw, rendered by one GPU (its slot) over the background alone; the root (slot 0) assembles them.
 * IST_SPLIT_IMAGE: image i -> slot i mod n_slots (BASELINE configs[3]).  IST_SPLIT_BAND: canvas rows dealt in canvas
 * order so that every slot renders the same number of output pixels (9 images on 8 GPUs: 1.125 images each); cuts fall
 * on multiples of 8 rows inside a draw's box.  A slot needs only source rows [sy0, sy1) of the part's image (readable
 * for 16 bytes past the last row when a partial buffer is passed, biased by -sy0 rows, to ist_job_launch).
 * Draws that overlap (edge anti-aliasing makes neighbours share a pixel row) cannot be sharded draw by draw: IST_E_UNSUPPORTED.
 * IST_SPLIT_ROWS: slot s owns canvas rows [cuts[s], cuts[s+1]) (ist_shard_row_cuts) ACROSS ALL DRAWS and renders the whole op
 * list clipped to them.  The unit that is rendered and delivered is the slot's BAND - full canvas width whatever the layout,
 * so it is a contiguous byte range of the canvas for horizontal strips (index.js:1540-1553: every rect spans the canvas
 * height, i.e. is a column band under the two cuts above) and centred 'original' rects too: received in place, no staging,
 * no placement launch, host sink always available; overlapping draws and anti-aliased seams are allowed (one owner per
 * pixel paints the whole stack).  Its parts are (slot's rows) x (one draw's box), slot by slot in op order, and say which
 * rows of which image the slot must hold (a horizontal strip on 8 slots: 1/8 of the rows of EVERY image per slot - still
 * disjoint input subsets); in_place is 1 for all of them (it describes the band).
 * IST_SPLIT_AUTO: IMAGE when that cut yields full-width parts only (vertical min / max strips: BASELINE configs[3]),
 * otherwise ROWS; ist_shard_resolve says which. */
enum { IST_SPLIT_IMAGE = 0, IST_SPLIT_BAND = 1, IST_SPLIT_ROWS = 2, IST_SPLIT_AUTO = 3 };
typedef struct ist_part {
  int32_t image, op;          /* source image; index of the draw in the op list */
  int32_t slot;               /* owner, 0 .. n_slots-1; slot 0 is the root */
  int32_t X0, Y0, X1, Y1;     /* canvas box, half open */
  int32_t sx0, sy0, sx1, sy1; /* source columns / rows the part samples, half open */
  int32_t in_place;           /* the box spans the canvas width: a contiguous byte range of the canvas */
} ist_part;
/* max_parts: n_ops + n_slots + 8 suffices for IMAGE / BAND, n_ops * n_slots for ROWS / AUTO */
IST_API int ist_shard_parts(const ist_op* ops, int n_ops, int64_t canvas_w, int64_t canvas_h, const ist_image_desc* images,
                            int n_images, int filter, int n_slots, int split, ist_part* parts, int max_parts, int* n_parts);
/* IST_SPLIT_ROWS: cuts[0 .. n_slots] - equal rows per slot, every cut on a multiple of 8 rows, cuts[n_slots] = canvas_h; a
 * canvas shorter than 8 * n_slots rows leaves some slots empty (cuts[s] == cuts[s+1]; never slot 0) */
IST_API int ist_shard_row_cuts(int64_t canvas_h, int n_slots, int32_t* cuts);
/* the split IST_SPLIT_AUTO stands for on this op list (other values are returned unchanged); negative on error */
IST_API int ist_shard_resolve(const ist_op* ops, int n_ops, int64_t canvas_w, int64_t canvas_h, const ist_image_desc* images,
                              int n_images, int filter, int split);

/* ---- device path: inputs and output already resident in HBM ------------------------------------------------- */
IST_API ist_ctx* ist_ctx_create(int device);
IST_API void ist_ctx_destroy(ist_ctx* ctx);
/* waits for everything the context itself has in flight (its streams and staging lanes).  Hosts call it before process exit so
 * that no DMA of the library is still pending when the runtime (or a profiler attached to it) shuts down. */
IST_API int ist_ctx_sync(ist_ctx* ctx);
/* PNG export form for every *_png entry point of this context.  1 (default): Paeth filter + run-length matches + a
 * dynamic Huffman code per 16 KiB, all on the GPU: photographs shrink to about 0.43 x raw (smaller than zlib level 6 on
 * the same filtered stream), flat areas (gaps, screenshots) to 2-3 per cent; random data stays 1:1.  0: stored deflate
 * blocks, file = 1.001 x raw, one HBM-bound pass (3x faster).  Both decode to the same pixels
 * (canvasToTempFilePath quality:1 is lossless, utils/canvas.js:205-242). */
IST_API int ist_ctx_set_png_level(ist_ctx* ctx, int level);
/* PNG colour form for every *_png entry point of this context (single, batch, bitmaps, files, paths, *_png_preview, ist_render_png
 * and ist_png_encode_*).  IST_PNG_RGBA (default): colour type 6; every call does exactly what it did before this setting
 * existed.  IST_PNG_RGB: colour type 2, 8 bit - ALPHA IS NOT READ: R, G and B are taken as stored (the contract of the JPEG
 * export; a caller with a translucent canvas composites it first).  Every stitched canvas is opaque (the plan's white fillRect
 * lies under source-over), so for those the RGB file decodes to the same colours with 12-17 per cent fewer bytes on
 * photographs and more on flat content.  The filtered stream is, per row, filter byte 4 and the Paeth residuals of the 3 w colour
 * bytes (left / up / upper left: the same channel of the neighbouring PIXEL, zero outside the image, ties in that order); a row
 * is R = 3 w + 1 bytes, a chunk 16384 / R whole rows or, for R > 16384, a piece of one row of at most 5461 pixels; everything
 * behind the filter is the RGBA form's rule for rule.  An RGB canvas never has more chunks than the RGBA one, so ist_png_bound
 * is an upper bound for both forms.
 * IST_E_NO_CONTEXT for a NULL context, IST_E_INVALID for any other value.  The stored form (level 0) writes RGBA only: on a
 * context at level 0 with IST_PNG_RGB every *_png call fails with IST_E_UNSUPPORTED before anything is enqueued (the message
 * names pngLevel 1).  The setting is sampled once, when a call starts: a setter that
 * runs while a call is in flight changes the next call, never part of this one. */
enum { IST_PNG_RGBA = 0, IST_PNG_RGB = 1 };
IST_API int ist_ctx_set_png_color(ist_ctx* ctx, int color);
/* PNG row filters for every *_png entry point of this context (single, batch, bitmaps, files, paths, *_png_preview, ist_render_png
 * and ist_png_encode_*), in either colour form.  IST_PNG_FILTER_PAETH (default): filter type 4 on every row; every call does exactly
 * what it did before this setting existed.  IST_PNG_FILTER_ADAPTIVE: a type per row, chosen on the GPU by this rule.  For a canvas
 * in a colour form of bpp bytes per pixel (4 RGBA; 3 RGB, alpha not read) row y gets the filter type f of {0 None, 1 Sub, 2 Up,
 * 3 Average, 4 Paeth} with the least
 *     cost_f(y) = sum over the row's bpp w residual bytes r of (r < 128 ? r : 256 - r)
 * - the minimum sum of absolute differences; the filter byte itself is not counted.  Residuals follow the PNG specification
 * 9.2 - 9.4: left / up / upper left are the same channel of the neighbouring pixel and zero outside the image; Average is
 * (left + up) >> 1 on the unwrapped 0..255 values; Paeth breaks its ties as in the default form (left, up, upper left).  Ties
 * between filters go to the first of 4, 1, 2, 3, 0: Paeth wins ties, so a canvas on which nothing beats Paeth yields the default
 * form's stream bit for bit, and flat rows stay type 4 (on row 0, where Sub is Paeth and None is Up, neither Sub nor None is ever
 * chosen).  The choice is a function of the whole row's pixels and of the
 * row above only; it does not depend on the chunk grid or on the slabs.  Everything behind the filter is the existing rule
 * unchanged - grid, spans, tokens, code rule, stored against Huffman, pads, the Adler-32 over the filtered stream, slabs, the IDAT
 * layout - and so is the IHDR (filter method 0 allows a type per row) and ist_png_bound (the grid does not change, and the bound
 * counts every chunk as stored).  Files are 6-7 per cent smaller on photographs, 1-4 per cent on flat content; the heuristic can
 * lose a fraction of a per cent on a screenshot, which is why it is not the default.
 * IST_E_NO_CONTEXT for a NULL context, IST_E_INVALID for any other value.  The stored form (level 0) filters nothing: on a context
 * at level 0 with IST_PNG_FILTER_ADAPTIVE every *_png call fails with IST_E_UNSUPPORTED before anything is enqueued (the message
 * names pngLevel 1).  The setting is sampled once, when a call starts: a setter that
 * runs while a call is in flight changes the next call, never part of this one. */
enum { IST_PNG_FILTER_PAETH = 0, IST_PNG_FILTER_ADAPTIVE = 1 };
IST_API int ist_ctx_set_png_filter(ist_ctx* ctx, int filter);
/* PNG matches for every *_png entry point of this context (single, batch, bitmaps, files, paths, *_png_preview, ist_render_png and
 * ist_png_encode_*), in either colour form and with either row-filter setting.  IST_PNG_MATCH_RUN (default): a run of equal bytes
 * inside a 64-byte span is a literal and one match at distance 1; every call does exactly what it did before this setting existed.
 * IST_PNG_MATCH_WINDOW: a chunk may also copy from earlier spans of itself, by this rule.  In a chunk of n bytes b every position p
 * with p + 4 <= n has a key, the little-endian 32-bit word b[p..p+3], and H(p) = ((key * 2654435761) mod 2^32) >> 20.  cand(p) is the
 * greatest q with a key, H(q) == H(p) and q < 64 * (p / 64) - the most recent position of that hash in an earlier span - or none: a
 * function of the chunk's bytes alone.  Every span is parsed on its own from its first byte.  At p: run = the bytes from p on equal
 * to b[p], inside the span; m = the number of bytes for which b[cand(p) + i] == b[p + i], at most 63 and not past the span's end, 0
 * without a candidate (the source may run into the destination span: deflate's overlapping copy).  m >= 4 and m >= run: one match of m
 * bytes at distance p - cand(p); otherwise run >= 4: the literal and a match of run - 1 bytes at distance 1, as before; otherwise a
 * literal.  The literal/length code follows the existing code rule; a second code over the 30 distance symbols follows the same rule
 * (one distance symbol in use: length 1; none: symbol 0 with length 1); a chunk one of whose codes does not complete in the rule's 16
 * rounds has no window form.  The block is the run form's with HDIST = the highest distance symbol in use, its HDIST + 1 lengths
 * behind the 286 literal/length lengths in the same 4-bit code; a match is length code, length extra bits, distance code, distance
 * extra bits.  Per chunk the default setting's choice between stored and run form is made first, unchanged; the window form replaces
 * it only where its chunk, lead bytes and pads to 16 bytes included, is smaller (a tie keeps the default setting's bytes): no chunk
 * and no file is larger than with IST_PNG_MATCH_RUN, and ist_png_bound is unchanged.  Filter, colour form, grid, spans, stored form,
 * pads, the Adler-32, slabs, the IDAT layout and the IHDR are unchanged.  Rendered text comes out at half the bytes (49.9 per cent on a 4032 x 27216 canvas, profiles/r17_png_match.json), photographs
 * keep the run form in nearly every chunk, and the encoder takes several times as long, which is why it is not the default.
 * IST_E_NO_CONTEXT for a NULL context, IST_E_INVALID for any other value.  The stored form (level 0) matches nothing: on a context at
 * level 0 with IST_PNG_MATCH_WINDOW every *_png call fails with IST_E_UNSUPPORTED before anything is enqueued (the message names
 * pngLevel 1).  The setting is sampled once, when a call starts: a setter that
 * runs while a call is in flight changes the next call, never part of this one. */
enum { IST_PNG_MATCH_RUN = 0, IST_PNG_MATCH_WINDOW = 1 };
IST_API int ist_ctx_set_png_match(ist_ctx* ctx, int match);
/* compile an op list for a canvas (replaces createOffscreenCanvas + the recorded draw calls; utils/canvas.js:131,
 * index.js:1391-1428, 1532-1551).  clear_rgba = canvas initial colour ({0,0,0,0} for a fresh canvas).
 * clip = NULL renders the whole canvas; otherwise only that region is written (getImageData(0,0,1,1), 1564). */
IST_API ist_job* ist_job_create(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                                const ist_op* ops, int n_ops, const ist_image_desc* images, int n_images,
                                int filter, const ist_region* clip);
IST_API int ist_job_info_get(const ist_job* job, ist_job_info* out);
/* The destination row pitch (bytes) this job runs fastest on, for a host that allocates the canvas itself: 4 * canvas_w (dense rows)
 * when the job has a flat form - a strip of whole rows at unit scale, which ist_job_launch then walks as rows of 32 KiB - otherwise
 * 4 * canvas_w rounded up to a multiple of 4096 (measured: INTEGRATION.md "Row pitch").  Any pitch >= 4 * canvas_w that is a multiple
 * of 4 stays legal.  0 on a NULL job. */
IST_API size_t ist_job_preferred_dst_pitch(const ist_job* job);
/* one fused launch: every canvas pixel (in clip) is written exactly once.  src[i] / dst are DEVICE pointers.
 * stream = hipStream_t (NULL = default stream).  Asynchronous: returns after enqueueing. */
IST_API int ist_job_launch(ist_job* job, const void* const* src, const size_t* src_pitch, int n_images,
                           void* dst, size_t dst_pitch, void* stream);
/* N x the raster flush of Page.onStitch (index.js:1186-1633, utils/canvas.js:205-242) for N independent jobs of ONE context, in as
 * few kernel launches as possible: the jobs are grouped by the kernel form they need (a copy-only job never runs in the heavier
 * resampling form) and every group is ONE launch, all on `stream`.  Job k reads the source slots [first_k, first_k + n_images[k])
 * of the concatenated src / src_pitch tables (first_k = n_images[0] + ... + n_images[k-1]) and writes dst[k] with pitch
 * dst_pitch[k].  Every rule of ist_job_launch holds per job (the flat form included); every job is checked before anything is
 * enqueued, and a bad job k fails the whole call with a message that names k.  Jobs may share sources; destinations must not
 * overlap (not checked).  IST_E_INVALID: n_jobs <= 0 or jobs of different contexts; IST_E_UNSUPPORTED: n_jobs > 4096 or a
 * stream that is being captured into a graph.  The per-launch job table (2120 bytes per job + 4 bytes per 64 tiles) is
 * copied to the device on `stream` ahead of the kernels; asynchronous otherwise, like ist_job_launch. */
IST_API int ist_jobs_launch(ist_job* const* jobs, int n_jobs, const void* const* src, const size_t* src_pitch, const int* n_images,
                            void* const* dst, const size_t* dst_pitch, void* stream);
/* waits for the streams the job was launched on (not for the device: other streams keep running), then recycles its tables.
 * A job launched on the legacy default stream (NULL) inherits that stream's own implicit synchronisation rules. */
IST_API void ist_job_destroy(ist_job* job);

/* ---- host path: what stitch(images, direction, opts) binds (host RGBA8 in, host RGBA8 out) ------------------- */
/* Transfers of this group: the library never page-locks or registers memory it does not own.  Caller buffers (pageable,
 * any pitch) are packed through a ring of pinned chunks by a few host threads; buffers the library RETURNS are pinned
 * blocks of a process-wide pool, filled by one DMA, and go back to the pool through ist_free (ist_pool_trim releases the
 * idle ones).
 * index.js:1251-1581 minus decode (1441-1520) and PNG encode (1579): plan, then render.
 * *out_pixels is owned by the library (canvas_w*canvas_h*4 bytes, pitch canvas_w*4); release with ist_free. */
IST_API int ist_stitch_rgba8(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src,
                             const size_t* src_pitch, int n_images, int direction, int mode, double gap,
                             const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_pixels);
/* one request of ist_stitch_rgba8_batch: the arguments of one ist_stitch_rgba8 call (limits NULL = ist_limits_unlimited) */
typedef struct ist_stitch_request {
  const ist_image_desc* images;
  const uint8_t* const* src;
  const size_t* src_pitch;      /* NULL: dense rows */
  int32_t n_images;
  int32_t direction, mode;
  double gap;
  const ist_limits* limits;
  int32_t filter;
  int32_t reserved;
} ist_stitch_request;
/* N x Page.onStitch (index.js:1186-1633) minus decode and PNG encode: ist_stitch_rgba8 for every request, with the requests' op
 * tables uploaded in one copy per sub-batch and their canvases rendered by one ist_jobs_launch per sub-batch.  Sub-batches hold
 * at most 512 MiB of sources + canvases and two are in flight (one uploads while the previous one's canvases come down), which
 * bounds the device memory the context keeps.  out_plans[k] / out_pixels[k] are what ist_stitch_rgba8 would return for request k
 * (release with ist_plan_free / ist_free): every canvas is a pinned block of its own, from a class of the result pool that keeps
 * up to 8 GiB idle for the next batch (ist_pool_trim releases it).  A request without images gets out_pixels[k] = NULL and a
 * zeroed plan (its IST_NOTHING_TO_DO).  Any failing request fails the whole call (the message names it) and nothing is returned. */
IST_API int ist_stitch_rgba8_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, ist_plan* out_plans, uint8_t** out_pixels);
/* render a recorded Canvas op list into a caller buffer (the Canvas-2D shim's export / getImageData) */
IST_API int ist_render_rgba8(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                             const ist_op* ops, int n_ops, const ist_image_desc* images,
                             const uint8_t* const* src, const size_t* src_pitch, int n_images, int filter,
                             const ist_region* region, uint8_t* dst, size_t dst_pitch);
IST_API void ist_free(void* p);                /* any buffer the library returned through an out pointer */
IST_API void ist_pool_trim(void);              /* release the idle pinned blocks ist_free is keeping for reuse */

/* ---- device groups: one stitch on several GPUs from ONE process (stitch(images, direction, {devices})) ------ */
/* onStitchVertical/Horizontal -> onStitch (index.js:771-788 -> :1186) with the per-image iterations (:1439-1554) dealt to
 * the GPUs of `devices` (devices[0] = the root; a device may be listed more than once).  The job is cut by ist_shard_parts;
 * parts render on their devices, finished bands reach the root's canvas through ONE grouped ncclSend/ncclRecv batch
 * (RCCL over xGMI; librccl.so.1 is loaded on first use of a group with more than one device): full-width bands are
 * received in place, others are staged and placed by a 1:1 launch behind their receive.  Parts whose device is the
 * root's render straight into the canvas.  The one-process-per-GPU form of the same layout is imagestitching_amd/dist.py. */
typedef struct ist_group ist_group;
typedef struct ist_group_job ist_group_job;
IST_API ist_group* ist_group_create(const int* devices, int ndev);
IST_API void ist_group_destroy(ist_group* g);
IST_API int ist_group_slots(const ist_group* g);
IST_API int ist_group_device(const ist_group* g, int slot);            /* -1 when slot is out of range */
/* device-resident: compile once, launch on new buffers.  split = IST_SPLIT_IMAGE / IST_SPLIT_BAND. */
IST_API ist_group_job* ist_group_job_create(ist_group* g, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                                            const ist_op* ops, int n_ops, const ist_image_desc* images, int n_images, int filter,
                                            int split);
IST_API void ist_group_job_destroy(ist_group_job* job);
/* the part table of the job (parts == NULL: only the count); part k's owner device = ist_group_device(g, parts[k].slot) */
IST_API int ist_group_job_parts(const ist_group_job* job, ist_part* parts, int max_parts, int* n_parts);
/* src[k] / src_pitch[k] belong to PART k: the address, on the part's device, of row 0 of the part's image (a holder of rows
 * [sy0, sy1) only passes the address of row sy0 minus sy0 * pitch; 16 bytes behind its last row must be readable).
 * dst: the canvas on the root's device, dst_pitch == canvas_w * 4.  Asynchronous: ist_group_sync waits for the canvas.
 * The group runs on its own streams: whatever the caller queued on these buffers must have completed before the call. */
IST_API int ist_group_job_launch(ist_group_job* job, const void* const* src, const size_t* src_pitch, int n_parts, void* dst,
                                 size_t dst_pitch);
IST_API int ist_group_sync(ist_group* g);
/* host buffers in, host buffer out (ist_stitch_rgba8 on a group): every device uploads only the source rows its parts
 * sample, over its own PCIe link; *out_pixels is library-owned (ist_free). */
IST_API int ist_group_stitch_rgba8(ist_group* g, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                                   int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter,
                                   int split, ist_plan* out_plan, uint8_t** out_pixels);
/* the same in one call; groups are cached per device list for the life of the process */
IST_API int ist_stitch_rgba8_multi(const int* devices, int ndev, const ist_image_desc* images, const uint8_t* const* src,
                                   const size_t* src_pitch, int n_images, int direction, int mode, double gap,
                                   const ist_limits* limits, int filter, int split, ist_plan* out_plan, uint8_t** out_pixels);

/* ---- decode: PNG file -> RGBA8 (host; the Image.src step, utils/canvas.js:27-121, for 'png' inputs, index.js:4) ---- */
/* colour types 0/2/3/4/6, bit depths 1-16 (16-bit keeps the high byte), tRNS, plain or Adam7-interlaced.  JPEG / WebP /
 * HEIC return IST_E_UNSUPPORTED; damaged files IST_E_DECODE ('图片N解码异常' analogue).
 * Every decode entry point takes the CAPACITY of the output buffer (out_pitch bytes per row, out_rows rows) and fails
 * with IST_E_INVALID when the file's own header asks for more: the header is untrusted input. */
IST_API int ist_png_info(const uint8_t* file, int64_t len, int32_t* width, int32_t* height);
IST_API int ist_png_decode_rgba8(const uint8_t* file, int64_t len, uint8_t* out, size_t out_pitch, int64_t out_rows);
/* JPEG (baseline / extended sequential / progressive, 8 bit, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0, restart
 * intervals): Huffman decoding on the host, dequantise + IDCT + upsampling + colour conversion on the GPU.  *orientation = EXIF tag 0x0112
 * (0 when absent) - what getImageInfo feeds the planner (index.js:734).  Lossless / arithmetic-coded JPEG: IST_E_UNSUPPORTED. */
IST_API int ist_jpeg_info(const uint8_t* file, int64_t len, int32_t* width, int32_t* height, int32_t* orientation);
IST_API int ist_jpeg_decode_rgba8(ist_ctx* ctx, const uint8_t* file, int64_t len, uint8_t* out, size_t out_pitch, int64_t out_rows);
/* by signature: PNG, JPEG, BMP (uncompressed 1-32 bit, bit fields, RLE8 / RLE4), GIF (first frame) or WebP (lossless VP8L and lossy
 * VP8 key frames, with or without an ALPH chunk; orientation from the container's EXIF chunk; animation: the first frame) - every
 * raster member of SUPPORTED_IMAGE_TYPES (index.js:4).  ctx may be NULL for everything except JPEG (whose reconstruction
 * runs on the GPU). */
IST_API int ist_image_info(const uint8_t* file, int64_t len, int32_t* width, int32_t* height, int32_t* orientation);
IST_API int ist_image_decode_rgba8(ist_ctx* ctx, const uint8_t* file, int64_t len, uint8_t* out, size_t out_pitch, int64_t out_rows);

/* files -> decoded bitmaps in CALLER-OWNED DEVICE memory (the Image.src step ending in HBM): baseline JPEG entropy decoding
 * (one interleaved scan, at most two DC + two AC tables, with or without restart intervals) and reconstruction on the GPU, progressive JPEG / PNG / BMP / GIF entropy stages on host threads.  dst[i] must hold
 * dst_rows[i] rows of dst_pitch[i] bytes (sizes from ist_image_info); out_descs (optional) receives what the planner needs
 * (size, EXIF orientation, opaque).  Returns when the bitmaps are complete.
 * Ordering: the library writes dst[i] from its OWN streams.  Whatever the caller has queued on those buffers (a launch
 * that still reads the previous contents, a fill) must have completed before the call - the library cannot see the
 * caller's streams.  The Python host synchronises the tensors' current torch stream before it calls. */
IST_API int ist_decode_files_device(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images,
                                    void* const* dst, const size_t* dst_pitch, const int64_t* dst_rows, ist_image_desc* out_descs);
/* phase times of the last ist_stitch_files_png / ist_decode_files_device on this context, in milliseconds (measurement
 * aid: while on, every phase ends with a stream synchronisation) */
enum { IST_PHASE_HOST_DECODE = 0, IST_PHASE_PLAN_ARENA = 1, IST_PHASE_ENTROPY_GPU = 2, IST_PHASE_RECONSTRUCT = 3, IST_PHASE_STITCH = 4,
       IST_PHASE_PNG = 5, IST_PHASE_D2H = 6, IST_PHASE_COUNT = 8 };
IST_API int ist_ctx_set_timing(ist_ctx* ctx, int on);
IST_API int ist_ctx_last_timing(ist_ctx* ctx, double* ms, int n);

/* ---- reduced-size JPEG decode: 1/2, 1/4, 1/8 (csrc/ist_jpeg_scaled.hip; the decoded bitmap that is smaller than the image, bmp.width
 * against width, index.js:1522-1523) ----
 * A JPEG file decodes at 1 / d of its natural size, d = 1, 2, 4 or 8, from the coefficients the full-size decode reads: the entropy
 * stage is the same, the reconstruction is libjpeg-turbo's decode-to-scale (scale_num / scale_denom; Pillow's Image.draft), byte for
 * byte.  The contract (restated in numpy in tests/jpeg_scaled_reference.py), with N = 8 / d:
 *   - output size: sw = ceil(W N / 8), sh = ceil(H N / 8).
 *   - IDCT size S of a component sampled (h, v) (a lone component counts as 1 x 1): start at S = N; while S < 8 and
 *     (hmax N) mod (h S 2) == 0 and (vmax N) mod (v S 2) == 0, S doubles.  The component's true plane is cw = ceil(W h S / (hmax 8)) by
 *     ch = ceil(H v S / (vmax 8)) samples and is upsampled by ux = hmax N / (h S), uy = vmax N / (v S).  For the layouts the decoder
 *     takes: 4:2:0 chroma at 2 N without upsampling (at d = 2 luma is 4 x 4 and chroma the full 8 x 8), 4:2:2 keeps ux = 2, 4:4:0
 *     keeps uy = 2; ux = uy = 2 never occurs for d > 1.
 *   - upsampling: h2v1 and h1v2 are the triangle filters of the full-size decode with the same roundings ((3 near + far + 1) >> 2
 *     towards the previous sample, + 2 towards the next, edges replicated); h2v1 replicates when the scaled plane is at most 2
 *     samples wide; at d = 8 every upsampling is replication (libjpeg drops the filter when the smallest IDCT is 1 x 1).
 *   - reduced IDCT of the dequantised coefficients c[v][u], 32-bit arithmetic, DESCALE(x, n) = (x + (1 << (n - 1))) >> n
 *     (arithmetic shift), F(x) = round(8192 x):
 *       4 x 4: pass 1 on columns 0, 1, 2, 3, 5, 6, 7 reading rows 0, 1, 2, 3, 5, 6, 7 (index 4 is unused), pass 2 on the four rows
 *         over the same seven columns.  t0 = x0 << 14, t2 = x2 F(1.847759065) - x6 F(0.765366865), t10 = t0 + t2, t12 = t0 - t2,
 *         o0 = -x7 F(0.211164243) + x5 F(1.451774981) - x3 F(2.172734803) + x1 F(1.061594337),
 *         o2 = -x7 F(0.509795579) - x5 F(0.601344887) + x3 F(0.899976223) + x1 F(2.562915447);
 *         outputs 0..3 = t10 + o2, t12 + o0, t12 - o0, t10 - o2, DESCALEd by 12 in pass 1 and by 19 in pass 2.
 *       2 x 2: pass 1 on columns 0, 1, 3, 5, 7 reading rows 0, 1, 3, 5, 7, pass 2 on the two rows.  t10 = x0 << 15,
 *         t0 = -x7 F(0.720959822) + x5 F(0.850430095) - x3 F(1.272758580) + x1 F(3.624509785);
 *         outputs t10 + t0, t10 - t0, DESCALEd by 13 in pass 1 and by 20 in pass 2.
 *       1 x 1: DESCALE(c[0][0], 3).       8 x 8: the full-size IDCT.
 *     Every sample then gets + 128 and is clamped to 0..255.  Colour conversion, the RGB rule and alpha 255 are the full-size ones.
 * The denominator applies to every JPEG the decoder takes (baseline on the GPU Huffman path, sequential and progressive files on the
 * host entropy path); other file types decode at 1 / 1.  d = 1 runs the full-size launches and nothing else.  A denominator outside
 * {1, 2, 4, 8} is IST_E_INVALID, the message names the file, before anything is enqueued.  Every other rule is the unscaled call's. */
/* (sw, sh) of a w x h image at 1 / denom.  Pure CPU.  IST_E_INVALID: w or h < 1, a denominator outside {1, 2, 4, 8}, a NULL output */
IST_API int ist_jpeg_scaled_size(int32_t w, int32_t h, int32_t denom, int32_t* sw, int32_t* sh);
/* the largest d in {1, 2, 4, 8} with ceil(w / d) >= min_w and ceil(h / d) >= min_h, 1 if none qualifies: the denominator at which a
 * w x h file still covers min_w x min_h stored pixels.  Pure CPU.  IST_E_INVALID (negative) for a non-positive argument. */
IST_API int ist_decode_scale_fit(int32_t w, int32_t h, int32_t min_w, int32_t min_h);
/* ist_image_decode_rgba8 at 1 / denom: out holds sw x sh pixels (capacity checks use the scaled size) */
IST_API int ist_image_decode_rgba8_scaled(ist_ctx* ctx, const uint8_t* file, int64_t len, int32_t denom, uint8_t* out, size_t out_pitch,
                                          int64_t out_rows);
/* ist_decode_files_device with one denominator per file (denom == NULL: all 1, which IS ist_decode_files_device): dst[i] holds the
 * scaled bitmap; out_descs[i].width / height = the natural size, bmp_width / bmp_height = the scaled size of a JPEG decoded at d > 1
 * (0 = as natural for every other file, as ist_decode_files_device reports it). */
IST_API int ist_decode_files_device_scaled(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images, const int32_t* denom,
                                           void* const* dst, const size_t* dst_pitch, const int64_t* dst_rows, ist_image_desc* out_descs);
IST_API int64_t ist_debug_jpeg_scaled_launches(void);   /* reduced-IDCT launches made so far */

/* ---- files in, file out: the whole onStitch (decode -> plan -> resample+blit -> PNG export; index.js:1441-1581) ---- */
/* files[i] = the bytes of one image file of any type ist_image_info recognises.  Baseline JPEG: container parse + de-stuffing
 * on a host thread per image, Huffman decoding, reconstruction, stitch and PNG compression on the GPU; progressive JPEG /
 * PNG / BMP / GIF / WebP: entropy stage on that host thread, the rest on the GPU.  Decoded bitmaps, canvas and PNG stay in
 * HBM - only file bytes go in and PNG bytes come out.  A file that does not decode fails with IST_E_DECODE /
 * IST_E_UNSUPPORTED and the message '图片N解码异常: ...' (index.js:1512-1514).
 * files[i] must not change during the call: a file is parsed twice (frame header for the device layout, then the scan); a
 * JPEG whose frame layout differs between the two reads fails with IST_E_DECODE instead of overrunning the layout. */
IST_API int ist_stitch_files_png(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images,
                                 int direction, int mode, double gap, const ist_limits* limits, int filter,
                                 ist_plan* out_plan, uint8_t** out_png, int64_t* out_len);
/* the same from file PATHS (what wx.chooseImage hands the page: tempFilePaths, index.js:1441-1450): the library READS the
 * files (one parked worker per file) into blocks the context keeps from call to call - it does not map them, so a file that
 * another process rewrites or truncates meanwhile can neither change under the parsers nor raise SIGBUS in the host
 * process.  A path that cannot be opened, is not a regular file, is empty, or shrinks while it is read fails with
 * IST_E_DECODE and '图片N解码异常: ...'. */
IST_API int ist_stitch_paths_png(ist_ctx* ctx, const char* const* paths, int n_images,
                                 int direction, int mode, double gap, const ist_limits* limits, int filter,
                                 ist_plan* out_plan, uint8_t** out_png, int64_t* out_len);

/* ---- export: lossless PNG (fileType 'png', quality 1; utils/canvas.js:205-242, index.js:1577-1579) --------------- */
/* upper bound of the file size for a w x h canvas, in either colour form (ist_ctx_set_png_color: an RGB canvas never has more
 * chunks than the RGBA one, and the bound counts every chunk as stored) */
IST_API int64_t ist_png_bound(int64_t w, int64_t h);
/* encode a canvas that is resident in HBM into a device buffer (16-byte aligned, ist_png_bound bytes); one HBM-bound
 * pass; the checksums are combined on the host, so the call synchronises `stream` before it returns */
IST_API int ist_png_encode_device(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, void* out,
                                  int64_t out_cap, int64_t* out_len, void* stream);
/* N canvases resident in HBM -> N PNG files in caller device buffers, ONE compression launch (at the context's level) and one
 * gather launch for all of them; synchronises `stream` before it returns (checksums are combined on the host).  File k is
 * byte for byte the file ist_png_encode_device writes for canvas k.  Every canvas is checked by the rules of
 * ist_png_encode_device (out[k] 16-byte aligned, out_cap[k] >= ist_png_bound) before anything is enqueued; a bad one fails the
 * whole call with a message that names it.  IST_E_INVALID: n <= 0; IST_E_UNSUPPORTED: n > 4096. */
IST_API int ist_png_encode_batch_device(ist_ctx* ctx, const void* const* canvases, const size_t* pitch,
                                        const int64_t* w, const int64_t* h, int n, void* const* out,
                                        const int64_t* out_cap, int64_t* out_len, void* stream);
IST_API int64_t ist_debug_png_batch_launches(void);   /* compression launches made by batch encodes so far */
/* host pixels -> PNG bytes (library-owned, release with ist_free) */
IST_API int ist_png_encode_rgba8(ist_ctx* ctx, const uint8_t* pixels, size_t pitch, int64_t w, int64_t h,
                                 uint8_t** out_png, int64_t* out_len);
/* recorded Canvas op list -> PNG bytes (wx.canvasToTempFilePath of the shim); the canvas never leaves the device */
IST_API int ist_render_png(ist_ctx* ctx, int64_t canvas_w, int64_t canvas_h, const uint8_t clear_rgba[4],
                           const ist_op* ops, int n_ops, const ist_image_desc* images, const uint8_t* const* src,
                           const size_t* src_pitch, int n_images, int filter, uint8_t** out_png, int64_t* out_len);
/* onStitch stages 2-5 including the export: plan, render, PNG */
IST_API int ist_stitch_png(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src,
                           const size_t* src_pitch, int n_images, int direction, int mode, double gap,
                           const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png,
                           int64_t* out_len);
/* N x Page.onStitch with the export (index.js:1186-1633): ist_stitch_rgba8_batch with a PNG file in place of each canvas.  Every
 * sub-batch is rendered by one ist_jobs_launch and encoded straight from device memory by ONE compression launch (at the
 * context's level) and one gather launch; its files come down while the next sub-batch's sources go up.  out_png[k] /
 * out_len[k] are what ist_stitch_png returns for request k (the zlib stream byte for byte; IDAT chunk boundaries may differ),
 * each a pinned block of its real length from the batch class of the result pool (release with ist_free).  A request without
 * images gets NULL and a zeroed plan; any failing request fails the whole call (the message names it) and nothing is returned. */
IST_API int ist_stitch_png_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, ist_plan* out_plans,
                                 uint8_t** out_png, int64_t* out_len);

/* ---- resident bitmaps: decode or upload once, stitch again and again from HBM (the page's bitmap cache, index.js:534-627, used at
 * :1442 and :1515-1517: a reordered, re-gapped or turned stitch decodes nothing again) -------------------------------------------- */
/* One RGBA8 image in device memory that the LIBRARY owns: one block on the context's device, dense rows (4 * bitmap width bytes) plus
 * the readable tail every staged source has, and the image's desc (natural size, EXIF orientation, opaque, file_size) for the planner.
 * Reference-counted: the creator holds one reference (ist_bitmap_release drops it), every call that takes a bitmap holds one of its own
 * until it returns, and the block is freed when the last one drops - a host may release a bitmap while a call that uses it runs.
 * A bitmap outlives nothing: it does not keep its context alive, and it is usable with any context of its device. */
typedef struct ist_bitmap ist_bitmap;
/* host RGBA8 pixels (bitmap_w x bitmap_h of *desc, rows src_pitch bytes apart; 0 = dense) -> a new bitmap with *desc.  NULL on failure:
 * IST_E_NO_CONTEXT without a context, IST_E_DECODE '图片0解码异常' for NULL pixels or an empty bitmap, IST_E_INVALID for a short pitch */
IST_API ist_bitmap* ist_bitmap_upload(ist_ctx* ctx, const ist_image_desc* desc, const uint8_t* src, size_t src_pitch);
/* files -> n new bitmaps (out[i]): the decode of ist_decode_files_device into blocks of the library, desc[i] as ist_stitch_files_png
 * plans it (size, EXIF orientation, opaque for JPEG, file_size = lens[i]).  All or nothing: when file k fails, nothing is returned
 * (out[] is left NULL) and the message is '图片k解码异常: ...'.  n <= 0: IST_NOTHING_TO_DO; more than 128: IST_E_UNSUPPORTED. */
IST_API int ist_bitmaps_decode(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, ist_bitmap** out);
/* the same with one decode denominator per file (1, 2, 4, 8; NULL: all 1 - "reduced-size JPEG decode" above): a JPEG decoded at 1 / d
 * is an ordinary bitmap whose desc has bmp_width / bmp_height = the scaled size and width / height = the natural size, so plan,
 * stitch, previews, thumbnails and exports take it as it is; it holds 4 sw sh bytes (+ the tail) instead of 4 w h. */
IST_API int ist_bitmaps_decode_scaled(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, const int32_t* denom, ist_bitmap** out);
IST_API int ist_bitmap_desc(const ist_bitmap* b, ist_image_desc* out);
/* the pixels back into host memory (dst_rows rows of dst_pitch bytes must hold the bitmap) */
IST_API int ist_bitmap_download(ist_bitmap* b, uint8_t* dst, size_t dst_pitch, int64_t dst_rows);
IST_API void ist_bitmap_retain(ist_bitmap* b);
IST_API void ist_bitmap_release(ist_bitmap* b);
/* ist_stitch_rgba8 / ist_stitch_png with the bitmaps as the images: the descs are the bitmaps' own, and the one fused launch reads them
 * where they are (no source crosses PCIe); only the canvas, or its PNG file, comes down.  The result is byte for byte what the host
 * entry point returns for the same pixels and descs.  A NULL entry is IST_E_DECODE '图片N解码异常', a bitmap of another device than the
 * context's IST_E_INVALID, more than 128 bitmaps IST_E_UNSUPPORTED, n == 0 IST_NOTHING_TO_DO. */
IST_API int ist_stitch_bitmaps_rgba8(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap,
                                     const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_pixels);
IST_API int ist_stitch_bitmaps_png(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap,
                                   const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len);
IST_API int64_t ist_debug_bitmap_bytes(void);   /* device bytes held by the bitmaps alive in this process */

/* ---- previews: the stitched canvas, or a bitmap, shrunk from HBM (the redraw that follows the export, index.js:1597-1603: the exported
 * file is loaded back and drawn into the 343 x 457 preview node, shrunk to fit) ------------------------------------------------------ */
/* There is no raster rule of its own: the preview of a w x h RGBA8 image at pw x ph is what a fresh transparent pw x ph canvas reads back
 * after ONE drawImage(img, 0, 0, w, h, 0, 0, pw, ph) under IST_FILTER_AREA - the box over premultiplied values on an axis that shrinks,
 * the bilinear pair on one that does not, one rounding, straight alpha.  A draw that shrinks on BOTH axes (every preview of a result
 * larger than its box) runs a source-stationary reduce whose time follows 4 * w * h whatever the ratio (ist_preview.hip): every source
 * byte is read once, partial sums go to scratch of the context with plain stores and are added in a fixed order (no atomics: the same
 * input gives the same bytes).  Any other draw is a one-draw IST_FILTER_AREA job of the context.  EXIF orientation is not applied: a
 * bitmap's preview is of its stored pixels, as ist_bitmap_download's are. */
/* the fit rule (index.js:1600-1602) in IEEE double, Math.round = floor(x + 0.5): scaleFit = min(box_w / w, box_h / h), *out_w =
 * round(w * scaleFit), *out_h = round(h * scaleFit).  One deviation: each side is at least 1 (for a strip thin enough the reference
 * computes 0 and draws nothing).  Like the reference, the rule ENLARGES an image smaller than its box.  Pure CPU.  IST_E_INVALID: w or
 * h < 1, a box side that is not finite or <= 0, a NULL output. */
IST_API int ist_preview_fit(int64_t w, int64_t h, double box_w, double box_h, int32_t* out_w, int32_t* out_h);
/* device to device, asynchronous on `stream` (hipStream_t, NULL = default stream), like ist_job_launch.  src: w x h pixels, rows
 * src_pitch bytes apart (any multiple of 4 that is >= 4 * w); dst: pw x ph, dst_pitch likewise.  opaque: the caller's hint that every
 * alpha byte is 255 (the alpha bytes are then not read as weights; the preview's are 255).  The partial sums live in grow-only scratch
 * of the context; calls on different streams are ordered behind each other by an event, never by a host wait.  The one exception is a
 * draw that does NOT shrink on both axes (the job path): the context keeps the job of the last such shape, and a call with another
 * shape destroys it - which waits for the streams it ran on - and compiles a new one, whose tables go up with a blocking copy; a
 * repeated shape enqueues and returns.  Growing the scratch (a larger shape than any before) frees the old block, which also waits
 * for the device.  IST_E_NO_CONTEXT;
 * IST_E_INVALID: NULL buffers, w / h / pw / ph < 1, a short or unaligned pitch; IST_E_NO_DEVICE. */
IST_API int ist_preview_device(ist_ctx* ctx, const void* src, size_t src_pitch, int64_t w, int64_t h, int opaque,
                               void* dst, size_t dst_pitch, int32_t pw, int32_t ph, void* stream);
/* the preview an *_png_preview call returns beside its file */
typedef struct ist_preview {
  double  box_w, box_h;     /* in: the node the preview is fitted into (ist_preview_fit) */
  int32_t width, height;    /* out */
  uint8_t* pixels;          /* out: library-owned (pinned pool, release with ist_free); pitch 4 * width */
} ist_preview;
/* ist_stitch_png / ist_stitch_bitmaps_png / ist_stitch_files_png / ist_stitch_paths_png, with the preview of the canvas the file was
 * made from: ONE reduce of the canvas in HBM, queued behind the last render on a stream of its own - beside the encoder's last slab,
 * not in front of it, and with no host wait before the file's trip over PCIe starts.  The file is byte for byte the one the call
 * without `preview` returns; preview == NULL IS that call (nothing new is launched).  IST_E_INVALID: a box side that is not finite or
 * <= 0.  On any failure nothing is returned and preview->pixels is NULL. */
IST_API int ist_stitch_png_preview(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                                   int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter,
                                   ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview);
IST_API int ist_stitch_bitmaps_png_preview(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap,
                                           const ist_limits* limits, int filter, ist_plan* out_plan, uint8_t** out_png, int64_t* out_len,
                                           ist_preview* preview);
IST_API int ist_stitch_files_png_preview(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n_images,
                                         int direction, int mode, double gap, const ist_limits* limits, int filter,
                                         ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview);
IST_API int ist_stitch_paths_png_preview(ist_ctx* ctx, const char* const* paths, int n_images,
                                         int direction, int mode, double gap, const ist_limits* limits, int filter,
                                         ist_plan* out_plan, uint8_t** out_png, int64_t* out_len, ist_preview* preview);
/* a bitmap's stored pixels at pw x ph into host memory (ph rows of dst_pitch >= 4 * pw bytes): a thumbnail without the 48 MB of
 * ist_bitmap_download.  IST_E_INVALID: NULL bitmap or dst, pw / ph < 1, a short pitch, a bitmap of another device than the context's. */
IST_API int ist_bitmap_preview(ist_ctx* ctx, ist_bitmap* b, int32_t pw, int32_t ph, uint8_t* dst, size_t dst_pitch);
/* launches of the source-stationary reduce in this process so far (tests tell it from the job path with it) */
IST_API int64_t ist_debug_preview_launches(void);
/* the workgroup shape the reduce runs a w x h -> pw x ph preview with (pure CPU, no context: tests assert the regime of a case with
 * it, as with ist_debug_cells): out = per_group (output pixels that share one 256-column footprint), groups (per output row), passes
 * (256-column passes over a footprint), sub (lanes that fold one box), chunk_rows, chunks (row chunks per box).  Returns 1 with out
 * zeroed for a shape that does not shrink on both axes (the job path).  IST_E_INVALID: NULL out. */
IST_API int ist_debug_preview_geometry(int64_t w, int64_t h, int32_t pw, int32_t ph, int32_t out[6]);
/* the chunk grid the compressing PNG encoder cuts a w x h canvas into, in colour form `color` (pure CPU, no context): out = n_chunks,
 * rows_per_chunk (0: a chunk is a piece of one row), pieces_per_row, piece_px.  IST_E_INVALID: w or h < 1, an unknown colour form,
 * NULL out. */
IST_API int ist_debug_png_grid(int64_t w, int64_t h, int color, int64_t out[4]);

/* ---- thumbnails: a grid of images cropped, turned and shrunk together (the page's grid of chosen images: one <image mode="aspectFill">
 * per image at thumbWpx x thumbWpx, pages/index/index.wxml:4-22, cell size from index.js:313-343; the modal image of index.wxml:202 is
 * the aspectFit form) ------------------------------------------------------------------------------------------------------------- */
/* The rule, pure CPU, IEEE double without FMA (like ist_preview_fit).  A stored bitmap bw x bh (bmp_width / bmp_height of its desc when
 * given, else width / height) has orientation o in 1..8 (0 or anything outside 1..8 counts as 1).  Its DISPLAYED size W x H is bw x bh
 * for o <= 4 and bh x bw for o >= 5, and the displayed image is the standard EXIF one (S the stored array, rows first):
 *     1  S              2  S[:, ::-1]         3  S[::-1, ::-1]       4  S[::-1]
 *     5  S.T            6  S.T[:, ::-1]       7  S.T[::-1, ::-1]     8  S.T[::-1]
 * (6 is the quarter turn clockwise).  Orientation 7 is the TRUE transverse here.  The stitch reproduces utils/canvas.js:187-192 as
 * written, which is a quirk of drawWithOrientation; an <image> node never goes through that function, so a thumbnail does not copy it.
 * IST_THUMB_FILL (aspectFill) into a cell tw x th, everything in displayed space:
 *     tw / W >= th / H:  cw = W, ch = clamp(floor(th * W / tw + 0.5), 1, H);    otherwise:  ch = H, cw = clamp(floor(tw * H / th + 0.5), 1, W)
 *     cx = floor((W - cw) / 2), cy = floor((H - ch) / 2);  the window (cx, cy, cw, ch) is shrunk to tw x th
 * IST_THUMB_FIT (aspectFit): the window is the whole image, the output is ist_preview_fit(W, H, tw, th).
 * apply_orientation == 0: every image is treated as o = 1 (ist_bitmap_preview's stored pixels, with a crop).
 * Pixels: the window is mapped back into stored space - a mirrored axis puts the floor's spare pixel on the other side
 * (x_stored = bw - cx - cw) - and the output is the displayed-space orientation of the PREVIEW (the contract above: one drawImage
 * under IST_FILTER_AREA on a fresh transparent canvas) of that stored window at the output size, sides swapped for o >= 5.  No new
 * weights, clamps or rounding. */
enum { IST_THUMB_FILL = 0, IST_THUMB_FIT = 1 };
/* ist_thumb_item.turn: the reduced stored window is mirrored along x (FLIP_X) and / or y (FLIP_Y), THEN its axes are swapped (TRANSPOSE) */
enum { IST_TURN_FLIP_X = 1, IST_TURN_FLIP_Y = 2, IST_TURN_TRANSPOSE = 4 };
typedef struct ist_thumb_spec {
  int32_t cell_w, cell_h;       /* tw, th: >= 1 */
  int32_t mode;                 /* IST_THUMB_FILL / IST_THUMB_FIT */
  int32_t apply_orientation;    /* 0: every image as orientation 1 */
} ist_thumb_spec;
typedef struct ist_thumb_item {
  int32_t width, height;        /* the thumbnail, displayed space */
  int32_t src_x, src_y, src_w, src_h;   /* the window in STORED space */
  int32_t turn;                 /* IST_TURN_* bits that take the shrunk stored window to the thumbnail */
  int32_t reserved;
  int64_t offset;               /* of the thumbnail's first byte in the output block; rows are 4 * width bytes, thumbnails dense */
} ist_thumb_item;
/* the rule for n images: out[k] for descs[k]; offsets are dense (out[k + 1].offset = out[k].offset + 4 * width * height), *out_bytes
 * (optional) their end.  IST_E_INVALID: NULL descs / spec / out, n < 0, a cell side < 1, an unknown mode, an empty image (the message
 * names it); IST_E_UNSUPPORTED: n > 4096. */
IST_API int ist_thumb_layout(const ist_image_desc* descs, int n, const ist_thumb_spec* spec, ist_thumb_item* out, int64_t* out_bytes);
/* device to device, asynchronous on `stream` like ist_preview_device: image k is bitmap_w x bitmap_h of descs[k] at src[k], rows
 * pitch[k] bytes apart (a multiple of 4, >= 4 * width); thumbnail k lands at dst + out[k].offset (dst_cap bytes must hold them all).
 * Images that shrink on both axes are reduced TOGETHER: per form (descs[k].opaque set or not) one stage-1 and one stage-2 launch of
 * the batch twins of the preview reduce cover every such image of a sub-batch - as many images as keep the partial sums within
 * 256 MiB of the context's grow-only preview scratch (every image of a 9-image grid, and of any grid of phone photos) - and their
 * table goes up in one copy.  The crop costs nothing (a window is a base address and a size) and the turn lives in stage 2's store;
 * pixel for pixel the bytes are ist_preview_device's of the stored window, turned.  An image that does NOT shrink on both axes (smaller
 * than its cell on an axis: the rare case) is a one-draw IST_FILTER_AREA job whose CTM is the turn; those jobs are launched together
 * by one ist_jobs_launch and then destroyed, which waits for `stream` - a call with such an image is not asynchronous.  Those jobs
 * are compiled before anything is enqueued: a call that fails on one of them leaves nothing in flight.
 * IST_E_NO_CONTEXT; IST_E_INVALID: what ist_thumb_layout rejects, NULL tables, n < 1, a short dst_cap, a short or unaligned pitch;
 * IST_E_DECODE '图片N解码异常': src[N] is NULL; IST_E_UNSUPPORTED: n > 4096. */
IST_API int ist_thumbs_device(ist_ctx* ctx, const ist_image_desc* descs, const void* const* src, const size_t* pitch, int n,
                              const ist_thumb_spec* spec, void* dst, int64_t dst_cap, ist_thumb_item* out, void* stream);
/* the same over resident bitmaps (descs and pixels are the bitmaps' own), and the thumbnails come down in ONE copy into ONE pinned
 * block of the pool: *out_pixels (release with ist_free), thumbnail k at out[k].offset.  A NULL bitmap is IST_E_DECODE '图片N解码异常', a
 * bitmap of another device than the context's IST_E_INVALID; the call holds its own references until it returns.  n < 1: IST_E_INVALID. */
IST_API int ist_bitmaps_thumbs(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, const ist_thumb_spec* spec, ist_thumb_item* out,
                               uint8_t** out_pixels);
/* launch PAIRS (one stage-1 + one stage-2 launch of the batch reduce) made by thumbnail calls in this process so far */
IST_API int64_t ist_debug_thumb_launches(void);

/* ---- export: baseline JPEG (fileType 'jpg'; the seam is safeCanvasToTempFilePath's `prefer`, utils/canvas.js:205-221; the page's
 *      other file producer, wx.compressImage, utils/canvas.js:262, writes JPEGs) -------------------------------------------------
 * A w x h RGBA8 canvas becomes a baseline JFIF file, 1 <= w, h <= 65535 (a larger side: IST_E_UNSUPPORTED, the message names the
 * side).  quality is 1..100, subsampling IST_JPEG_420 or IST_JPEG_444.  The file is pinned byte for byte; all arithmetic is signed
 * integer, '>>' an arithmetic shift, '//' floor division of non-negative numbers:
 *   - ALPHA IS NOT READ: R, G and B are taken as stored.  Every stitched canvas is opaque (the plan's white fill sits under
 *     source-over); a caller with a translucent canvas composites it first.
 *   - colour, per pixel:   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                          Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *                          Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16        (all in 0..255, no clamp)
 *   - padding: the planes are extended to whole MCUs (16x16 for 4:2:0, 8x8 for 4:4:4) by repeating the last column and row;
 *   - 4:2:0 chroma, after padding: (a + b + c + d + 2) >> 2 over each 2x2;  level shift: s = v - 128;
 *   - FDCT, integer matrix form: T[u][x] = 2896 for u = 0, else sign * {4017, 3784, 3406, 2896, 2276, 1567, 799}[k-1] with
 *     k = (2x+1) u mod 32 folded into the first quadrant (= round(8192 a(u) cos((2x+1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2);
 *     rows r[y][u] = (sum_x T[u][x] s[y][x] + 512) >> 10, columns c[v][u] = (sum_y T[v][y] r[y][u] + 4096) >> 13: c is 8 x the
 *     orthonormal coefficient, every intermediate fits 32 bits;
 *   - quantisation tables: libjpeg's rule on T.81 tables K.1 / K.2: scale = 5000 // Q for Q < 50, else 200 - 2 Q;
 *     q = clamp((base scale + 50) // 100, 1, 255); luma in slot 0, chroma in slot 1;
 *   - quantise: k = sign(c) ((|c| + 4 q) // (8 q)); AC values clamped to +-1023 (a guard: 8-bit input does not reach it);
 *   - container: SOI, APP0 (JFIF 1.01, units 0, density 1x1), DQT 0, DQT 1 (8-bit, zig-zag order), DHT DC0, DC1, AC0, AC1 (Annex K
 *     tables K.3 - K.6), DRI = R, SOF0 (components 1, 2, 3; slots 0, 1, 1), SOS, the intervals, EOI.  One interleaved scan; R =
 *     ceil(w / MCU width), so one restart interval is one MCU row: its DC predictors restart, it is padded with 1 bits to a byte,
 *     every 0xFF is followed by 0x00, and RST((k-1) mod 8) stands between intervals k-1 and k.
 * Such files are eligible for the library's own GPU Huffman decoder (ist_decode_files_device).
 *
 * OPTIMISED HUFFMAN TABLES: IST_JPEG_OPTIMIZE, OR-ed into any `subsampling` argument below (as IST_FILTER_EDGE_AA is OR-ed into
 * `filter`), gives the file the four Huffman tables that are optimal for its own symbols.  Only the four DHT segments (still in
 * the order DC0, DC1, AC0, AC1) and the codes in the scan differ from the file without the flag; colour, padding, FDCT, quantiser,
 * clamps, DQTs, DRI, SOF0, SOS, the intervals, their padding, stuffing, the RSTn order and EOI do not.  Without the flag every call
 * does what it did before the flag existed.  Any value other than IST_JPEG_444 / IST_JPEG_420 with or without the flag is an
 * unknown subsampling (2, 3, 7, -1, 0x200, 0x102, ...).
 *   - symbol counts, exact 64-bit integers taken over the whole file, all intervals together (a 65535 x 65535 4:4:4 file has more
 *     than 2^32 AC symbols):
 *       DC slot 0: the size category 0..11 of every Y block's DC difference; the predictor restarts at 0 at the start of every
 *                  interval and the difference is clamped to +-2047 (as the scan codes it);   DC slot 1: the same over Cb and Cr;
 *       AC slot 0 (Y) / slot 1 (Cb, Cr): every run/size symbol 16 run + size a block emits, AC values clamped to +-1023; 0xF0 once
 *                  per ZRL (16 zeros in front of a non-zero value), 0x00 once per block that ends in zeros;
 *   - the table of one histogram (T.81 K.2; ist_jpeg_optimal_table is this rule):
 *       1. leaves: every symbol with a count > 0, and a reserved symbol 256 with count 1; a leaf is a node (weight, id = symbol);
 *       2. repeatedly take the two nodes that are smallest by (weight, id) and merge them into (sum of weights, smaller id); the
 *          code size of every symbol inside the merged node grows by 1;
 *       3. BITS[l] = number of leaves of size l, the reserved one included;
 *       4. while a size above 16 is populated (T.81 figure K.3), from the largest size i downwards: take two from size i, find
 *          the nearest populated j <= i - 2, then BITS[i] -= 2, BITS[i-1] += 1, BITS[j+1] += 2, BITS[j] -= 1;
 *       5. remove one code from the largest populated size (the reserved point: no code is all ones);
 *       6. HUFFVAL = the real symbols sorted by (size before step 4, symbol value);
 *       7. codes are canonical (T.81 C.2).
 *     An empty histogram gives 16 zero BITS and no values (no real file has one: every table sees a DC symbol or an EOB).
 *   - bound: an optimised DC code may be 16 bits long (Annex K's longest is 11), so a block is at most 27 + 63 x 26 = 1665 bits, 417
 *     bytes after stuffing: with the flag slot = (row_blocks * 417 + 2 + 15) & ~15 and
 *         bound = 1024 + MCU rows x (blocks per MCU row x 417 + 16);
 *     the header is at most 629 bytes (a DC table has at most 12 symbols, an AC table at most 162, as in Annex K). */
enum { IST_JPEG_444 = 0, IST_JPEG_420 = 1 };
enum { IST_JPEG_OPTIMIZE = 0x100 };
/* BITS (16 counts, lengths 1..16) and HUFFVAL (n_vals symbols) of the optimal table of 256 symbol counts, by the rule above.  Pure
 * CPU, no context.  IST_E_INVALID: a NULL argument, a negative count. */
IST_API int ist_jpeg_optimal_table(const int64_t freq[256], uint8_t bits[16], uint8_t vals[256], int* n_vals);
/* the two quantisation tables of a quality, natural order.  Pure CPU.  IST_E_INVALID: quality outside 1..100, a NULL table */
IST_API int ist_jpeg_quant_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
/* an upper bound of the file's size that the encoder guarantees; negative for bad arguments (a side < 1 or > 65535, an unknown
 * subsampling).  Pure CPU.  A block is at most 22 bits of DC (an 11-bit code + 11 bits) + 63 x 26 bits of AC (a 16-bit code + 10
 * bits) = 1660 bits before stuffing; stuffing at most doubles a byte: 415 bytes per block.  An interval adds at most one pad byte
 * (which may be stuffed) and its 2-byte marker, the file 629 bytes of header and 2 of EOI:
 *     bound = 1024 + MCU rows x (blocks per MCU row x 415 + 16)        (with IST_JPEG_OPTIMIZE: 417, see above). */
IST_API int64_t ist_jpeg_bound(int64_t w, int64_t h, int subsampling);
/* encode a canvas that is resident in HBM into a device buffer (16-byte aligned, out_cap >= ist_jpeg_bound): transform, entropy
 * code and gather run on `stream`, which is synchronised before the call returns (the host lays the intervals out).  Every argument
 * is checked before anything is enqueued.  IST_E_NO_CONTEXT; IST_E_INVALID: quality outside 1..100, an unknown subsampling, NULL
 * buffers, w or h < 1, a pitch < 4 w or not a multiple of 4, a short out_cap, an unaligned out; IST_E_UNSUPPORTED: a side above 65535. */
IST_API int ist_jpeg_encode_device(ist_ctx* ctx, const void* canvas, size_t pitch, int64_t w, int64_t h, int quality, int subsampling,
                                   void* out, int64_t out_cap, int64_t* out_len, void* stream);
/* host pixels -> JPEG bytes (a pooled pinned block of the file's length, release with ist_free) */
IST_API int ist_jpeg_encode_rgba8(ist_ctx* ctx, const uint8_t* pixels, size_t pitch, int64_t w, int64_t h, int quality, int subsampling,
                                  uint8_t** out_jpeg, int64_t* out_len);
/* ist_stitch_png / ist_stitch_bitmaps_png with the JPEG export: the canvas is rendered exactly as for ist_stitch_rgba8 and never
 * leaves the device; only the file comes down, in one copy of its real length.  The file is byte for byte ist_jpeg_encode_device of
 * the canvas ist_stitch_rgba8 returns.  Errors: those of the PNG call, and of ist_jpeg_encode_device for quality, subsampling and the
 * canvas size (checked before anything is rendered). */
IST_API int ist_stitch_jpeg(ist_ctx* ctx, const ist_image_desc* images, const uint8_t* const* src, const size_t* src_pitch,
                            int n_images, int direction, int mode, double gap, const ist_limits* limits, int filter, int quality,
                            int subsampling, ist_plan* out_plan, uint8_t** out_jpeg, int64_t* out_len);
IST_API int ist_stitch_bitmaps_jpeg(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, int direction, int mode, double gap,
                                    const ist_limits* limits, int filter, int quality, int subsampling, ist_plan* out_plan,
                                    uint8_t** out_jpeg, int64_t* out_len);
/* transform launches (one per slab of MCU rows) made by JPEG encodes in this process so far.  With IST_JPEG_OPTIMIZE the whole file
 * is counted before its first interval is coded: a file of one slab keeps its coefficients (1 launch), a file of N > 1 slabs is
 * transformed twice (2 N launches). */
IST_API int64_t ist_debug_jpeg_encode_launches(void);
/* histogram launches (IST_JPEG_OPTIMIZE: one per slab of a single file, one per counted round of a batch) so far */
IST_API int64_t ist_debug_jpeg_histogram_launches(void);
/* the symbol counts that the context's last encode with IST_JPEG_OPTIMIZE made, as its histogram kernel left them: the first n
 * counters of the block, 544 per optimised file of that call in file order; per file and table slot (luma, then chroma) 16 DC sizes,
 * then 256 AC symbols.  Synchronises the context's stream and copies; launches nothing.  IST_E_NO_CONTEXT; IST_E_INVALID: a NULL out,
 * n negative, no multiple of 544 or above what the block holds (it grows with the calls and is never cleared between them). */
IST_API int ist_debug_jpeg_counts(ist_ctx* ctx, int64_t* out, int64_t n);

/* ---- batched JPEG export: many canvases per launch --------------------------------------------------------------------------
 * The encoder's unit of work is the restart interval (one MCU row), and an interval of file A needs an interval of file B as little
 * as another interval of file A: a batch is the intervals of many files in one grid per kernel.  A batch runs in ROUNDS: as many
 * MCU rows, in file order, as keep coefficients + interval slots within the encoder's scratch budget (256 MiB).  One MCU row costs
 * row_blocks * 128 + slot bytes, row_blocks = ceil(w / MCU width) x blocks per MCU, slot = (row_blocks * 415 + 2 + 15) & ~15.  A round
 * closes when the next row would not fit; a row above the budget on its own gets a round to itself.  The run of consecutive MCU
 * rows of one file in one round is a PIECE; a file above the budget spans rounds as several pieces, in order.  One round is one
 * transform, one entropy and one gather launch, one stream synchronisation (the host lays the intervals out, per file) and ONE
 * host-to-device copy (tables, headers, piece records); the gather writes every byte of a file, header and EOI included.
 * Files with IST_JPEG_OPTIMIZE (their rows cost the 417-byte slot) may be mixed with files without: a batch of one round
 * transforms once, counts the optimised pieces, synchronises once more and sends the block up again with the files' own tables
 * and headers; a batch of several rounds first transforms and counts every round that holds an optimised piece, then runs its
 * rounds (at most two transform launches per round). */
typedef struct ist_jpeg_piece { int32_t file, round, mcu_row0, mcu_rows; } ist_jpeg_piece;
/* pieces of a batch in encoding order; budget_bytes 0 = the encoder's own.  Returns the number of pieces (also when out is NULL or cap
 * is too small: nothing is written beyond cap), negative on a bad argument (n < 1, a NULL array, a side outside 1..65535, an unknown
 * subsampling, a negative budget or cap).  Pure CPU. */
IST_API int64_t ist_jpeg_batch_layout(const int64_t* w, const int64_t* h, const int* subsampling, int n,
                                      int64_t budget_bytes, ist_jpeg_piece* out, int64_t cap);
/* ist_jpeg_encode_device for n canvases: file k is byte for byte the file that call writes for canvas k with quality[k] and
 * subsampling[k].  Every file is checked by that call's rules before anything is enqueued; a bad file fails the whole call with a
 * message that names it ("file k: ...").  n <= 0 or a NULL array: IST_E_INVALID; n > 4096: IST_E_UNSUPPORTED.  `stream` is
 * synchronised before the call returns. */
IST_API int ist_jpeg_encode_batch_device(ist_ctx* ctx, const void* const* canvases, const size_t* pitch, const int64_t* w,
                                         const int64_t* h, const int* quality, const int* subsampling, int n,
                                         void* const* out, const int64_t* out_cap, int64_t* out_len, void* stream);
/* ist_stitch_png_batch with a JPEG in place of each PNG: the same sub-batches through the same two halves, each sub-batch's canvases
 * encoded by the batch encoder; file k is byte for byte the file ist_stitch_jpeg returns for request k with quality[k] and
 * subsampling[k].  A request without images gets NULL, length 0 and a zeroed plan.  All or nothing: a failing request fails the
 * call, the message names it ("request k: ..."), and nothing is returned. */
IST_API int ist_stitch_jpeg_batch(ist_ctx* ctx, const ist_stitch_request* reqs, int n_reqs, const int* quality,
                                  const int* subsampling, ist_plan* out_plans, uint8_t** out_jpeg, int64_t* out_len);
/* rounds (one transform launch each) made by batch encodes in this process so far */
IST_API int64_t ist_debug_jpeg_batch_launches(void);

/* ---- lossless JPEG joins: a strip of compatible JPEG files becomes one JPEG in the coefficient domain -------------------------
 * What jpegtran does for one file, done for a strip: the sources' QUANTISED coefficients (the decoder's dense planes, see
 * ist_debug_jpeg_gpu_coefficients) are moved, block by block, into the export's coefficient scratch and entropy-coded by the export's
 * kernels.  No pixel is ever made: no IDCT, no colour conversion, no stitch, no FDCT, no second quantisation, no generation loss, and
 * no quality to choose.
 *
 * THE RULE.  A join of n files (1 <= n <= 128) in `direction` IST_VERTICAL or IST_HORIZONTAL:
 *   - layout and tables: the result has image 0's sampling layout (4:4:4 or 4:2:0) and image 0's quantisation tables.  The header is
 *     the export's (SOI, APP0, DQT x 2, DHT x 4, DRI, SOF0, SOS) with DQT 0 = the SOURCES' luma table and DQT 1 = the sources' chroma
 *     table, not the tables of a quality;
 *   - geometry: vertical W = w_0, H = sum h_i, and component c's block rows are the sources' block rows of that component, one image
 *     after the other; horizontal H = h_0, W = sum w_i, and each block row is the sources' block rows of the same index side by
 *     side.  (W, H) is the canvas ist_plan_compute gives for these images with IST_MODE_MIN, gap 0, unlimited caps (super-sample 1);
 *   - everything else is the export's contract unchanged: one restart interval per MCU row, DC predictors zero at each interval, the
 *     Annex K tables (or, with IST_JPEG_OPTIMIZE, the file's optimal tables by the rule above), padding bits, stuffing, RSTn order, EOI.
 *   So the file equals, byte for byte, the export's file of a frame whose coefficient arrays are the sources' arrays concatenated
 *   along the block-row axis (vertical) or the block-column axis (horizontal).
 *
 * ELIGIBILITY is decided from the headers alone, by the decoder's own parser (the segments are walked and the scan headers read as a
 * decode reads them, up to the scan header that fixes the last component's table; no entropy-coded byte is decoded).  Images are looked at in order and, per image, the reasons in the order of this
 * list; the first failing image and its reason are reported:
 *   IST_JOIN_NOT_JPEG  not a JPEG, or one the decoder refuses (its message is kept);
 *   IST_JOIN_LAYOUT    not three components in the YCbCr colour space (the decoder's libjpeg rule: JFIF, Adobe transform, component
 *                      ids), or a sampling layout other than 4:4:4 / 4:2:0, the two the export writes;
 *   IST_JOIN_MIXED     the layout differs from image 0's;
 *   IST_JOIN_TABLES    a component's quantisation table (the one in force when its first scan starts, as the decoder latches it)
 *                      differs from image 0's; in image 0, Cb's differs from Cr's, or an entry is 0 or above 255 (a DQT the export's
 *                      8-bit segment cannot carry; a component no scan names has an all-zero table);
 *   IST_JOIN_SIZE      widths differ (vertical) or heights differ (horizontal);
 *   IST_JOIN_ALIGN     an image other than the last has a height (vertical) or width (horizontal) that is not a multiple of the MCU
 *                      size (8 for 4:4:4, 16 for 4:2:0).  The last image may be partial on both axes, and every image may be partial
 *                      across the join axis;
 *   IST_JOIN_ORIENT    EXIF orientation above 1 (lossless turns are out of scope);
 *   IST_JOIN_LIMIT     the joined side (sum of heights, vertical; of widths, horizontal) exceeds 65535 at this image; also n > 128
 *                      (image = 128, decided before any file is read);
 *   IST_JOIN_RANGE     found on the device only, by ist_jpeg_join_files: a DC outside [-1024, 1023] or an AC outside [-1023, 1023].
 *                      The entropy kernel would clamp such a value silently and the join would not be lossless; inside these bounds
 *                      every coded DC difference is within +-2047.  Every 8-bit baseline file of a real encoder is inside them.  The
 *                      call fails and no file is returned (image = -1: the kernel does not say which).
 * The context's colour-profile setting is not read: no pixel exists, and the export writes no profile anyway.  EXIF and ICC segments
 * of the sources are not carried. */
enum { IST_JOIN_OK = 0, IST_JOIN_NOT_JPEG = 1, IST_JOIN_LAYOUT = 2, IST_JOIN_MIXED = 3, IST_JOIN_TABLES = 4, IST_JOIN_SIZE = 5,
       IST_JOIN_ALIGN = 6, IST_JOIN_ORIENT = 7, IST_JOIN_LIMIT = 8, IST_JOIN_RANGE = 9 };
typedef struct ist_jpeg_join_info {
  int32_t reason, image;      /* IST_JOIN_*; the first failing image (-1: none) */
  int32_t subsampling;        /* IST_JPEG_444 / IST_JPEG_420 of image 0 once it is known to have one of them, else -1 */
  int32_t reserved;
  int64_t width, height;      /* of the joined file when reason is IST_JOIN_OK, else 0 */
} ist_jpeg_join_info;
/* Pure CPU, no context: headers only.  Returns 0 and reason = IST_JOIN_OK, or IST_E_UNSUPPORTED with reason / image filled and a
 * message that names the image and the reason ("image k: ...").  IST_E_INVALID for NULL arrays, n <= 0 or an unknown direction (a
 * NULL or empty entry of `files` is IST_JOIN_NOT_JPEG of that image).  out may be NULL. */
IST_API int ist_jpeg_join_check(const uint8_t* const* files, const int64_t* lens, int n, int direction, ist_jpeg_join_info* out);
/* files -> one JPEG (a pooled pinned block of the file's length, release with ist_free).  flags: 0 or IST_JPEG_OPTIMIZE.  The files are
 * entropy-decoded as ist_decode_files_device decodes them (the GPU Huffman decoder where it takes the file, the host decoders
 * otherwise) but stop at the coefficient planes; one join launch per slab of MCU rows fills the encoder's scratch in place of its
 * transform, and the export's entropy (histogram, gather) launches run unchanged.  With IST_JPEG_OPTIMIZE and more than one slab the
 * fill runs twice, as the transform does.  Errors, in this order: IST_E_NO_CONTEXT; IST_E_INVALID: unknown flags, then NULL arrays /
 * n <= 0 / an unknown direction ("bad argument"), then a NULL output; then what ist_jpeg_join_check refuses (out_info, optional, is
 * filled as by that call); a file whose scan does not decode: IST_E_DECODE '图片N解码异常: ...'; IST_JOIN_RANGE (IST_E_UNSUPPORTED).
 * On any failure *out_jpeg is NULL and nothing is held. */
IST_API int ist_jpeg_join_files(ist_ctx* ctx, const uint8_t* const* files, const int64_t* lens, int n, int direction, int flags,
                                ist_jpeg_join_info* out_info, uint8_t** out_jpeg, int64_t* out_len);
/* join launches (one per slab of MCU rows; two with IST_JPEG_OPTIMIZE and more than one slab) made in this process so far.  A join
 * makes no transform, reconstruction or stitch launch: ist_debug_jpeg_encode_launches does not move across it. */
IST_API int64_t ist_debug_jpeg_join_launches(void);

/* ---- overlap removal for scrolled screenshots --------------------------------------------------------------------------------
 * A vertical strip of screenshots repeats a bar at the top and at the bottom of every shot, and the content of each shot overlaps
 * the shot above it by an unknown number of rows.  Per neighbouring pair (A above, B below) the library finds the shared header H,
 * the shared footer F and the overlap K, and ist_overlap_rows says which rows of every image to keep.  THE CONTRACT (restated in
 * numpy by tests/overlap_reference.py; the GPU agrees with it exactly).  Bitmaps are RGBA8, alpha is not read, all arithmetic is
 * integer, sums are 64-bit, and no result depends on the order of a sum.
 *   Signature.  For an image of width w, row y and cell c in [0, 32):  S(y, c) = sum of R + 2 G + B over the pixels x with
 *     e(c) <= x < e(c + 1), e(c) = floor(c w / 32).  A cell may be empty (w < 32).  S fits in uint32.
 *     D(p, q) = sum over c of |S(p, c) - S(q, c)| for two rows;  T = tolerance * w.
 *     (Cell sums, not hashes: independent per-pixel noise grows like the square root of a cell's pixels while T grows like w, and a
 *     scroll indicator touches one cell.)
 *   Pair.  Widths differ: {0, 0, 0, 0}.  Otherwise hm = min(hA, hB), L = floor(hm / 2).
 *     Header H: m(y) = [D(A row y, B row y) <= T] for y < L; H = the greatest t in [1, L] with m(t - 1) true and
 *       #{y < t : not m(y)} <= floor(t / 4), else 0.  (The quarter lets a changed clock inside the bar pass.)
 *     Footer F: the same rule on rows counted from the bottom: row hA - 1 - y of A against row hB - 1 - y of B.
 *     Bodies: A rows [H, hA - F), B rows [H, hB - F), bodyA and bodyB rows; kmax = min(bodyA, bodyB - 1): the lower image always keeps
 *       a row of its own.
 *     Informative rows: row r of B's body (0 <= r < bodyB - 1) is informative iff D(B row H + r, B row H + r + 1) > T;
 *       inf(k) = #{informative r : r < min(k, bodyB - 1)}.
 *     cost(k) = sum over r < k of D(A row hA - F - k + r, B row H + r).
 *     Candidates: k in [min_rows, kmax] with cost(k) <= T k and inf(k) >= min_informative.
 *     Choice: k1 beats k2 iff cost(k1) k2 < cost(k2) k1 (the least mean row cost, cross-multiplied); an exact tie goes to the SMALLER
 *       k (when in doubt, keep pixels).  No candidate: K = 0.  H and F are reported even then.
 *   The defaults (tolerance 8 = two 8-bit levels per pixel in the units of S, min_rows 16, min_informative 8) are contract defaults,
 *   not measured optima.  Not handled: periodic content (a list of identical items is ambiguous by nature); content that changes
 *   inside the overlap between two shots raises the cost and may give K = 0; horizontal strips; sub-row alignment. */
typedef struct ist_overlap_opts { int32_t tolerance, min_rows, min_informative, reserved; } ist_overlap_opts;
typedef struct ist_overlap { int32_t header, footer, overlap, reserved; int64_t cost; } ist_overlap;
/* The three host rules, pure CPU.  IST_E_INVALID for a NULL pointer, a negative count or a negative option.
 * edge: d[0 .. n) = D of the row pairs counted from the edge, *t = H (or F) as above with L = n. */
IST_API int ist_overlap_edge(const int64_t* d, int n, int64_t T, int32_t* t);
/* select: cost[0 .. kmax], inf[0 .. kmax] (inf[k] = inf(k) above), *k = K.  opts NULL: the defaults. */
IST_API int ist_overlap_select(const int64_t* cost, const int32_t* inf, int kmax, int64_t T, const ist_overlap_opts* opts, int32_t* k);
/* the crop rule: image i of n (pairs[0 .. n - 1), heights[0 .. n)) keeps rows [top[i], bot[i]).  top[0] = 0, bot[n - 1] = heights[n - 1];
 * a pair with overlap > 0 gives top[i + 1] = header + overlap and bot[i] = heights[i] - footer (the shared header and the overlap leave
 * the lower image, the shared footer the upper one); a pair with overlap 0 crops nothing.  Then for i = 1 .. n - 2 in order: an image
 * left with less than one row voids pair i (bot[i] = heights[i], top[i + 1] = 0).  n < 1: IST_E_INVALID. */
IST_API int ist_overlap_rows(const ist_overlap* pairs, const int32_t* heights, int n, int32_t* top, int32_t* bot);
/* out[i] = the pair (bitmap i, bitmap i + 1), i < n - 1.  Three launches (signatures of all images; edge differences of all pairs;
 * costs and informative flags of all pairs) on the context's stream, which is synchronised twice: the host runs the edge rule between
 * the second and the third launch, and the selection after the third.  Scratch is the context's, grow-only: a repeated shape allocates
 * nothing.  Refused before anything is enqueued: n < 2 or a NULL table IST_E_INVALID; a NULL entry IST_E_DECODE; a bitmap of another
 * device than the context's IST_E_INVALID; a bitmap with EXIF orientation > 1, or decoded at a reduced scale, IST_E_UNSUPPORTED
 * ("image k: ..."); more than 128 images IST_E_UNSUPPORTED. */
IST_API int ist_bitmaps_overlap(ist_ctx* ctx, ist_bitmap* const* bitmaps, int n, const ist_overlap_opts* opts, ist_overlap* out);
/* the same for images in caller-owned device memory (image k: bitmap_w x bitmap_h of descs[k] at src[k], rows pitch[k] bytes apart,
 * 4-byte aligned).  The caller's writes to the images must have completed; the call returns with the results in host memory. */
IST_API int ist_overlap_device(ist_ctx* ctx, const void* const* src, const size_t* pitch, const ist_image_desc* descs, int n,
                               const ist_overlap_opts* opts, ist_overlap* out);
/* kernel launches made by the two calls above in this process so far (3 per call) */
IST_API int64_t ist_debug_overlap_launches(void);
/* the signature table of the context's LAST overlap call: `rows` rows (the images' rows in image order) of 32 uint32 each into out */
IST_API int ist_debug_overlap_signatures(ist_ctx* ctx, uint32_t* out, int64_t rows);
/* A bitmap that is rows [y0, y0 + rows) of another: it shares the parent's block and holds a reference on the parent, copies nothing,
 * and its row 0 is the parent's row y0.  Its desc is the parent's with `rows` as the height and file_size 0; ist_debug_bitmap_bytes
 * does not count it; every call that takes a bitmap takes a view.  Either may be released first: the block goes with its last
 * holder.  NULL on failure: IST_E_INVALID for a NULL bitmap or rows outside it, IST_E_UNSUPPORTED for a bitmap with EXIF orientation
 * > 1 or decoded at a reduced scale. */
IST_API ist_bitmap* ist_bitmap_rows(ist_bitmap* b, int32_t y0, int32_t rows);

/* ---- colour profiles: ICC-tagged files converted to sRGB on decode -----------------------------------------------------------
 * A file may carry an ICC profile that says what its RGB code values mean (Display P3 for phone photos, Adobe RGB for many exports);
 * exports are untagged, so a viewer reads them as sRGB.  With IST_COLOR_PROFILE_SRGB on a context, every bitmap the file decoders of
 * that context leave in device memory is converted to sRGB in place, by one launch behind its decode on the same stream.  The default
 * is IST_COLOR_PROFILE_IGNORE: every call does exactly what it did before this setting existed.  Relative colorimetric, clipping, no
 * black-point compensation.  Alpha is copied; straight-alpha colour values are converted whatever the alpha is.
 * THE CONTRACT (restated in numpy by tests/icc_reference.py; the GPU agrees with it byte for byte).  All integer; '>>' is an
 * arithmetic shift of a 64-bit value, '/' and '%' on non-negative integers.
 *   Where the profile is read.  JPEG: the APP2 segments in front of the first scan that begin "ICC_PROFILE\0", seq (from 1), count,
 *     joined in seq order; a missing chunk, a seq used twice, chunks that disagree on count, seq 0 or seq > count: no profile.  PNG: iCCP
 *     (name, NUL, method 0, a zlib stream of at most 4 MiB inflated) in front of the first IDAT; else an sRGB chunk means IDENTITY; gAMA /
 *     cHRM / cICP alone: no profile.  WebP: the ICCP chunk of a file with a VP8X chunk.  BMP, GIF: none.  A damaged profile never fails a
 *     decode.
 *   Which profiles are taken (everything else is IST_COLOR_UNSUPPORTED and the pixels stay as decoded).  The header's size field is
 *     >= 132 and <= the bytes given, and bounds everything; 'acsp' at byte 36; data colour space 'RGB ', PCS 'XYZ '; the tag table lies
 *     inside; the FIRST tag of each of rXYZ, gXYZ, bXYZ (type 'XYZ ', three s15Fixed16) and rTRC, gTRC, bTRC is used and lies inside with
 *     its whole body.  A TRC is 'curv' (count 0: identity; count 1: a u8Fixed8 gamma > 0; count n >= 2: n u16 entries) or 'para' with
 *     function type 0 .. 4 (parameters s15Fixed16, read as int / 65536.0; g > 0; a != 0 for types 1 and 2).  Matrix/TRC tags are used
 *     even when A2B0 is present; wtpt and chad are not read (the colorants are PCS-relative).  A matrix entry outside int32:
 *     UNSUPPORTED.
 *   dec[c][v], c = r, g, b, v = 0 .. 255, uint16.  A function f: clamp(floor(65535 f(v / 255.0) + 0.5), 0, 65535), f in IEEE double,
 *     powers by the C library's pow, B = max(a x + b, 0):
 *       gamma and para 0: x^g        para 1: x >= -b / a ? B^g : 0        para 2: x >= -b / a ? B^g + c : c
 *       para 3: x >= d ? B^g : c x   para 4: x >= d ? B^g + e : c x + f
 *     curv count 0: 257 v.  A table t[0 .. n-1]: p = v (n - 1), i = p / 255, r = p % 255,
 *       dec = (t[i] (255 - r) + t[min(i + 1, n - 1)] r + 127) / 255.
 *   Mq (Q16) = (INV C + 2^23) >> 24; C = the colorants as s15.16 integers, rows X, Y, Z, columns r, g, b; INV = the inverse of the sRGB
 *     colorants (D50) in Q24:  {{52584397, -27133356, -8233164}, {-16421465, 32147857, 561266}, {1207600, -3841813, 23584544}}
 *     (the sRGB colorants {{28576, 25239, 9375}, {14581, 46983, 3972}, {912, 6361, 46787}} give 65536 I exactly).
 *   Per pixel: lin_j = dec[j][v_j];  o_i = clamp((sum_j Mq[i][j] lin_j + 2^15) >> 16, 0, 65535);  the output code of channel i is the
 *     number of c in 1 .. 255 with T[c] <= o_i, T[c] = ceil(65535 s((c - 0.5) / 255)), s(x) = x <= 0.04045 ? x / 12.92 :
 *     ((x + 0.055) / 1.055)^2.4 - a fixed table, carried as a literal (csrc/ist_icc.h; tools/gen_icc_encode_table.py).
 *   Kinds: NONE (no profile); IDENTITY (Mq == 65536 I and every code of every channel maps to itself: nothing is launched); CONVERT;
 *     UNSUPPORTED. */
enum { IST_COLOR_PROFILE_IGNORE = 0, IST_COLOR_PROFILE_SRGB = 1 };
enum { IST_COLOR_NONE = 0, IST_COLOR_IDENTITY = 1, IST_COLOR_CONVERT = 2, IST_COLOR_UNSUPPORTED = 3 };
typedef struct ist_color_tables {
  int32_t kind;               /* IST_COLOR_* */
  int32_t mq[3][3];           /* Q16; rows = output r, g, b */
  uint16_t dec[3][256];
} ist_color_tables;
/* The setting of a context, read by ist_bitmaps_decode[_scaled], ist_decode_files_device[_scaled], ist_stitch_files_png /
 * ist_stitch_paths_png (+ _preview; an image reconstructed straight into its box of the canvas is converted there) and by the JPEG
 * branch of ist_image_decode_rgba8[_scaled] / ist_jpeg_decode_rgba8, whose pixels pass through device memory.  PNG, WebP, BMP and GIF
 * files of ist_image_decode_rgba8 are decoded on the host into the caller's buffer and never reach the device: they are NOT converted
 * there (decode them with ist_bitmaps_decode or ist_decode_files_device).  ist_bitmap_upload and raw host pixels are never converted.
 * IST_E_NO_CONTEXT for a NULL context, IST_E_INVALID for any other value. */
IST_API int ist_ctx_set_color_profile(ist_ctx* ctx, int profile);
/* *kind = the IST_COLOR_* of a file (by signature: JPEG, PNG, WebP; anything else NONE).  Host only, no context.  IST_E_INVALID: a
 * NULL argument or len <= 0. */
IST_API int ist_image_color(const uint8_t* file, int64_t len, int32_t* kind);
/* an ICC profile -> out->kind and, for CONVERT and IDENTITY, dec and mq (zeroed otherwise).  Host only.  Returns the kind;
 * IST_E_INVALID for a NULL argument or len <= 0. */
IST_API int ist_icc_tables(const uint8_t* icc, int64_t len, ist_color_tables* out);
/* the conversion on caller-owned device memory: the w x h box of RGBA8 at ptr (4-byte aligned; rows pitch bytes apart, a multiple of 4
 * that is >= 4 w), in place, asynchronous on `stream` (hipStream_t, NULL = default stream); no byte outside the box is written.  The
 * tables travel by value with the launch.  IDENTITY tables launch nothing.  IST_E_NO_CONTEXT; IST_E_INVALID: NULL ptr or tables,
 * w or h < 1, a short or unaligned pitch, an unaligned ptr, tables whose kind is neither CONVERT nor IDENTITY. */
IST_API int ist_color_convert_device(ist_ctx* ctx, void* ptr, size_t pitch, int64_t w, int64_t h, const ist_color_tables* tables, void* stream);
/* launches of the conversion kernel in this process so far */
IST_API int64_t ist_debug_color_launches(void);

#ifdef __cplusplus
}
#endif
#endif /* IMAGESTITCH_H_ */
