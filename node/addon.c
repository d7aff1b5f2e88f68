/*
 * addon.c — thin N-API binding of the C-ABI (include/imagestitch.h) for the TypeScript/Node host.
 *
 * The reference is JavaScript calling the platform Canvas (miniprogram-stitch/miniprogram/pages/index/index.js:1186,
 * utils/canvas.js); this addon is what a maintainer would require() in its place.  No pixel arithmetic here: every
 * function marshals arguments and calls libimagestitch.so.
 *
 *   plan(images, direction, mode, gap, limits)                         -> plan object        (pure CPU)
 *   stitch(images, direction, mode, gap, limits, filter, asPng?, devices?, split?) -> Promise<{width,height,data}>  (napi_async_work)
 *       devices: number[] (devices[0] = root) shards the stitch over several GPUs from this process (ist_stitch_rgba8_multi:
 *       RCCL gather over xGMI); split 0 = by image (round robin), 1 = by band (equal output rows, draw by draw), 2 = by rows (across all draws), 3 = auto
 *   stitchSync(...same...)                                             -> {width,height,data}
 *   stitchBatch(requests) / stitchBatchSync(requests): requests[k] = [images, direction, mode, gap, limits, filter]
 *       -> Promise<({width,height,data,plan} | null)[]> / the array itself  (ist_stitch_rgba8_batch: one GPU, many stitches)
 *   stitchPngBatch(requests) / stitchPngBatchSync(requests): the same requests
 *       -> Promise<({width,height,png,plan} | null)[]> / the array itself  (ist_stitch_png_batch: one GPU, many PNG files)
 *   stitchJpegBatch(requests) / stitchJpegBatchSync(requests): requests[k] = [..., quality, subsampling]
 *       -> Promise<({width,height,jpeg,plan} | null)[]> / the array itself  (ist_stitch_jpeg_batch: one GPU, many JPEG files)
 *   stitchFiles(files: Buffer[], direction, mode, gap, limits, filter, previewWidth?, previewHeight?) -> Promise<{width,height,png,plan}>
 *   render(canvasW, canvasH, clearRGBA, ops, images, filter, region, asPng?) -> Buffer (region pixels, or the PNG file)
 *   encodePng(data, width, height) -> Buffer;  stitch(..., filter, true) resolves {width,height,png}
 *   encodeJpeg(data, width, height, quality, subsampling) -> Buffer;  stitch / stitchBitmaps(..., filter, {quality, subsampling})
 *       resolve {width,height,jpeg} (ist_stitch_jpeg / ist_stitch_bitmaps_jpeg: asPng given as an object is the JPEG export)
 *   joinJpegCheck(files: Buffer[], direction) -> {ok, reason, image, width, height, subsampling} (ist_jpeg_join_check: pure CPU);
 *   joinJpeg(files: Buffer[], direction, flags?) -> Promise<Buffer> (ist_jpeg_join_files: the lossless join; flags 0 or IST_JPEG_OPTIMIZE)
 *   deviceCount(), lastError(), abiVersion()
 *   resident bitmaps (ist_bitmap_*): uploadBitmap([image]) -> handle;  decodeBitmaps(files: Buffer[], scales?: number[], colorProfile?: number) -> Promise<handle[]>;
 *   imageColor(file: Buffer) -> 0 .. 3 (IST_COLOR_*);
 *     decodeScaleFit(width, height, minWidth, minHeight) -> 1 | 2 | 4 | 8;
 *   bitmapDesc(h) -> {width,height,orientation,bmpWidth,bmpHeight,opaque,fileSize};  bitmapDownload(h) -> Buffer;  bitmapRelease(h);
 *   stitchBitmaps(handles, direction, mode, gap, limits, filter, asPng) -> Promise (as stitch);  stitchBitmapsSync(...same...);
 *   debugBitmapBytes();  bitmapRows(h, y0, rows) -> handle of a row view (ist_bitmap_rows);
 *   findOverlaps(handles, tolerance, minRows, minInformative) -> Promise<[{header, footer, overlap, cost}]>, findOverlapsSync(...same...)
 *   (ist_bitmaps_overlap), overlapRows(pairs, heights) -> [[top, bot]] (ist_overlap_rows).  A handle is an object that wraps ONE reference of a bitmap: bitmapRelease drops it (again: nothing), its
 *   finaliser drops it when the handle is collected unreleased; a stitch holds a reference of its own from the call to its completion.
 *
 * images[i] = {width, height, orientation?, fileSize?, opaque?, bmpWidth?, bmpHeight?, data?: Uint8Array|Buffer}
 * limits    = {platform: 0|1|2, maxSide, maxPixels, superSample} or null (MI355X default: caps lifted, superSample 1)
 * ops       = Float64Array, 18 doubles per op: kind, image, m[6], s[4], d[4], r|g<<8|b<<16|a<<24, reserved
 *
 * Caller bytes (pixels, files) are a Uint8Array, a Uint8ClampedArray or a Buffer and nothing else: bytes_of() is the one reader, and
 * every site answers anything else with a TypeError.  Every entry marshals ALL of its arguments before it asks for the context, so
 * a malformed call fails the same way with and without a device.  An image that a stitch or an upload needs and that came without
 * `data` is the decode failure (-6 '图片N解码异常'), decided at marshalling too.
 *
 * Every asynchronous entry is a job (below): a header, and per kind the library call, the JS result and the free.  job_queue runs
 * one as a Promise on the libuv pool, job_now runs its synchronous twin on the JS thread.
 */
#define NODE_GYP_MODULE_NAME imagestitch
#include <node_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/imagestitch.h"

static ist_ctx* g_ctx = NULL;

static pthread_once_t g_ctx_once = PTHREAD_ONCE_INIT;
static char g_ctx_err[256];
static void make_ctx(void) {
  g_ctx = ist_ctx_create(0);
  if (!g_ctx) snprintf(g_ctx_err, sizeof g_ctx_err, "%s", ist_last_error());
}
/* one context for the process; NULL (with the reason in g_ctx_err) when there is no HIP device: no CPU fallback */
static ist_ctx* get_ctx(void) {
  pthread_once(&g_ctx_once, make_ctx);
  return g_ctx;
}

/* ---- errors -------------------------------------------------------------------------------------------------------------- */
/* Error('拼图失败：' + why), code = the C-ABI code: the same shape as the reference's toast (index.js:1620) */
static napi_value make_error(napi_env env, int code, const char* why) {
  char msg[512], codebuf[16];
  snprintf(msg, sizeof msg, "\xe6\x8b\xbc\xe5\x9b\xbe\xe5\xa4\xb1\xe8\xb4\xa5\xef\xbc\x9a%s", why && *why ? why : "unknown");
  snprintf(codebuf, sizeof codebuf, "%d", code);
  napi_value m, c, e;
  napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &m);
  napi_create_string_utf8(env, codebuf, NAPI_AUTO_LENGTH, &c);
  napi_create_error(env, c, m, &e);
  return e;
}
static napi_value throw_code(napi_env env, int code, const char* why) { napi_throw(env, make_error(env, code, why)); return NULL; }
static napi_value throw_ist(napi_env env, int code) { return throw_code(env, code, ist_last_error()); }
static napi_value throw_type(napi_env env, const char* msg) { napi_throw_type_error(env, NULL, msg); return NULL; }
static napi_value throw_oom(napi_env env) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
/* the context of a synchronous entry; NULL with the -5 error pending when there is no device */
static ist_ctx* ctx_or_throw(napi_env env) {
  ist_ctx* ctx = get_ctx();
  if (!ctx) throw_code(env, IST_E_NO_DEVICE, g_ctx_err);
  return ctx;
}

/* ---- reading what the caller brings -------------------------------------------------------------------------------------- */
/* the call's arguments, up to cap of them (those not given read as undefined); 0 with TypeError(usage) pending below `need` */
/* The colour setting is the context's (ist_ctx_set_color_profile), and jobs run on pool threads: a call that decodes files holds this
 * lock from setting its own value to the end of its library call, and leaves IST_COLOR_PROFILE_IGNORE behind - so no call ever sees
 * another call's value, and every entry point without the option does what it always did. */
static pthread_mutex_t g_color_mu = PTHREAD_MUTEX_INITIALIZER;
static void color_begin(ist_ctx* ctx, int profile) { pthread_mutex_lock(&g_color_mu); if (ctx) ist_ctx_set_color_profile(ctx, profile); }
static void color_end(ist_ctx* ctx) { if (ctx) ist_ctx_set_color_profile(ctx, IST_COLOR_PROFILE_IGNORE); pthread_mutex_unlock(&g_color_mu); }

static int args_of(napi_env env, napi_callback_info info, size_t need, size_t cap, napi_value* argv, const char* usage) {
  size_t argc = cap;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) == napi_ok && argc >= need) return 1;
  napi_throw_type_error(env, NULL, usage);
  return 0;
}
static int int_of(napi_env env, napi_value v, int otherwise) {
  int32_t x;
  return napi_get_value_int32(env, v, &x) == napi_ok ? x : otherwise;
}
static double num_of(napi_env env, napi_value v, double otherwise) {
  double x;
  return napi_get_value_double(env, v, &x) == napi_ok ? x : otherwise;
}
static int bool_of(napi_env env, napi_value v, int otherwise) {
  bool b;
  return napi_get_value_bool(env, v, &b) == napi_ok ? b : otherwise;
}
static napi_valuetype type_of(napi_env env, napi_value v) {
  napi_valuetype t = napi_undefined;
  napi_typeof(env, v, &t);
  return t;
}
static int is_nullish(napi_env env, napi_value v) {
  const napi_valuetype t = type_of(env, v);
  return t == napi_null || t == napi_undefined;
}
static int array_len(napi_env env, napi_value v, uint32_t* n) {
  bool is_arr = false;
  return napi_is_array(env, v, &is_arr) == napi_ok && is_arr && napi_get_array_length(env, v, n) == napi_ok;
}
static napi_value undefined_of(napi_env env) { napi_value u; napi_get_undefined(env, &u); return u; }
static napi_value null_of(napi_env env) { napi_value u; napi_get_null(env, &u); return u; }

/* a typed array's element type, address and length in elements; 0 for anything else */
static int typed_of(napi_env env, napi_value v, napi_typedarray_type* tt, void** p, size_t* len) {
  bool ta = false; napi_value ab; size_t off;
  *p = NULL; *len = 0;
  return napi_is_typedarray(env, v, &ta) == napi_ok && ta && napi_get_typedarray_info(env, v, tt, len, p, &ab, &off) == napi_ok;
}
/* THE reader of caller bytes: 1 for a Uint8Array / Uint8ClampedArray (a Buffer is a Uint8Array), 0 for everything else - other typed
 * arrays, DataView, strings, null, plain objects.  Judged by the element type, never by napi_is_buffer, which is true of every
 * ArrayBufferView.  Nothing is thrown here: each site words its own TypeError.  An empty array is zero bytes at a valid address. */
static int bytes_of(napi_env env, napi_value v, const uint8_t** p, size_t* len) {
  static const uint8_t nothing[1] = {0};
  napi_typedarray_type tt; void* d;
  if (!typed_of(env, v, &tt, &d, len) || (tt != napi_uint8_array && tt != napi_uint8_clamped_array)) { *p = NULL; *len = 0; return 0; }
  *p = d ? (const uint8_t*)d : nothing;
  return 1;
}

static int get_named_f64(napi_env env, napi_value obj, const char* key, double* out) {
  napi_value v;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok || type_of(env, v) != napi_number) return 0;
  return napi_get_value_double(env, v, out) == napi_ok;
}
static int get_named_i64(napi_env env, napi_value obj, const char* key, int64_t* out) {
  double d;
  if (!get_named_f64(env, obj, key, &d)) return 0;
  *out = (int64_t)d;
  return 1;
}
static int get_named_bool(napi_env env, napi_value obj, const char* key) {
  napi_value v;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return 0;
  return type_of(env, v) == napi_number ? num_of(env, v, 0) != 0 : bool_of(env, v, 0);
}

typedef struct {
  int n;
  ist_image_desc* descs;
  const uint8_t** data;    /* NULL: the image came without pixels */
  size_t* pitch;
  napi_ref* refs;          /* keeps the JS buffers alive while async work runs */
} images_t;

static void images_free(napi_env env, images_t* im) {
  if (im->refs) for (int i = 0; i < im->n; i++) if (im->refs[i]) napi_delete_reference(env, im->refs[i]);
  free(im->descs); free(im->data); free(im->pitch); free(im->refs);
  memset(im, 0, sizeof *im);
}

/* 0 on failure: the exception is pending and *im is empty again */
static int images_parse(napi_env env, napi_value arr, images_t* im, int want_refs) {
  uint32_t n = 0;
  memset(im, 0, sizeof *im);
  if (!array_len(env, arr, &n)) { napi_throw_type_error(env, NULL, "images must be an array"); return 0; }
  im->n = (int)n;
  im->descs = (ist_image_desc*)calloc(n ? n : 1, sizeof(ist_image_desc));
  im->data = (const uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*));
  im->pitch = (size_t*)calloc(n ? n : 1, sizeof(size_t));
  im->refs = want_refs ? (napi_ref*)calloc(n ? n : 1, sizeof(napi_ref)) : NULL;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e, d; int64_t v; size_t len;
    napi_get_element(env, arr, i, &e);
    if (type_of(env, e) != napi_object) { napi_throw_type_error(env, NULL, "images[i] must be an object"); goto fail; }
    ist_image_desc* D = &im->descs[i];
    if (get_named_i64(env, e, "width", &v)) D->width = (int32_t)v;
    if (get_named_i64(env, e, "height", &v)) D->height = (int32_t)v;
    D->orientation = 1;
    if (get_named_i64(env, e, "orientation", &v)) D->orientation = (int32_t)v;
    if (get_named_i64(env, e, "bmpWidth", &v)) D->bmp_width = (int32_t)v;
    if (get_named_i64(env, e, "bmpHeight", &v)) D->bmp_height = (int32_t)v;
    if (get_named_i64(env, e, "fileSize", &v)) D->file_size = v;
    D->opaque = get_named_bool(env, e, "opaque");
    if (napi_get_named_property(env, e, "data", &d) != napi_ok || is_nullish(env, d)) continue;   /* no pixels: fine for a plan, see images_missing */
    if (!bytes_of(env, d, &im->data[i], &len)) { napi_throw_type_error(env, NULL, "image data must be a Uint8Array / Buffer"); goto fail; }
    const int64_t bw = D->bmp_width > 0 ? D->bmp_width : D->width, bh = D->bmp_height > 0 ? D->bmp_height : D->height;
    if (bw > 0 && bh > 0 && (int64_t)len < bw * bh * 4) { napi_throw_range_error(env, NULL, "image data is smaller than width*height*4"); goto fail; }
    im->pitch[i] = (size_t)bw * 4;
    if (want_refs) napi_create_reference(env, d, 1, &im->refs[i]);
  }
  return 1;
fail:
  images_free(env, im);
  return 0;
}

/* an image without pixels where a stitch or an upload needs them: 1 with the decode failure's reason in err ('图片N解码异常' like
 * index.js:1513, 'request k: ' in front for request k >= 0 of a batch); 0 when every image has its pixels */
static int images_missing(const images_t* im, int request, char* err, size_t cap) {
  for (int i = 0; i < im->n; i++) {
    if (im->data[i]) continue;
    const int at = request >= 0 ? snprintf(err, cap, "request %d: ", request) : 0;
    snprintf(err + at, cap - (size_t)at, "\xe5\x9b\xbe\xe7\x89\x87%d\xe8\xa7\xa3\xe7\xa0\x81\xe5\xbc\x82\xe5\xb8\xb8", i);
    return 1;
  }
  return 0;
}

static void limits_parse(napi_env env, napi_value v, ist_limits* lim) {
  ist_limits_unlimited(lim);
  if (type_of(env, v) != napi_object) return;
  int64_t plat = -1; double d;
  if (get_named_i64(env, v, "platform", &plat) && plat >= 0) ist_limits_default((int)plat, lim);
  if (get_named_f64(env, v, "maxSide", &d)) lim->max_side = d;
  if (get_named_f64(env, v, "maxPixels", &d)) lim->max_pixels = d;
  if (get_named_f64(env, v, "superSample", &d)) lim->max_super_sample = d;
}

/* the (direction, mode, gap, limits, filter) run that follows the sources of every stitch call: a[0..4] */
typedef struct { int direction, mode, filter; double gap; ist_limits lim; } strip_t;
#define STRIP_ARGS(s) (s)->direction, (s)->mode, (s)->gap, &(s)->lim, (s)->filter      /* the same run, as the C-ABI takes it */
static void strip_parse(napi_env env, const napi_value* a, strip_t* s) {
  s->direction = int_of(env, a[0], 0);
  s->mode = int_of(env, a[1], 0);
  s->gap = num_of(env, a[2], 0);
  limits_parse(env, a[3], &s->lim);
  s->filter = int_of(env, a[4], 0);
}

/* a list of files: their bytes, each Buffer referenced until files_free */
typedef struct { int n; const uint8_t** ptr; int64_t* len; napi_ref* refs; } files_t;

static void files_free(napi_env env, files_t* f) {
  if (f->refs) for (int i = 0; i < f->n; i++) if (f->refs[i]) napi_delete_reference(env, f->refs[i]);
  free(f->ptr); free(f->len); free(f->refs);
  memset(f, 0, sizeof *f);
}
/* 0 on failure: a TypeError is pending (not_array when v is no array) and *f is empty again */
static int files_parse(napi_env env, napi_value v, const char* not_array, files_t* f) {
  uint32_t n = 0;
  memset(f, 0, sizeof *f);
  if (!array_len(env, v, &n)) { napi_throw_type_error(env, NULL, not_array); return 0; }
  f->n = (int)n;
  f->ptr = (const uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*)); f->len = (int64_t*)calloc(n ? n : 1, sizeof(int64_t)); f->refs = (napi_ref*)calloc(n ? n : 1, sizeof(napi_ref));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e; size_t len;
    napi_get_element(env, v, i, &e);
    if (!bytes_of(env, e, &f->ptr[i], &len)) { napi_throw_type_error(env, NULL, "files[i] must be a Buffer / Uint8Array"); files_free(env, f); return 0; }
    f->len[i] = (int64_t)len;
    napi_create_reference(env, e, 1, &f->refs[i]);
  }
  return 1;
}

/* ---- what goes back ------------------------------------------------------------------------------------------------------- */
static void set_num(napi_env env, napi_value obj, const char* key, double v) {
  napi_value n; napi_create_double(env, v, &n); napi_set_named_property(env, obj, key, n);
}
static void set_bool(napi_env env, napi_value obj, const char* key, int v) {
  napi_value b; napi_get_boolean(env, v != 0, &b); napi_set_named_property(env, obj, key, b);
}

static napi_value plan_to_js(napi_env env, const ist_plan* p) {
  napi_value o, rects;
  napi_create_object(env, &o);
  set_num(env, o, "outW", p->out_w); set_num(env, o, "outH", p->out_h);
  set_num(env, o, "scaleDown", p->scale_down); set_num(env, o, "superSample", p->super_sample);
  set_num(env, o, "canvasW", (double)p->canvas_w); set_num(env, o, "canvasH", (double)p->canvas_h);
  set_bool(env, o, "bigTask", p->big_task);
  napi_create_array_with_length(env, (size_t)p->n_rects, &rects);
  for (int i = 0; i < p->n_rects; i++) {
    napi_value r; napi_create_object(env, &r);
    set_num(env, r, "image", p->rects[i].image); set_num(env, r, "orientation", p->rects[i].orientation);
    set_num(env, r, "dx", p->rects[i].dx); set_num(env, r, "dy", p->rects[i].dy);
    set_num(env, r, "dw", p->rects[i].dw); set_num(env, r, "dh", p->rects[i].dh);
    napi_set_element(env, rects, (uint32_t)i, r);
  }
  napi_set_named_property(env, o, "rects", rects);
  return o;
}

static void free_block(napi_env env, void* data, void* hint) { (void)env; (void)hint; ist_free(data); }
/* a block of the library moves into a Buffer that gives it back (ist_free) when it is collected; NULL, the block freed, when it cannot */
static napi_value block_to_buffer(napi_env env, void* block, size_t bytes) {
  napi_value buf;
  if (napi_create_external_buffer(env, bytes, block, free_block, NULL, &buf) == napi_ok) return buf;
  ist_free(block);
  return NULL;
}
/* the same for an entry that returns the file itself: the Buffer, or NULL with an Error pending */
static napi_value file_to_js(napi_env env, uint8_t* file, int64_t len) {
  napi_value buf = block_to_buffer(env, file, (size_t)len);
  return buf ? buf : throw_oom(env);
}

/* {width, height, data}: previews, thumbnails, decoded files */
static napi_value pixels_to_js(napi_env env, double width, double height, napi_value data) {
  napi_value o;
  napi_create_object(env, &o);
  set_num(env, o, "width", width);
  set_num(env, o, "height", height);
  napi_set_named_property(env, o, "data", data);
  return o;
}

typedef enum { OUT_PIXELS, OUT_PNG, OUT_JPEG } out_kind;    /* what a stitch hands back: the canvas, or its file */

/* {width, height, data | png | jpeg, plan, preview?} of one stitched canvas.  Takes over *block (file_len bytes of a file, the
 * canvas itself for OUT_PIXELS) and, when pv is given, pv->pixels; frees the plan.  NULL when the block cannot be wrapped: nothing
 * of the request is left allocated either way. */
static napi_value export_to_js(napi_env env, out_kind out, ist_plan* plan, uint8_t** block, int64_t file_len, ist_preview* pv) {
  static const char* const KEY[] = {"data", "png", "jpeg"};
  napi_value o;
  napi_value buf = block_to_buffer(env, *block, out == OUT_PIXELS ? (size_t)plan->canvas_w * (size_t)plan->canvas_h * 4 : (size_t)file_len);
  *block = NULL;
  if (!buf || napi_create_object(env, &o) != napi_ok) o = NULL;
  else {
    set_num(env, o, "width", (double)plan->canvas_w);
    set_num(env, o, "height", (double)plan->canvas_h);
    napi_set_named_property(env, o, KEY[out], buf);
    if (pv && pv->pixels) {
      napi_value small = block_to_buffer(env, pv->pixels, (size_t)pv->width * (size_t)pv->height * 4);
      pv->pixels = NULL;
      if (small) napi_set_named_property(env, o, "preview", pixels_to_js(env, (double)pv->width, (double)pv->height, small));
    }
    napi_set_named_property(env, o, "plan", plan_to_js(env, plan));
  }
  if (pv && pv->pixels) { ist_free(pv->pixels); pv->pixels = NULL; }
  ist_plan_free(plan);
  return o;
}

/* ---- jobs ----------------------------------------------------------------------------------------------------------------- */
/* A job is what an entry made of its arguments (its struct begins with this header) plus three functions of its kind.  run() makes
 * the library call with the context, on a pool thread or - the Sync twin - on the JS thread; result() and free() run on the JS thread. */
typedef struct job job;
typedef struct {
  int (*run)(ist_ctx* ctx, job* j);               /* the library call: its return code */
  napi_value (*result)(napi_env env, job* j);     /* the value of a call that returned IST_OK; NULL when it could not be built */
  void (*free)(napi_env env, job* j);
} job_kind;
struct job {
  const job_kind* kind;
  int decided;                 /* marshalling settled the outcome (rc, err): nothing to run, no context asked for */
  int rc; char err[256];
  napi_deferred deferred; napi_async_work work;
};

static void job_run(job* j) {
  if (j->decided) return;
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  j->rc = j->kind->run(ctx, j);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());      /* (this thread's message) */
}
/* how a job that has run ends: 1 with its value (null for IST_NOTHING_TO_DO), 0 with its Error */
static int job_outcome(napi_env env, job* j, napi_value* out) {
  if (j->rc < 0) { *out = make_error(env, j->rc, j->err); return 0; }
  *out = j->rc == IST_NOTHING_TO_DO ? null_of(env) : j->kind->result(env, j);
  if (*out) return 1;
  *out = make_error(env, IST_E_NOMEM, "could not wrap the result");
  return 0;
}
static void job_execute(napi_env env, void* data) { (void)env; job_run((job*)data); }
static void job_complete(napi_env env, napi_status status, void* data) {
  job* j = (job*)data;
  napi_value v;
  (void)status;
  if (job_outcome(env, j, &v)) napi_resolve_deferred(env, j->deferred, v);
  else napi_reject_deferred(env, j->deferred, v);
  napi_delete_async_work(env, j->work);
  j->kind->free(env, j);
}
/* the Promise of a job, run on the libuv pool while the event loop keeps turning (the reference yields between images with
 * `await _sleep(0)`, index.js:1567).  j NULL: its parser has thrown.  The job is freed here when it cannot be queued. */
static napi_value job_queue(napi_env env, job* j, const char* name) {
  napi_value promise, res;
  if (!j) return NULL;
  if (napi_create_promise(env, &j->deferred, &promise) == napi_ok && napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &res) == napi_ok &&
      napi_create_async_work(env, NULL, res, job_execute, job_complete, j, &j->work) == napi_ok) {
    if (napi_queue_async_work(env, j->work) == napi_ok) return promise;
    napi_delete_async_work(env, j->work);
  }
  j->kind->free(env, j);
  napi_throw_error(env, NULL, "could not queue the work");
  return NULL;
}
/* the same job run here and now: its value, or NULL with its Error thrown */
static napi_value job_now(napi_env env, job* j) {
  napi_value v;
  if (!j) return NULL;
  job_run(j);
  if (!job_outcome(env, j, &v)) { napi_throw(env, v); v = NULL; }
  j->kind->free(env, j);
  return v;
}

/* ---- resident bitmaps: handles -------------------------------------------------------------------------------------------- */
typedef struct { ist_bitmap* b; } bitmap_ref;   /* NULL once released */

static void bitmap_finalize(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  bitmap_ref* r = (bitmap_ref*)data;
  if (r->b) ist_bitmap_release(r->b);
  free(r);
}

/* a new handle that takes over the caller's reference of b (released again when the handle cannot be made) */
static napi_value bitmap_wrap(napi_env env, ist_bitmap* b) {
  napi_value o;
  bitmap_ref* r = (bitmap_ref*)calloc(1, sizeof *r);
  if (!r || napi_create_object(env, &o) != napi_ok) { free(r); ist_bitmap_release(b); return NULL; }
  r->b = b;
  if (napi_wrap(env, o, r, bitmap_finalize, NULL, NULL) != napi_ok) { free(r); ist_bitmap_release(b); return NULL; }
  return o;
}

/* the record of a handle; NULL with a TypeError pending when v is none */
static bitmap_ref* bitmap_ref_of(napi_env env, napi_value v) {
  bitmap_ref* r = NULL;
  if (napi_unwrap(env, v, (void**)&r) != napi_ok || !r) { napi_throw_type_error(env, NULL, "not a Bitmap handle"); return NULL; }
  return r;
}
/* the bitmap of a handle; NULL with an Error pending when it has been released (use after release) */
static ist_bitmap* bitmap_of(napi_env env, napi_value v) {
  bitmap_ref* r = bitmap_ref_of(env, v);
  if (!r) return NULL;
  if (!r->b) { napi_throw_error(env, NULL, "the bitmap has been released"); return NULL; }
  return r->b;
}

/* a list of handles as the request's bitmaps, every one retained HERE, on the JS thread, so that a release() or a collection between
 * the call and the work's execution cannot free it; null / undefined entries stay NULL (a missing image: '图片N解码异常' from the
 * library).  bitmaps_free drops the references again. */
typedef struct { int n; ist_bitmap** b; } bitmaps_t;

static void bitmaps_free(bitmaps_t* bm) {
  for (int i = 0; i < bm->n; i++) if (bm->b[i]) ist_bitmap_release(bm->b[i]);
  free(bm->b);
  memset(bm, 0, sizeof *bm);
}
/* 0 on failure: the exception is pending (TypeError(usage) when v is no array) and *bm is empty again */
static int bitmaps_parse(napi_env env, napi_value v, const char* usage, bitmaps_t* bm) {
  uint32_t n = 0;
  memset(bm, 0, sizeof *bm);
  if (!array_len(env, v, &n)) { napi_throw_type_error(env, NULL, usage); return 0; }
  bm->n = (int)n;
  bm->b = (ist_bitmap**)calloc(n ? n : 1, sizeof(ist_bitmap*));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e;
    napi_get_element(env, v, i, &e);
    if (is_nullish(env, e)) continue;
    if (!(bm->b[i] = bitmap_of(env, e))) { bitmaps_free(bm); return 0; }
    ist_bitmap_retain(bm->b[i]);
  }
  return 1;
}

/* ---- plan ----------------------------------------------------------------------------------------------------------------- */
/* plan(images, direction, mode, gap, limits) */
static napi_value js_plan(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  images_t im; ist_limits lim; ist_plan p;
  if (!args_of(env, info, 4, 5, argv, "plan(images, direction, mode, gap, limits)")) return NULL;
  if (!images_parse(env, argv[0], &im, 0)) return NULL;
  limits_parse(env, argv[4], &lim);
  const int rc = ist_plan_compute(im.descs, im.n, int_of(env, argv[1], 0), int_of(env, argv[2], 0), num_of(env, argv[3], 0), &lim, &p);
  images_free(env, &im);
  if (rc < 0) return throw_ist(env, rc);
  if (rc == IST_NOTHING_TO_DO) return null_of(env);
  napi_value out = plan_to_js(env, &p);
  ist_plan_free(&p);
  return out;
}

/* ---- one stitch: host images, resident bitmaps or files in; the canvas, a PNG or a JPEG out --------------------------------- */
typedef struct {
  job h;
  enum { SRC_IMAGES, SRC_BITMAPS, SRC_FILES } src;
  images_t im; bitmaps_t bm; files_t files;
  strip_t s;
  out_kind out; int quality, subsampling; /* OUT_JPEG: {quality, subsampling} */
  int devices[64]; int ndev, split;       /* opts.devices / opts.split: ndev 0 = the process-wide single context */
  int profile;                            /* SRC_FILES: IST_COLOR_PROFILE_* of opts.colorProfile */
  int want_preview; ist_preview pv;       /* OUT_PNG with {preview: {width, height}}: the canvas shrunk to fit that box, beside the file */
  ist_plan plan; uint8_t* block; int64_t file_len;    /* the canvas, or file_len bytes of its file */
} stitch_job;

static int stitch_run(ist_ctx* ctx, job* h) {
  stitch_job* j = (stitch_job*)h;
  const strip_t* s = &j->s;
  const images_t* im = &j->im;
  ist_preview* pv = j->want_preview ? &j->pv : NULL;
  if (j->src == SRC_FILES) {
    color_begin(ctx, j->profile);
    const int rc = ist_stitch_files_png_preview(ctx, j->files.ptr, j->files.len, j->files.n, STRIP_ARGS(s), &j->plan, &j->block, &j->file_len, pv);
    color_end(ctx);
    return rc;
  }
  if (j->src == SRC_BITMAPS)
    return j->out == OUT_JPEG ? ist_stitch_bitmaps_jpeg(ctx, j->bm.b, j->bm.n, STRIP_ARGS(s), j->quality, j->subsampling, &j->plan, &j->block, &j->file_len)
         : j->out == OUT_PNG  ? ist_stitch_bitmaps_png_preview(ctx, j->bm.b, j->bm.n, STRIP_ARGS(s), &j->plan, &j->block, &j->file_len, pv)
                              : ist_stitch_bitmaps_rgba8(ctx, j->bm.b, j->bm.n, STRIP_ARGS(s), &j->plan, &j->block);
  if (j->out == OUT_JPEG) return ist_stitch_jpeg(ctx, im->descs, im->data, im->pitch, im->n, STRIP_ARGS(s), j->quality, j->subsampling, &j->plan, &j->block, &j->file_len);
  if (j->out == OUT_PNG) return ist_stitch_png_preview(ctx, im->descs, im->data, im->pitch, im->n, STRIP_ARGS(s), &j->plan, &j->block, &j->file_len, pv);
  if (j->ndev > 0) return ist_stitch_rgba8_multi(j->devices, j->ndev, im->descs, im->data, im->pitch, im->n, STRIP_ARGS(s), j->split, &j->plan, &j->block);
  return ist_stitch_rgba8(ctx, im->descs, im->data, im->pitch, im->n, STRIP_ARGS(s), &j->plan, &j->block);
}
static napi_value stitch_result(napi_env env, job* h) {
  stitch_job* j = (stitch_job*)h;
  return export_to_js(env, j->out, &j->plan, &j->block, j->file_len, j->want_preview ? &j->pv : NULL);
}
static void stitch_free(napi_env env, job* h) {
  stitch_job* j = (stitch_job*)h;
  images_free(env, &j->im); bitmaps_free(&j->bm); files_free(env, &j->files);
  free(j);
}
static const job_kind STITCH = {stitch_run, stitch_result, stitch_free};

/* the asPng argument of a native stitch call: true is the PNG export, an object {quality, subsampling: IST_JPEG_*} the JPEG export
 * (stitchJpeg) */
static void export_parse(napi_env env, napi_value as, stitch_job* j) {
  if (type_of(env, as) == napi_object) {
    napi_value q, s;
    j->out = OUT_JPEG; j->quality = 90; j->subsampling = IST_JPEG_420;
    if (napi_get_named_property(env, as, "quality", &q) == napi_ok) j->quality = int_of(env, q, j->quality);
    if (napi_get_named_property(env, as, "subsampling", &s) == napi_ok) j->subsampling = int_of(env, s, j->subsampling);
  } else if (bool_of(env, as, 0)) j->out = OUT_PNG;
}
/* the trailing (previewWidth, previewHeight) arguments of a PNG call: both numbers -> the preview is asked for, with that box */
static void preview_parse(napi_env env, napi_value w, napi_value h, stitch_job* j) {
  if (j->out != OUT_PNG || type_of(env, w) != napi_number || type_of(env, h) != napi_number) return;
  j->want_preview = 1;
  j->pv.box_w = num_of(env, w, 0); j->pv.box_h = num_of(env, h, 0);
}
static stitch_job* stitch_job_new(int src) {
  stitch_job* j = (stitch_job*)calloc(1, sizeof *j);
  j->h.kind = &STITCH; j->src = src;
  return j;
}

static job* stitch_parse(napi_env env, napi_callback_info info, int want_refs) {
  napi_value argv[11]; uint32_t n = 0;
  if (!args_of(env, info, 6, 11, argv, "stitch(images, direction, mode, gap, limits, filter, asPng, devices, split, previewWidth, previewHeight)")) return NULL;
  stitch_job* j = stitch_job_new(SRC_IMAGES);
  if (!images_parse(env, argv[0], &j->im, want_refs)) { stitch_free(env, &j->h); return NULL; }
  strip_parse(env, argv + 1, &j->s);
  export_parse(env, argv[6], j);
  preview_parse(env, argv[9], argv[10], j);
  if (array_len(env, argv[7], &n)) {                    /* devices: number[] */
    if (n > 64) { napi_throw_range_error(env, NULL, "devices: at most 64 entries"); stitch_free(env, &j->h); return NULL; }
    for (uint32_t i = 0; i < n; i++) { napi_value e; napi_get_element(env, argv[7], i, &e); j->devices[i] = int_of(env, e, -1); }
    j->ndev = (int)n;
  }
  j->split = int_of(env, argv[8], 0);
  if (images_missing(&j->im, -1, j->h.err, sizeof j->h.err)) { j->h.decided = 1; j->h.rc = IST_E_DECODE; }
  return &j->h;
}
static napi_value js_stitch(napi_env env, napi_callback_info info) { return job_queue(env, stitch_parse(env, info, 1), "imagestitch.stitch"); }
static napi_value js_stitch_sync(napi_env env, napi_callback_info info) { return job_now(env, stitch_parse(env, info, 0)); }

/* stitchBitmaps(handles, direction, mode, gap, limits, filter, asPng, previewWidth, previewHeight) */
static job* stitch_bitmaps_parse(napi_env env, napi_callback_info info) {
  static const char usage[] = "stitchBitmaps(bitmaps, direction, mode, gap, limits, filter, asPng, previewWidth, previewHeight)";
  napi_value argv[9];
  if (!args_of(env, info, 6, 9, argv, usage)) return NULL;
  stitch_job* j = stitch_job_new(SRC_BITMAPS);
  if (!bitmaps_parse(env, argv[0], usage, &j->bm)) { stitch_free(env, &j->h); return NULL; }
  strip_parse(env, argv + 1, &j->s);
  export_parse(env, argv[6], j);
  preview_parse(env, argv[7], argv[8], j);
  return &j->h;
}
static napi_value js_stitch_bitmaps(napi_env env, napi_callback_info info) { return job_queue(env, stitch_bitmaps_parse(env, info), "imagestitch.stitchBitmaps"); }
static napi_value js_stitch_bitmaps_sync(napi_env env, napi_callback_info info) { return job_now(env, stitch_bitmaps_parse(env, info)); }

/* stitchFiles(files: Buffer[], direction, mode, gap, limits, filter, previewWidth, previewHeight, colorProfile) -> Promise<{width,height,png,plan}>
 * the device-resident pipeline (ist_stitch_files_png): only file bytes go in, only PNG bytes come out.  colorProfile: IST_COLOR_PROFILE_*
 * (absent: ignore), set on the context for this call alone */
static napi_value js_stitch_files(napi_env env, napi_callback_info info) {
  napi_value argv[9];
  if (!args_of(env, info, 6, 9, argv, "stitchFiles(files, direction, mode, gap, limits, filter, previewWidth, previewHeight, colorProfile)")) return NULL;
  stitch_job* j = stitch_job_new(SRC_FILES);
  if (!files_parse(env, argv[0], "files must be an array of Buffers", &j->files)) { stitch_free(env, &j->h); return NULL; }
  strip_parse(env, argv + 1, &j->s);
  j->out = OUT_PNG;
  preview_parse(env, argv[6], argv[7], j);
  j->profile = int_of(env, argv[8], IST_COLOR_PROFILE_IGNORE);
  return job_queue(env, &j->h, "imagestitch.stitchFiles");
}

/* ---- batches --------------------------------------------------------------------------------------------------------------- */
/* stitchBatch(requests) / stitchBatchSync(requests): requests[k] = [images, direction, mode, gap, limits, filter] (what stitch takes, minus
 * the device-group arguments: a batch runs on one GPU).  N x Page.onStitch (index.js:1186-1633) through ist_stitch_rgba8_batch.
 * Result: an array with {width,height,data,plan} per request, null for a request without images.
 * stitchPngBatch / stitchPngBatchSync: the same requests, a PNG file per request (the form setPngLevel chose).
 * stitchJpegBatch / stitchJpegBatchSync: requests[k] = [..., quality, subsampling], a JPEG file per request (ist_stitch_jpeg_batch). */
typedef struct {
  job h;
  int n; out_kind out;
  images_t* im; strip_t* strips; ist_stitch_request* reqs;
  int* quality; int* subsampling;         /* OUT_JPEG: requests[k][6], requests[k][7] */
  ist_plan* plans; uint8_t** blocks; int64_t* lens;    /* request k's canvas, or lens[k] bytes of its file */
} batch_job;

static int batch_run(ist_ctx* ctx, job* h) {
  batch_job* j = (batch_job*)h;
  return j->out == OUT_JPEG ? ist_stitch_jpeg_batch(ctx, j->reqs, j->n, j->quality, j->subsampling, j->plans, j->blocks, j->lens)
       : j->out == OUT_PNG  ? ist_stitch_png_batch(ctx, j->reqs, j->n, j->plans, j->blocks, j->lens)
                            : ist_stitch_rgba8_batch(ctx, j->reqs, j->n, j->plans, j->blocks);
}
static napi_value batch_result(napi_env env, job* h) {
  batch_job* j = (batch_job*)h;
  napi_value arr;
  if (napi_create_array_with_length(env, (size_t)j->n, &arr) != napi_ok) return NULL;
  for (int k = 0; k < j->n; k++) {
    napi_value e = j->blocks[k] ? export_to_js(env, j->out, &j->plans[k], &j->blocks[k], j->lens[k], NULL) : null_of(env);
    if (!e) return NULL;
    napi_set_element(env, arr, (uint32_t)k, e);
  }
  return arr;
}
static void batch_free(napi_env env, job* h) {
  batch_job* j = (batch_job*)h;
  for (int k = 0; k < j->n; k++) {
    images_free(env, &j->im[k]);
    ist_plan_free(&j->plans[k]);
    if (j->blocks[k]) ist_free(j->blocks[k]);
  }
  free(j->im); free(j->strips); free(j->reqs); free(j->plans); free(j->blocks); free(j->lens); free(j->quality); free(j->subsampling); free(j);
}
static const job_kind BATCH = {batch_run, batch_result, batch_free};

static job* batch_parse(napi_env env, napi_callback_info info, int want_refs, out_kind out) {
  static const char usage[] = "stitchBatch([[images, direction, mode, gap, limits, filter], ...])";
  napi_value argv[1]; uint32_t n = 0;
  if (!args_of(env, info, 1, 1, argv, usage)) return NULL;
  if (!array_len(env, argv[0], &n)) return (job*)throw_type(env, usage);
  batch_job* j = (batch_job*)calloc(1, sizeof *j);
  j->h.kind = &BATCH; j->out = out;
  j->n = (int)n;
  j->im = (images_t*)calloc(n ? n : 1, sizeof(images_t));
  j->strips = (strip_t*)calloc(n ? n : 1, sizeof(strip_t));
  j->reqs = (ist_stitch_request*)calloc(n ? n : 1, sizeof(ist_stitch_request));
  j->plans = (ist_plan*)calloc(n ? n : 1, sizeof(ist_plan));
  j->blocks = (uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*));
  j->lens = (int64_t*)calloc(n ? n : 1, sizeof(int64_t));
  j->quality = (int*)calloc(n ? n : 1, sizeof(int));
  j->subsampling = (int*)calloc(n ? n : 1, sizeof(int));
  if (n == 0) j->h.decided = 1;                         /* (rc IST_OK: an empty array, with or without a device) */
  for (uint32_t k = 0; k < n; k++) {
    napi_value r, a[8]; uint32_t m = 0;
    napi_get_element(env, argv[0], k, &r);
    if (!array_len(env, r, &m) || m < 6) {
      napi_throw_type_error(env, NULL, "stitchBatch: requests[k] must be [images, direction, mode, gap, limits, filter]");
      batch_free(env, &j->h); return NULL;
    }
    for (uint32_t i = 0; i < 8; i++) napi_get_element(env, r, i, &a[i]);      /* (past the end: undefined) */
    if (!images_parse(env, a[0], &j->im[k], want_refs)) { batch_free(env, &j->h); return NULL; }
    const strip_t* s = &j->strips[k];
    strip_parse(env, a + 1, &j->strips[k]);
    j->quality[k] = int_of(env, a[6], 90); j->subsampling[k] = int_of(env, a[7], IST_JPEG_420);
    ist_stitch_request* q = &j->reqs[k];
    q->images = j->im[k].descs; q->src = j->im[k].data; q->src_pitch = j->im[k].pitch; q->n_images = j->im[k].n;
    q->direction = s->direction; q->mode = s->mode; q->gap = s->gap; q->limits = &s->lim; q->filter = s->filter;
    if (!j->h.decided && images_missing(&j->im[k], (int)k, j->h.err, sizeof j->h.err)) { j->h.decided = 1; j->h.rc = IST_E_DECODE; }
  }
  return &j->h;
}

static napi_value js_stitch_batch(napi_env env, napi_callback_info info) { return job_queue(env, batch_parse(env, info, 1, OUT_PIXELS), "imagestitch.stitchBatch"); }
static napi_value js_stitch_batch_sync(napi_env env, napi_callback_info info) { return job_now(env, batch_parse(env, info, 0, OUT_PIXELS)); }
static napi_value js_stitch_png_batch(napi_env env, napi_callback_info info) { return job_queue(env, batch_parse(env, info, 1, OUT_PNG), "imagestitch.stitchPngBatch"); }
static napi_value js_stitch_png_batch_sync(napi_env env, napi_callback_info info) { return job_now(env, batch_parse(env, info, 0, OUT_PNG)); }
static napi_value js_stitch_jpeg_batch(napi_env env, napi_callback_info info) { return job_queue(env, batch_parse(env, info, 1, OUT_JPEG), "imagestitch.stitchJpegBatch"); }
static napi_value js_stitch_jpeg_batch_sync(napi_env env, napi_callback_info info) { return job_now(env, batch_parse(env, info, 0, OUT_JPEG)); }

/* ---- render, encode, decode ------------------------------------------------------------------------------------------------ */
/* render(canvasW, canvasH, clearRGBA(Uint8Array 4), ops(Float64Array 18/op), images, filter, region|null, asPng?) -> Buffer.  An image
 * may come without pixels here: an op list need not touch it.  A clear colour of fewer than 4 bytes is transparent black. */
static napi_value js_render(napi_env env, napi_callback_info info) {
  napi_value argv[8];
  if (!args_of(env, info, 6, 8, argv, "render(canvasW, canvasH, clear, ops, images, filter, region)")) return NULL;
  const double cw = num_of(env, argv[0], 0), ch = num_of(env, argv[1], 0);
  uint8_t clear[4] = {0, 0, 0, 0};
  const uint8_t* cp; size_t clen;
  if (bytes_of(env, argv[2], &cp, &clen) && clen >= 4) memcpy(clear, cp, 4);
  napi_typedarray_type tt; size_t len; void* p;
  if (!typed_of(env, argv[3], &tt, &p, &len)) return throw_type(env, "ops must be a Float64Array");
  if (tt != napi_float64_array || len % 18) return throw_type(env, "ops must be a Float64Array with 18 doubles per op");
  ist_region reg = {0, 0, (int32_t)cw, (int32_t)ch};
  const int have_region = type_of(env, argv[6]) == napi_object;
  if (have_region) {
    int64_t v;
    if (get_named_i64(env, argv[6], "x", &v)) reg.x = (int32_t)v;
    if (get_named_i64(env, argv[6], "y", &v)) reg.y = (int32_t)v;
    if (get_named_i64(env, argv[6], "w", &v)) reg.w = (int32_t)v;
    if (get_named_i64(env, argv[6], "h", &v)) reg.h = (int32_t)v;
  }
  images_t im;
  if (!images_parse(env, argv[4], &im, 0)) return NULL;
  ist_ctx* ctx = NULL;
  if (reg.w < 1 || reg.h < 1) napi_throw_range_error(env, NULL, "empty region");
  else ctx = ctx_or_throw(env);
  if (!ctx) { images_free(env, &im); return NULL; }
  const int n_ops = (int)(len / 18), filter = int_of(env, argv[5], 1);
  ist_op* ops = (ist_op*)calloc(n_ops ? n_ops : 1, sizeof(ist_op));
  const double* q = (const double*)p;
  for (int i = 0; i < n_ops; i++, q += 18) {
    ops[i].kind = (int32_t)q[0]; ops[i].image = (int32_t)q[1];
    memcpy(ops[i].m, q + 2, 6 * sizeof(double));
    memcpy(ops[i].s, q + 8, 4 * sizeof(double));
    memcpy(ops[i].d, q + 12, 4 * sizeof(double));
    const uint32_t c = (uint32_t)q[16];
    ops[i].rgba[0] = c & 255; ops[i].rgba[1] = (c >> 8) & 255; ops[i].rgba[2] = (c >> 16) & 255; ops[i].rgba[3] = (c >> 24) & 255;
  }
  napi_value out = NULL;
  if (bool_of(env, argv[7], 0)) {       /* asPng: wx.canvasToTempFilePath({fileType:'png'}) - the canvas stays on the device */
    uint8_t* png = NULL; int64_t n = 0;
    const int rc = ist_render_png(ctx, (int64_t)cw, (int64_t)ch, clear, ops, n_ops, im.descs, im.data, im.pitch, im.n, filter, &png, &n);
    out = rc < 0 ? throw_ist(env, rc) : file_to_js(env, png, n);
  } else {
    void* out_data = NULL;
    if (napi_create_buffer(env, (size_t)reg.w * (size_t)reg.h * 4, &out_data, &out) != napi_ok) out = throw_oom(env);
    else {
      const int rc = ist_render_rgba8(ctx, (int64_t)cw, (int64_t)ch, clear, ops, n_ops, im.descs, im.data, im.pitch, im.n, filter,
                                      have_region ? &reg : NULL, (uint8_t*)out_data, (size_t)reg.w * 4);
      if (rc < 0) out = throw_ist(env, rc);
    }
  }
  images_free(env, &im); free(ops);
  return out;
}

/* the (data, width, height) that open an encoder's arguments; 0 with the exception pending */
static int rgba_parse(napi_env env, const napi_value* a, const char* not_bytes, const uint8_t** p, double* w, double* h) {
  size_t len;
  if (!bytes_of(env, a[0], p, &len)) { napi_throw_type_error(env, NULL, not_bytes); return 0; }
  *w = num_of(env, a[1], 0); *h = num_of(env, a[2], 0);
  if (*w < 1 || *h < 1 || (double)len < *w * *h * 4) { napi_throw_range_error(env, NULL, "data is smaller than width*height*4"); return 0; }
  return 1;
}

/* encodePng(data: Uint8Array RGBA, width, height) -> Buffer (PNG file bytes) */
static napi_value js_encode_png(napi_env env, napi_callback_info info) {
  napi_value argv[3]; const uint8_t* p; double w, h; ist_ctx* ctx;
  if (!args_of(env, info, 3, 3, argv, "encodePng(data, width, height)")) return NULL;
  if (!rgba_parse(env, argv, "encodePng expects a Buffer / Uint8Array", &p, &w, &h) || !(ctx = ctx_or_throw(env))) return NULL;
  uint8_t* png = NULL; int64_t n = 0;
  const int rc = ist_png_encode_rgba8(ctx, p, (size_t)w * 4, (int64_t)w, (int64_t)h, &png, &n);
  return rc < 0 ? throw_ist(env, rc) : file_to_js(env, png, n);
}

/* encodeJpeg(data: Uint8Array RGBA, width, height, quality, subsampling: IST_JPEG_*) -> Buffer (JFIF file bytes; alpha is not read) */
static napi_value js_encode_jpeg(napi_env env, napi_callback_info info) {
  napi_value argv[5]; const uint8_t* p; double w, h; ist_ctx* ctx;
  if (!args_of(env, info, 5, 5, argv, "encodeJpeg(data, width, height, quality, subsampling)")) return NULL;
  if (!rgba_parse(env, argv, "encodeJpeg expects a Buffer / Uint8Array", &p, &w, &h) || !(ctx = ctx_or_throw(env))) return NULL;
  uint8_t* jpg = NULL; int64_t n = 0;
  const int rc = ist_jpeg_encode_rgba8(ctx, p, (size_t)w * 4, (int64_t)w, (int64_t)h, int_of(env, argv[3], 0), int_of(env, argv[4], -1), &jpg, &n);
  return rc < 0 ? throw_ist(env, rc) : file_to_js(env, jpg, n);
}

/* decodeImage(file: Buffer) -> {width, height, orientation, opaque, data}: PNG (host) or JPEG (host Huffman + GPU reconstruction) */
static napi_value js_decode_image(napi_env env, napi_callback_info info) {
  napi_value argv[1]; const uint8_t* p; size_t len;
  if (!args_of(env, info, 1, 1, argv, "decodeImage(buffer)")) return NULL;
  if (!bytes_of(env, argv[0], &p, &len)) return throw_type(env, "decodeImage expects a Buffer / Uint8Array");
  int32_t w = 0, h = 0, orient = 0;
  int rc = ist_image_info(p, (int64_t)len, &w, &h, &orient);
  if (rc < 0) return throw_ist(env, rc);
  const int is_jpeg = len >= 2 && p[0] == 0xFF && p[1] == 0xD8;
  ist_ctx* ctx = is_jpeg ? ctx_or_throw(env) : NULL;
  if (is_jpeg && !ctx) return NULL;
  void* out_data = NULL; napi_value buf;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) return throw_oom(env);
  color_begin(ctx, IST_COLOR_PROFILE_IGNORE);            /* (never inside another call's setting) */
  rc = ist_image_decode_rgba8(ctx, p, (int64_t)len, (uint8_t*)out_data, (size_t)w * 4, (int64_t)h);
  color_end(ctx);
  if (rc < 0) return throw_ist(env, rc);
  napi_value o = pixels_to_js(env, w, h, buf);
  set_num(env, o, "orientation", orient ? orient : 1);
  set_bool(env, o, "opaque", is_jpeg);
  return o;
}

/* decodePng(file: Buffer) -> {width, height, data: Buffer RGBA8}   (host decode, no GPU needed) */
static napi_value js_decode_png(napi_env env, napi_callback_info info) {
  napi_value argv[1]; const uint8_t* p; size_t len;
  if (!args_of(env, info, 1, 1, argv, "decodePng(buffer)")) return NULL;
  if (!bytes_of(env, argv[0], &p, &len)) return throw_type(env, "decodePng expects a Buffer / Uint8Array");
  int32_t w = 0, h = 0;
  int rc = ist_png_info(p, (int64_t)len, &w, &h);
  if (rc < 0) return throw_ist(env, rc);
  void* out_data = NULL; napi_value buf;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) return throw_oom(env);
  rc = ist_png_decode_rgba8(p, (int64_t)len, (uint8_t*)out_data, (size_t)w * 4, (int64_t)h);
  if (rc < 0) return throw_ist(env, rc);
  return pixels_to_js(env, w, h, buf);
}

static napi_value js_device_count(napi_env env, napi_callback_info info) {
  (void)info; napi_value v; napi_create_int32(env, ist_device_count(), &v); return v;
}
static napi_value js_last_error(napi_env env, napi_callback_info info) {
  (void)info; napi_value v; napi_create_string_utf8(env, ist_last_error(), NAPI_AUTO_LENGTH, &v); return v;
}
static napi_value js_abi_version(napi_env env, napi_callback_info info) {
  (void)info; napi_value v; napi_create_int32(env, ist_abi_version(), &v); return v;
}

/* a process-wide PNG setting of the context: applies to every PNG this process exports afterwards */
static napi_value set_png(napi_env env, napi_callback_info info, const char* usage, int (*set)(ist_ctx*, int)) {
  napi_value argv[1]; int32_t v = 0; ist_ctx* ctx;
  if (!args_of(env, info, 1, 1, argv, usage)) return NULL;
  if (napi_get_value_int32(env, argv[0], &v) != napi_ok) return throw_type(env, usage);
  if (!(ctx = ctx_or_throw(env))) return NULL;
  const int rc = set(ctx, v);
  return rc < 0 ? throw_ist(env, rc) : undefined_of(env);
}
/* setPngLevel(level): 0 stored deflate blocks, 1 compressed on the GPU (ist_ctx_set_png_level) */
static napi_value js_set_png_level(napi_env env, napi_callback_info info) { return set_png(env, info, "setPngLevel(level)", ist_ctx_set_png_level); }
/* setPngColor(color): 0 RGBA (colour type 6), 1 RGB (colour type 2, alpha not read; level 1 only) - ist_ctx_set_png_color */
static napi_value js_set_png_color(napi_env env, napi_callback_info info) { return set_png(env, info, "setPngColor(color)", ist_ctx_set_png_color); }
/* setPngFilter(filter): 0 Paeth on every row, 1 adaptive (a type per row, chosen on the GPU; level 1 only) - ist_ctx_set_png_filter */
static napi_value js_set_png_filter(napi_env env, napi_callback_info info) { return set_png(env, info, "setPngFilter(filter)", ist_ctx_set_png_filter); }
/* setPngMatch(match): 0 runs inside a 64-byte span, 1 window (a chunk also copies from its earlier spans, found on the GPU; level 1 only) - ist_ctx_set_png_match */
static napi_value js_set_png_match(napi_env env, napi_callback_info info) { return set_png(env, info, "setPngMatch(match)", ist_ctx_set_png_match); }

/* ---- resident bitmaps ------------------------------------------------------------------------------------------------------ */
/* the code of a failed ist_bitmap_upload (it returns NULL; the message tells which rule failed) */
static int upload_fail_code(void) {
  const char* m = ist_last_error();
  if (!strncmp(m, "\xe5\x9b\xbe\xe7\x89\x87", 6)) return IST_E_DECODE;       /* '图片0解码异常' */
  if (!strncmp(m, "src_pitch", 9)) return IST_E_INVALID;
  if (!strncmp(m, "out of device memory", 20)) return IST_E_NOMEM;
  return IST_E_HIP;
}

/* uploadBitmap([image]) -> handle: one host image (as stitch takes it) into a bitmap with its desc */
static napi_value js_upload_bitmap(napi_env env, napi_callback_info info) {
  napi_value argv[1]; images_t im; char err[256];
  if (!args_of(env, info, 1, 1, argv, "uploadBitmap([image])")) return NULL;
  if (!images_parse(env, argv[0], &im, 0)) return NULL;
  ist_ctx* ctx = NULL;
  if (im.n != 1) napi_throw_type_error(env, NULL, "uploadBitmap takes one image");
  else if (images_missing(&im, -1, err, sizeof err)) throw_code(env, IST_E_DECODE, err);
  else ctx = ctx_or_throw(env);
  ist_bitmap* b = ctx ? ist_bitmap_upload(ctx, &im.descs[0], im.data[0], im.pitch[0]) : NULL;
  images_free(env, &im);
  if (!ctx) return NULL;
  if (!b) return throw_ist(env, upload_fail_code());
  napi_value h = bitmap_wrap(env, b);
  if (!h) napi_throw_error(env, NULL, "could not wrap the bitmap");
  return h;
}

/* decodeBitmaps(files: Buffer[], scales?: number[], colorProfile?: number) -> Promise<handle[]> (ist_bitmaps_decode_scaled: all or
 * nothing; scales = one decode denominator per file, 1 / 2 / 4 / 8, checked by the library; absent: all 1, which is ist_bitmaps_decode;
 * colorProfile = IST_COLOR_PROFILE_*, absent: ignore, set on the context for this call alone) */
typedef struct { job h; files_t files; int32_t* denom; int profile; ist_bitmap** out; } decode_job;

static int decode_run(ist_ctx* ctx, job* h) {
  decode_job* j = (decode_job*)h;
  if (!j->files.n) return IST_OK;
  color_begin(ctx, j->profile);
  const int rc = ist_bitmaps_decode_scaled(ctx, j->files.ptr, j->files.len, j->files.n, j->denom, j->out);
  color_end(ctx);
  return rc;
}
static napi_value decode_result(napi_env env, job* h) {
  decode_job* j = (decode_job*)h;
  napi_value arr;
  if (napi_create_array_with_length(env, (size_t)j->files.n, &arr) != napi_ok) return NULL;
  for (int i = 0; i < j->files.n; i++) {
    napi_value b = bitmap_wrap(env, j->out[i]);
    j->out[i] = NULL;                                     /* the handle owns the reference now (or released it) */
    if (!b || napi_set_element(env, arr, (uint32_t)i, b) != napi_ok) return NULL;
  }
  return arr;
}
static void decode_free(napi_env env, job* h) {
  decode_job* j = (decode_job*)h;
  for (int i = 0; i < j->files.n; i++) if (j->out[i]) ist_bitmap_release(j->out[i]);
  files_free(env, &j->files);
  free(j->denom); free(j->out); free(j);
}
static const job_kind DECODE = {decode_run, decode_result, decode_free};

static napi_value js_decode_bitmaps(napi_env env, napi_callback_info info) {
  static const char usage[] = "decodeBitmaps(files: Buffer[], scales?: number[], colorProfile?: number)";
  napi_value argv[3]; files_t files; int32_t* denom = NULL; uint32_t ns = 0;
  if (!args_of(env, info, 1, 3, argv, usage) || !files_parse(env, argv[0], usage, &files)) return NULL;
  if (!is_nullish(env, argv[1])) {
    if (!array_len(env, argv[1], &ns) || ns != (uint32_t)files.n) { files_free(env, &files); return throw_type(env, "decodeBitmaps: scales must hold one number per file"); }
    denom = (int32_t*)calloc(ns ? ns : 1, sizeof *denom);
    for (uint32_t i = 0; i < ns; i++) {
      napi_value v;
      denom[i] = napi_get_element(env, argv[1], i, &v) == napi_ok && type_of(env, v) == napi_number ? int_of(env, v, 0) : 0;      /* (0: the library names the file) */
    }
  }
  decode_job* j = (decode_job*)calloc(1, sizeof *j);
  j->h.kind = &DECODE; j->files = files; j->denom = denom; j->profile = int_of(env, argv[2], IST_COLOR_PROFILE_IGNORE);
  j->out = (ist_bitmap**)calloc(files.n ? files.n : 1, sizeof(ist_bitmap*));
  return job_queue(env, &j->h, "imagestitch.decodeBitmaps");
}

/* ---- lossless JPEG joins (ist_jpeg_join_check, ist_jpeg_join_files) -------------------------------------------------------- */
/* {ok, reason, image, width, height, subsampling}: reason / subsampling as the library's codes (index.js names them) */
static napi_value join_info_to_js(napi_env env, const ist_jpeg_join_info* info) {
  napi_value o;
  if (napi_create_object(env, &o) != napi_ok) return NULL;
  set_bool(env, o, "ok", info->reason == IST_JOIN_OK);
  set_num(env, o, "reason", info->reason);
  set_num(env, o, "image", info->image);
  set_num(env, o, "width", (double)info->width);
  set_num(env, o, "height", (double)info->height);
  set_num(env, o, "subsampling", info->subsampling);
  return o;
}

/* joinJpegCheck(files: Buffer[], direction: number) -> the record (ist_jpeg_join_check: pure CPU, headers only; a refusal is a
 * record, not an Error) */
static napi_value js_join_jpeg_check(napi_env env, napi_callback_info info) {
  static const char usage[] = "joinJpegCheck(files: Buffer[], direction: number)";
  napi_value argv[2]; files_t files; ist_jpeg_join_info rec;
  if (!args_of(env, info, 2, 2, argv, usage) || !files_parse(env, argv[0], usage, &files)) return NULL;
  const int rc = ist_jpeg_join_check(files.ptr, files.len, files.n, int_of(env, argv[1], -1), &rec);
  files_free(env, &files);
  if (rc < 0 && rc != IST_E_UNSUPPORTED) return throw_ist(env, rc);
  return join_info_to_js(env, &rec);
}

/* joinJpeg(files: Buffer[], direction: number, flags: number) -> Promise<Buffer> (ist_jpeg_join_files; flags 0 or IST_JPEG_OPTIMIZE) */
typedef struct { job h; files_t files; int direction, flags; uint8_t* file; int64_t len; } join_job;

static int join_run(ist_ctx* ctx, job* h) {
  join_job* j = (join_job*)h;
  return ist_jpeg_join_files(ctx, j->files.ptr, j->files.len, j->files.n, j->direction, j->flags, NULL, &j->file, &j->len);
}
static napi_value join_result(napi_env env, job* h) {
  join_job* j = (join_job*)h;
  napi_value buf = block_to_buffer(env, j->file, (size_t)j->len);
  j->file = NULL;                                         /* the Buffer owns the block now (or it was freed) */
  return buf;
}
static void join_free(napi_env env, job* h) {
  join_job* j = (join_job*)h;
  if (j->file) ist_free(j->file);
  files_free(env, &j->files);
  free(j);
}
static const job_kind JOIN = {join_run, join_result, join_free};

static napi_value js_join_jpeg(napi_env env, napi_callback_info info) {
  static const char usage[] = "joinJpeg(files: Buffer[], direction: number, flags?: number)";
  napi_value argv[3]; files_t files;
  if (!args_of(env, info, 2, 3, argv, usage) || !files_parse(env, argv[0], usage, &files)) return NULL;
  join_job* j = (join_job*)calloc(1, sizeof *j);
  if (!j) { files_free(env, &files); return throw_oom(env); }
  j->h.kind = &JOIN; j->files = files; j->direction = int_of(env, argv[1], -1); j->flags = int_of(env, argv[2], 0);
  return job_queue(env, &j->h, "imagestitch.joinJpeg");
}

/* imageColor(file: Buffer) -> 0 .. 3, the IST_COLOR_* kind of the file's ICC profile (ist_image_color: pure CPU) */
static napi_value js_image_color(napi_env env, napi_callback_info info) {
  napi_value argv[1], out; const uint8_t* p; size_t len; int32_t kind = 0;
  if (!args_of(env, info, 1, 1, argv, "imageColor(buffer)")) return NULL;
  if (!bytes_of(env, argv[0], &p, &len)) return throw_type(env, "imageColor expects a Buffer / Uint8Array");
  const int rc = ist_image_color(p, (int64_t)len, &kind);
  if (rc < 0) return throw_ist(env, rc);
  return napi_create_int32(env, kind, &out) == napi_ok ? out : NULL;
}

/* decodeScaleFit(width, height, minWidth, minHeight) -> 1 | 2 | 4 | 8 (ist_decode_scale_fit: pure CPU) */
static napi_value js_decode_scale_fit(napi_env env, napi_callback_info info) {
  napi_value argv[4], out;
  if (!args_of(env, info, 4, 4, argv, "decodeScaleFit(width, height, minWidth, minHeight)")) return NULL;
  const int d = ist_decode_scale_fit(int_of(env, argv[0], 0), int_of(env, argv[1], 0), int_of(env, argv[2], 0), int_of(env, argv[3], 0));
  if (d < 0) return throw_ist(env, d);
  napi_create_int32(env, d, &out);
  return out;
}

static napi_value js_bitmap_desc(napi_env env, napi_callback_info info) {
  napi_value argv[1]; ist_bitmap* b; ist_image_desc d;
  if (!args_of(env, info, 1, 1, argv, "bitmapDesc(handle)") || !(b = bitmap_of(env, argv[0]))) return NULL;
  const int rc = ist_bitmap_desc(b, &d);
  if (rc < 0) return throw_ist(env, rc);
  napi_value o;
  napi_create_object(env, &o);
  set_num(env, o, "width", d.width); set_num(env, o, "height", d.height); set_num(env, o, "orientation", d.orientation);
  set_num(env, o, "bmpWidth", d.bmp_width > 0 ? d.bmp_width : d.width); set_num(env, o, "bmpHeight", d.bmp_height > 0 ? d.bmp_height : d.height);
  set_bool(env, o, "opaque", d.opaque);
  set_num(env, o, "fileSize", (double)d.file_size);
  return o;
}

/* bitmapDownload(handle) -> Buffer (bmpWidth * bmpHeight * 4 bytes, dense rows) */
static napi_value js_bitmap_download(napi_env env, napi_callback_info info) {
  napi_value argv[1]; ist_bitmap* b; ist_image_desc d;
  if (!args_of(env, info, 1, 1, argv, "bitmapDownload(handle)") || !(b = bitmap_of(env, argv[0]))) return NULL;
  ist_bitmap_desc(b, &d);
  const int64_t w = d.bmp_width > 0 ? d.bmp_width : d.width, h = d.bmp_height > 0 ? d.bmp_height : d.height;
  void* out_data = NULL; napi_value buf;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) return throw_oom(env);
  const int rc = ist_bitmap_download(b, (uint8_t*)out_data, (size_t)w * 4, h);
  return rc < 0 ? throw_ist(env, rc) : buf;
}

/* bitmapPreview(handle, boxWidth, boxHeight) -> {width, height, data}: the stored pixels shrunk to fit the box (ist_preview_fit, then
 * ist_bitmap_preview: reduced in GPU memory, only the preview crosses PCIe) */
static napi_value js_bitmap_preview(napi_env env, napi_callback_info info) {
  napi_value argv[3]; ist_bitmap* b; ist_ctx* ctx; ist_image_desc d; int32_t pw = 0, ph = 0;
  if (!args_of(env, info, 3, 3, argv, "bitmapPreview(handle, width, height)") || !(b = bitmap_of(env, argv[0]))) return NULL;
  if (type_of(env, argv[1]) != napi_number || type_of(env, argv[2]) != napi_number) return throw_type(env, "bitmapPreview(handle, width, height): the box sides must be numbers");
  if (!(ctx = ctx_or_throw(env))) return NULL;
  ist_bitmap_desc(b, &d);
  int rc = ist_preview_fit(d.bmp_width > 0 ? d.bmp_width : d.width, d.bmp_height > 0 ? d.bmp_height : d.height, num_of(env, argv[1], 0), num_of(env, argv[2], 0), &pw, &ph);
  if (rc < 0) return throw_ist(env, rc);
  void* out_data = NULL; napi_value buf;
  if (napi_create_buffer(env, (size_t)pw * (size_t)ph * 4, &out_data, &buf) != napi_ok) return throw_oom(env);
  rc = ist_bitmap_preview(ctx, b, pw, ph, (uint8_t*)out_data, (size_t)pw * 4);
  return rc < 0 ? throw_ist(env, rc) : pixels_to_js(env, pw, ph, buf);
}

/* thumbnails(handles, cellWidth, cellHeight, mode, orient) -> Promise<[{width, height, data}]> (ist_bitmaps_thumbs: the grid of chosen
 * images, index.wxml:4-22 - every bitmap cropped or fitted, turned and shrunk in one launch pair per form, one copy down).  Every
 * data Buffer is a view of ONE pinned block, given back to the pool when the last of them is collected. */
typedef struct { job h; bitmaps_t bm; ist_thumb_spec spec; ist_thumb_item* items; uint8_t* pixels; } thumbs_job;
typedef struct { uint8_t* pixels; int live; } thumbs_block;

static void thumbs_block_drop(thumbs_block* blk) {
  if (--blk->live == 0) { ist_free(blk->pixels); free(blk); }
}
static void thumbs_view_gone(napi_env env, void* data, void* hint) {
  (void)env; (void)data;
  thumbs_block_drop((thumbs_block*)hint);                 /* (finalizers run on the JS thread: no lock) */
}
static int thumbs_run(ist_ctx* ctx, job* h) {
  thumbs_job* j = (thumbs_job*)h;
  return ist_bitmaps_thumbs(ctx, j->bm.b, j->bm.n, &j->spec, j->items, &j->pixels);
}
static napi_value thumbs_result(napi_env env, job* h) {
  thumbs_job* j = (thumbs_job*)h;
  napi_value arr;
  if (napi_create_array_with_length(env, (size_t)j->bm.n, &arr) != napi_ok) return NULL;
  thumbs_block* blk = (thumbs_block*)calloc(1, sizeof *blk);
  blk->pixels = j->pixels; blk->live = 1;                 /* (this function's own hold, dropped below) */
  j->pixels = NULL;
  for (int i = 0; i < j->bm.n && arr; i++) {
    const ist_thumb_item* t = &j->items[i];
    napi_value buf;
    if (napi_create_external_buffer(env, (size_t)t->width * (size_t)t->height * 4, blk->pixels + t->offset, thumbs_view_gone, blk, &buf) != napi_ok) { arr = NULL; break; }
    blk->live++;
    if (napi_set_element(env, arr, (uint32_t)i, pixels_to_js(env, (double)t->width, (double)t->height, buf)) != napi_ok) arr = NULL;
  }
  thumbs_block_drop(blk);
  return arr;
}
static void thumbs_free(napi_env env, job* h) {
  thumbs_job* j = (thumbs_job*)h;
  (void)env;
  bitmaps_free(&j->bm);
  if (j->pixels) ist_free(j->pixels);
  free(j->items); free(j);
}
static const job_kind THUMBS = {thumbs_run, thumbs_result, thumbs_free};

static napi_value js_thumbnails(napi_env env, napi_callback_info info) {
  static const char usage[] = "thumbnails(bitmaps, cellWidth, cellHeight, mode, orient)";
  napi_value argv[5]; bitmaps_t bm;
  if (!args_of(env, info, 5, 5, argv, usage) || !bitmaps_parse(env, argv[0], usage, &bm)) return NULL;
  thumbs_job* j = (thumbs_job*)calloc(1, sizeof *j);
  j->h.kind = &THUMBS; j->bm = bm;
  j->items = (ist_thumb_item*)calloc(bm.n ? bm.n : 1, sizeof(ist_thumb_item));
  const double w = num_of(env, argv[1], 0), h = num_of(env, argv[2], 0);
  j->spec.cell_w = w >= 1 && w <= 2147483647.0 ? (int32_t)w : 0;      /* (0: the library's 'the cell must be at least 1 x 1') */
  j->spec.cell_h = h >= 1 && h <= 2147483647.0 ? (int32_t)h : 0;
  j->spec.mode = int_of(env, argv[3], 0);
  j->spec.apply_orientation = bool_of(env, argv[4], 1);
  return job_queue(env, &j->h, "imagestitch.thumbnails");
}

/* ---- overlap removal for scrolled screenshots ------------------------------------------------------------------------------ */
/* findOverlaps(handles, tolerance, minRows, minInformative) -> Promise<[{header, footer, overlap, cost}]> (ist_bitmaps_overlap: one
 * record per neighbouring pair of a vertical strip, top to bottom); findOverlapsSync(...same...) -> the array itself */
typedef struct { job h; bitmaps_t bm; ist_overlap_opts opts; ist_overlap* out; } overlap_job;

static int overlap_run(ist_ctx* ctx, job* h) {
  overlap_job* j = (overlap_job*)h;
  return ist_bitmaps_overlap(ctx, j->bm.b, j->bm.n, &j->opts, j->out);
}
static napi_value overlap_result(napi_env env, job* h) {
  overlap_job* j = (overlap_job*)h;
  napi_value arr;
  if (napi_create_array_with_length(env, (size_t)(j->bm.n - 1), &arr) != napi_ok) return NULL;
  for (int i = 0; i + 1 < j->bm.n; i++) {
    napi_value o;
    if (napi_create_object(env, &o) != napi_ok) return NULL;
    set_num(env, o, "header", j->out[i].header); set_num(env, o, "footer", j->out[i].footer);
    set_num(env, o, "overlap", j->out[i].overlap); set_num(env, o, "cost", (double)j->out[i].cost);
    if (napi_set_element(env, arr, (uint32_t)i, o) != napi_ok) return NULL;
  }
  return arr;
}
static void overlap_free(napi_env env, job* h) {
  overlap_job* j = (overlap_job*)h;
  (void)env;
  bitmaps_free(&j->bm);
  free(j->out); free(j);
}
static const job_kind OVERLAP = {overlap_run, overlap_result, overlap_free};

static job* overlap_parse(napi_env env, napi_callback_info info) {
  static const char usage[] = "findOverlaps(bitmaps, tolerance, minRows, minInformative)";
  napi_value argv[4]; bitmaps_t bm;
  if (!args_of(env, info, 4, 4, argv, usage) || !bitmaps_parse(env, argv[0], usage, &bm)) return NULL;
  overlap_job* j = (overlap_job*)calloc(1, sizeof *j);
  j->h.kind = &OVERLAP; j->bm = bm;
  j->opts.tolerance = int_of(env, argv[1], -1); j->opts.min_rows = int_of(env, argv[2], -1); j->opts.min_informative = int_of(env, argv[3], -1);      /* (-1: the library's 'negative option') */
  j->out = (ist_overlap*)calloc(bm.n > 1 ? (size_t)bm.n - 1 : 1, sizeof(ist_overlap));
  return &j->h;
}
static napi_value js_find_overlaps(napi_env env, napi_callback_info info) { return job_queue(env, overlap_parse(env, info), "imagestitch.findOverlaps"); }
static napi_value js_find_overlaps_sync(napi_env env, napi_callback_info info) { return job_now(env, overlap_parse(env, info)); }

/* overlapRows(pairs: [{header, footer, overlap}], heights: number[]) -> [[top, bot]] (ist_overlap_rows: the crop rule, pure CPU) */
static napi_value js_overlap_rows(napi_env env, napi_callback_info info) {
  static const char usage[] = "overlapRows(pairs, heights)";
  napi_value argv[2], arr = NULL; uint32_t np = 0, n = 0;
  if (!args_of(env, info, 2, 2, argv, usage)) return NULL;
  if (!array_len(env, argv[0], &np) || !array_len(env, argv[1], &n) || np + 1 != (n ? n : 1)) return throw_type(env, "overlapRows(pairs, heights): n images need n - 1 pairs");
  ist_overlap* pairs = (ist_overlap*)calloc(np ? np : 1, sizeof *pairs);
  int32_t* rows = (int32_t*)calloc(3 * (size_t)(n ? n : 1), sizeof *rows);      /* heights, top, bot */
  for (uint32_t i = 0; i < np; i++) {
    napi_value e; int64_t v;
    napi_get_element(env, argv[0], i, &e);
    if (get_named_i64(env, e, "header", &v)) pairs[i].header = (int32_t)v;
    if (get_named_i64(env, e, "footer", &v)) pairs[i].footer = (int32_t)v;
    if (get_named_i64(env, e, "overlap", &v)) pairs[i].overlap = (int32_t)v;
  }
  for (uint32_t i = 0; i < n; i++) { napi_value e; napi_get_element(env, argv[1], i, &e); rows[i] = int_of(env, e, 0); }
  const int rc = ist_overlap_rows(pairs, rows, (int)n, rows + n, rows + 2 * (size_t)n);
  if (rc < 0) throw_ist(env, rc);
  else if (napi_create_array_with_length(env, n, &arr) == napi_ok) {
    for (uint32_t i = 0; i < n; i++) {
      napi_value pr, t, b;
      napi_create_array_with_length(env, 2, &pr);
      napi_create_int32(env, rows[n + i], &t); napi_create_int32(env, rows[2 * (size_t)n + i], &b);
      napi_set_element(env, pr, 0, t); napi_set_element(env, pr, 1, b);
      napi_set_element(env, arr, i, pr);
    }
  }
  free(pairs); free(rows);
  return arr;
}

/* bitmapRows(handle, y0, rows) -> handle of a view: rows [y0, y0 + rows) of the bitmap where they are (ist_bitmap_rows) */
static napi_value js_bitmap_rows(napi_env env, napi_callback_info info) {
  napi_value argv[3]; ist_bitmap* b;
  if (!args_of(env, info, 3, 3, argv, "bitmapRows(handle, y0, rows)") || !(b = bitmap_of(env, argv[0]))) return NULL;
  if (type_of(env, argv[1]) != napi_number || type_of(env, argv[2]) != napi_number) return throw_type(env, "bitmapRows(handle, y0, rows): y0 and rows must be numbers");
  ist_bitmap* v = ist_bitmap_rows(b, int_of(env, argv[1], -1), int_of(env, argv[2], 0));
  if (!v) return throw_ist(env, strstr(ist_last_error(), "orientation") || strstr(ist_last_error(), "reduced scale") ? IST_E_UNSUPPORTED : IST_E_INVALID);
  napi_value h = bitmap_wrap(env, v);
  if (!h) napi_throw_error(env, NULL, "could not wrap the bitmap");
  return h;
}

/* bitmapRelease(handle): drops the handle's reference (a released handle: nothing) */
static napi_value js_bitmap_release(napi_env env, napi_callback_info info) {
  napi_value argv[1]; bitmap_ref* r;
  if (!args_of(env, info, 1, 1, argv, "bitmapRelease(handle)") || !(r = bitmap_ref_of(env, argv[0]))) return NULL;
  if (r->b) { ist_bitmap_release(r->b); r->b = NULL; }
  return undefined_of(env);
}

static napi_value js_debug_bitmap_bytes(napi_env env, napi_callback_info info) {
  (void)info; napi_value v; napi_create_double(env, (double)ist_debug_bitmap_bytes(), &v); return v;
}

/* environment teardown: nothing of the library may still be in flight when the HIP runtime shuts down (include/imagestitch.h,
 * ist_ctx_sync); the idle pinned result blocks go back to the system */
static void on_env_cleanup(void* arg) {
  (void)arg;
  if (g_ctx) (void)ist_ctx_sync(g_ctx);
  ist_pool_trim();
}

static napi_value init(napi_env env, napi_value exports) {
  napi_add_env_cleanup_hook(env, on_env_cleanup, NULL);
  napi_property_descriptor props[] = {
      {"plan", NULL, js_plan, NULL, NULL, NULL, napi_default, NULL},
      {"stitch", NULL, js_stitch, NULL, NULL, NULL, napi_default, NULL},
      {"stitchSync", NULL, js_stitch_sync, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBatch", NULL, js_stitch_batch, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBatchSync", NULL, js_stitch_batch_sync, NULL, NULL, NULL, napi_default, NULL},
      {"stitchPngBatch", NULL, js_stitch_png_batch, NULL, NULL, NULL, napi_default, NULL},
      {"stitchPngBatchSync", NULL, js_stitch_png_batch_sync, NULL, NULL, NULL, napi_default, NULL},
      {"stitchJpegBatch", NULL, js_stitch_jpeg_batch, NULL, NULL, NULL, napi_default, NULL},
      {"stitchJpegBatchSync", NULL, js_stitch_jpeg_batch_sync, NULL, NULL, NULL, napi_default, NULL},
      {"stitchFiles", NULL, js_stitch_files, NULL, NULL, NULL, napi_default, NULL},
      {"render", NULL, js_render, NULL, NULL, NULL, napi_default, NULL},
      {"encodePng", NULL, js_encode_png, NULL, NULL, NULL, napi_default, NULL},
      {"encodeJpeg", NULL, js_encode_jpeg, NULL, NULL, NULL, napi_default, NULL},
      {"setPngLevel", NULL, js_set_png_level, NULL, NULL, NULL, napi_default, NULL},
      {"setPngColor", NULL, js_set_png_color, NULL, NULL, NULL, napi_default, NULL},
      {"setPngFilter", NULL, js_set_png_filter, NULL, NULL, NULL, napi_default, NULL},
      {"setPngMatch", NULL, js_set_png_match, NULL, NULL, NULL, napi_default, NULL},
      {"decodePng", NULL, js_decode_png, NULL, NULL, NULL, napi_default, NULL},
      {"decodeImage", NULL, js_decode_image, NULL, NULL, NULL, napi_default, NULL},
      {"deviceCount", NULL, js_device_count, NULL, NULL, NULL, napi_default, NULL},
      {"lastError", NULL, js_last_error, NULL, NULL, NULL, napi_default, NULL},
      {"abiVersion", NULL, js_abi_version, NULL, NULL, NULL, napi_default, NULL},
      {"uploadBitmap", NULL, js_upload_bitmap, NULL, NULL, NULL, napi_default, NULL},
      {"decodeBitmaps", NULL, js_decode_bitmaps, NULL, NULL, NULL, napi_default, NULL},
      {"joinJpegCheck", NULL, js_join_jpeg_check, NULL, NULL, NULL, napi_default, NULL},
      {"joinJpeg", NULL, js_join_jpeg, NULL, NULL, NULL, napi_default, NULL},
      {"imageColor", NULL, js_image_color, NULL, NULL, NULL, napi_default, NULL},
      {"decodeScaleFit", NULL, js_decode_scale_fit, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapDesc", NULL, js_bitmap_desc, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapDownload", NULL, js_bitmap_download, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapPreview", NULL, js_bitmap_preview, NULL, NULL, NULL, napi_default, NULL},
      {"thumbnails", NULL, js_thumbnails, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapRelease", NULL, js_bitmap_release, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBitmaps", NULL, js_stitch_bitmaps, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBitmapsSync", NULL, js_stitch_bitmaps_sync, NULL, NULL, NULL, napi_default, NULL},
      {"debugBitmapBytes", NULL, js_debug_bitmap_bytes, NULL, NULL, NULL, napi_default, NULL},
      {"findOverlaps", NULL, js_find_overlaps, NULL, NULL, NULL, napi_default, NULL},
      {"findOverlapsSync", NULL, js_find_overlaps_sync, NULL, NULL, NULL, napi_default, NULL},
      {"overlapRows", NULL, js_overlap_rows, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapRows", NULL, js_bitmap_rows, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
