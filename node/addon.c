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
 *   render(canvasW, canvasH, clearRGBA, ops, images, filter, region, asPng?) -> Buffer (region pixels, or the PNG file)
 *   encodePng(data, width, height) -> Buffer;  stitch(..., filter, true) resolves {width,height,png}
 *   encodeJpeg(data, width, height, quality, subsampling) -> Buffer;  stitch / stitchBitmaps(..., filter, {quality, subsampling})
 *       resolve {width,height,jpeg} (ist_stitch_jpeg / ist_stitch_bitmaps_jpeg: asPng given as an object is the JPEG export)
 *   deviceCount(), lastError(), abiVersion()
 *   resident bitmaps (ist_bitmap_*): uploadBitmap([image]) -> handle;  decodeBitmaps(files: Buffer[]) -> Promise<handle[]>;
 *   bitmapDesc(h) -> {width,height,orientation,bmpWidth,bmpHeight,opaque,fileSize};  bitmapDownload(h) -> Buffer;  bitmapRelease(h);
 *   stitchBitmaps(handles, direction, mode, gap, limits, filter, asPng) -> Promise (as stitch);  stitchBitmapsSync(...same...);
 *   debugBitmapBytes().  A handle is an object that wraps ONE reference of a bitmap: bitmapRelease drops it (again: nothing), its
 *   finaliser drops it when the handle is collected unreleased; a stitch holds a reference of its own from the call to its completion.
 *
 * images[i] = {width, height, orientation?, fileSize?, opaque?, bmpWidth?, bmpHeight?, data?: Uint8Array|Buffer}
 * limits    = {platform: 0|1|2, maxSide, maxPixels, superSample} or null (MI355X default: caps lifted, superSample 1)
 * ops       = Float64Array, 18 doubles per op: kind, image, m[6], s[4], d[4], r|g<<8|b<<16|a<<24, reserved
 */
#define NODE_GYP_MODULE_NAME imagestitch
#include <node_api.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/imagestitch.h"

#define CHECK(call)                                                      \
  do {                                                                   \
    if ((call) != napi_ok) {                                             \
      napi_throw_error(env, NULL, "N-API call failed: " #call);          \
      return NULL;                                                       \
    }                                                                    \
  } while (0)

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

static napi_value throw_ist(napi_env env, int code) {
  char msg[512];
  const char* why = ist_last_error();
  /* same shape as the reference's toast: '拼图失败：' + message (index.js:1620) */
  strcpy(msg, "\xe6\x8b\xbc\xe5\x9b\xbe\xe5\xa4\xb1\xe8\xb4\xa5\xef\xbc\x9a");
  strncat(msg, why && *why ? why : "unknown", sizeof(msg) - strlen(msg) - 1);
  char codebuf[16];
  snprintf(codebuf, sizeof codebuf, "%d", code);
  napi_throw_error(env, codebuf, msg);
  return NULL;
}

static int get_named_i64(napi_env env, napi_value obj, const char* key, int64_t* out) {
  napi_value v; napi_valuetype t; double d;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return 0;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return 0;
  if (napi_get_value_double(env, v, &d) != napi_ok) return 0;
  *out = (int64_t)d;
  return 1;
}
static int get_named_f64(napi_env env, napi_value obj, const char* key, double* out) {
  napi_value v; napi_valuetype t;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return 0;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return 0;
  return napi_get_value_double(env, v, out) == napi_ok;
}
static int get_named_bool(napi_env env, napi_value obj, const char* key) {
  napi_value v; napi_valuetype t; bool b = false;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return 0;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_boolean) { napi_get_value_bool(env, v, &b); return b; }
  if (t == napi_number) { double d = 0; napi_get_value_double(env, v, &d); return d != 0; }
  return 0;
}

typedef struct {
  int n;
  ist_image_desc* descs;
  const uint8_t** data;
  size_t* pitch;
  napi_ref* refs;          /* keeps the JS buffers alive while async work runs */
} images_t;

static void images_free(napi_env env, images_t* im) {
  if (im->refs) for (int i = 0; i < im->n; i++) if (im->refs[i]) napi_delete_reference(env, im->refs[i]);
  free(im->descs); free(im->data); free(im->pitch); free(im->refs);
  memset(im, 0, sizeof *im);
}

/* returns 0 on failure (exception pending) */
static int images_parse(napi_env env, napi_value arr, images_t* im, int want_refs) {
  bool is_arr = false; uint32_t n = 0;
  memset(im, 0, sizeof *im);
  if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr) { napi_throw_type_error(env, NULL, "images must be an array"); return 0; }
  napi_get_array_length(env, arr, &n);
  im->n = (int)n;
  im->descs = (ist_image_desc*)calloc(n ? n : 1, sizeof(ist_image_desc));
  im->data = (const uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*));
  im->pitch = (size_t*)calloc(n ? n : 1, sizeof(size_t));
  im->refs = want_refs ? (napi_ref*)calloc(n ? n : 1, sizeof(napi_ref)) : NULL;
  for (uint32_t i = 0; i < n; i++) {
    napi_value e, d; napi_valuetype t; int64_t v;
    napi_get_element(env, arr, i, &e);
    if (napi_typeof(env, e, &t) != napi_ok || t != napi_object) { napi_throw_type_error(env, NULL, "images[i] must be an object"); return 0; }
    ist_image_desc* D = &im->descs[i];
    if (get_named_i64(env, e, "width", &v)) D->width = (int32_t)v;
    if (get_named_i64(env, e, "height", &v)) D->height = (int32_t)v;
    D->orientation = 1;
    if (get_named_i64(env, e, "orientation", &v)) D->orientation = (int32_t)v;
    if (get_named_i64(env, e, "bmpWidth", &v)) D->bmp_width = (int32_t)v;
    if (get_named_i64(env, e, "bmpHeight", &v)) D->bmp_height = (int32_t)v;
    if (get_named_i64(env, e, "fileSize", &v)) D->file_size = v;
    D->opaque = get_named_bool(env, e, "opaque");
    if (napi_get_named_property(env, e, "data", &d) == napi_ok) {
      bool is_ta = false, is_buf = false;
      napi_is_typedarray(env, d, &is_ta);
      napi_is_buffer(env, d, &is_buf);
      void* p = NULL; size_t len = 0;
      if (is_buf) napi_get_buffer_info(env, d, &p, &len);
      else if (is_ta) {
        napi_typedarray_type tt; napi_value ab; size_t off;
        napi_get_typedarray_info(env, d, &tt, &len, &p, &ab, &off);
        if (tt != napi_uint8_array && tt != napi_uint8_clamped_array) { napi_throw_type_error(env, NULL, "image data must be a Uint8Array / Buffer"); return 0; }
      }
      if (p) {
        const int64_t bw = D->bmp_width > 0 ? D->bmp_width : D->width, bh = D->bmp_height > 0 ? D->bmp_height : D->height;
        if (bw > 0 && bh > 0 && (int64_t)len < bw * bh * 4) { napi_throw_range_error(env, NULL, "image data is smaller than width*height*4"); return 0; }
        im->data[i] = (const uint8_t*)p;
        im->pitch[i] = (size_t)bw * 4;
        if (want_refs) napi_create_reference(env, d, 1, &im->refs[i]);
      }
    }
  }
  return 1;
}

static void limits_parse(napi_env env, napi_value v, ist_limits* lim) {
  napi_valuetype t = napi_undefined;
  napi_typeof(env, v, &t);
  ist_limits_unlimited(lim);
  if (t != napi_object) return;
  int64_t plat = -1; double d;
  if (get_named_i64(env, v, "platform", &plat) && plat >= 0) ist_limits_default((int)plat, lim);
  if (get_named_f64(env, v, "maxSide", &d)) lim->max_side = d;
  if (get_named_f64(env, v, "maxPixels", &d)) lim->max_pixels = d;
  if (get_named_f64(env, v, "superSample", &d)) lim->max_super_sample = d;
}

static void set_num(napi_env env, napi_value obj, const char* key, double v) {
  napi_value n; napi_create_double(env, v, &n); napi_set_named_property(env, obj, key, n);
}

static napi_value plan_to_js(napi_env env, const ist_plan* p) {
  napi_value o, rects;
  napi_create_object(env, &o);
  set_num(env, o, "outW", p->out_w); set_num(env, o, "outH", p->out_h);
  set_num(env, o, "scaleDown", p->scale_down); set_num(env, o, "superSample", p->super_sample);
  set_num(env, o, "canvasW", (double)p->canvas_w); set_num(env, o, "canvasH", (double)p->canvas_h);
  napi_value b; napi_get_boolean(env, p->big_task != 0, &b); napi_set_named_property(env, o, "bigTask", b);
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

/* plan(images, direction, mode, gap, limits) */
static napi_value js_plan(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) { napi_throw_type_error(env, NULL, "plan(images, direction, mode, gap, limits)"); return NULL; }
  images_t im;
  if (!images_parse(env, argv[0], &im, 0)) { images_free(env, &im); return NULL; }
  int32_t direction = 0, mode = 0; double gap = 0; ist_limits lim;
  napi_get_value_int32(env, argv[1], &direction);
  napi_get_value_int32(env, argv[2], &mode);
  napi_get_value_double(env, argv[3], &gap);
  limits_parse(env, argc > 4 ? argv[4] : argv[3], &lim);
  if (argc <= 4) ist_limits_unlimited(&lim);
  ist_plan p;
  const int rc = ist_plan_compute(im.descs, im.n, direction, mode, gap, &lim, &p);
  images_free(env, &im);
  if (rc < 0) return throw_ist(env, rc);
  if (rc == IST_NOTHING_TO_DO) { napi_value u; napi_get_null(env, &u); return u; }
  napi_value out = plan_to_js(env, &p);
  ist_plan_free(&p);
  return out;
}

typedef struct {
  images_t im;
  int direction, mode, filter; double gap; ist_limits lim;
  int want_png; int64_t png_len;          /* stitchPng: `pixels` holds the PNG file bytes */
  int devices[64]; int ndev, split;       /* opts.devices / opts.split: ndev 0 = the process-wide single context */
  ist_plan plan; uint8_t* pixels; int rc; char err[256];
  napi_deferred deferred; napi_async_work work;
  ist_bitmap** bitmaps; int n_bitmaps;    /* stitchBitmaps: the request's bitmaps (NULL entries allowed), one reference each, taken on the JS thread */
  int want_preview; ist_preview pv;       /* stitchPng {preview: {width, height}}: the canvas shrunk to fit that box, beside the file */
  int want_jpeg, quality, subsampling;    /* stitchJpeg: `pixels` holds the JPEG file bytes (png_len of them) */
} stitch_job;

static void stitch_job_free(napi_env env, stitch_job* j) {
  images_free(env, &j->im);
  for (int i = 0; i < j->n_bitmaps; i++) ist_bitmap_release(j->bitmaps[i]);
  free(j->bitmaps);
  free(j);
}

static void free_pixels(napi_env env, void* data, void* hint) { (void)env; (void)hint; ist_free(data); }

/* the asPng argument of a native stitch call as the JPEG export (stitchJpeg): an object {quality, subsampling: IST_JPEG_*} */
static int jpeg_parse(napi_env env, napi_value v, int* quality, int* subsampling) {
  napi_valuetype t = napi_undefined;
  napi_typeof(env, v, &t);
  if (t != napi_object) return 0;
  napi_value q, s; int32_t x = 0;
  *quality = 90; *subsampling = IST_JPEG_420;
  if (napi_get_named_property(env, v, "quality", &q) == napi_ok && napi_get_value_int32(env, q, &x) == napi_ok) *quality = x;
  if (napi_get_named_property(env, v, "subsampling", &s) == napi_ok && napi_get_value_int32(env, s, &x) == napi_ok) *subsampling = x;
  return 1;
}

/* trailing (previewWidth, previewHeight) arguments of a native PNG call: both numbers -> *pv armed with the box */
static int preview_parse(napi_env env, napi_value w, napi_value h, ist_preview* pv) {
  napi_valuetype tw = napi_undefined, th = napi_undefined;
  napi_typeof(env, w, &tw); napi_typeof(env, h, &th);
  if (tw != napi_number || th != napi_number) return 0;
  memset(pv, 0, sizeof *pv);
  napi_get_value_double(env, w, &pv->box_w);
  napi_get_value_double(env, h, &pv->box_h);
  return 1;
}

/* {width, height, data} over the library's pinned block (ist_free when the Buffer is collected); NULL when it cannot be wrapped */
static napi_value preview_to_js(napi_env env, ist_preview* pv) {
  napi_value o, buf;
  if (napi_create_external_buffer(env, (size_t)pv->width * (size_t)pv->height * 4, pv->pixels, free_pixels, NULL, &buf) != napi_ok) { ist_free(pv->pixels); pv->pixels = NULL; return NULL; }
  pv->pixels = NULL;
  napi_create_object(env, &o);
  set_num(env, o, "width", (double)pv->width);
  set_num(env, o, "height", (double)pv->height);
  napi_set_named_property(env, o, "data", buf);
  return o;
}

static napi_value stitch_result(napi_env env, stitch_job* j) {
  napi_value o, buf;
  napi_create_object(env, &o);
  const size_t bytes = (j->want_png || j->want_jpeg) ? (size_t)j->png_len : (size_t)j->plan.canvas_w * (size_t)j->plan.canvas_h * 4;
  if (napi_create_external_buffer(env, bytes, j->pixels, free_pixels, NULL, &buf) != napi_ok) { ist_free(j->pixels); if (j->want_preview) ist_free(j->pv.pixels); return NULL; }
  set_num(env, o, "width", (double)j->plan.canvas_w);
  set_num(env, o, "height", (double)j->plan.canvas_h);
  napi_set_named_property(env, o, j->want_jpeg ? "jpeg" : j->want_png ? "png" : "data", buf);
  if (j->want_preview && j->pv.pixels) { napi_value pv = preview_to_js(env, &j->pv); if (pv) napi_set_named_property(env, o, "preview", pv); }
  napi_set_named_property(env, o, "plan", plan_to_js(env, &j->plan));
  ist_plan_free(&j->plan);
  return o;
}

static void stitch_execute(napi_env env, void* data) {
  (void)env;
  stitch_job* j = (stitch_job*)data;
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  if (j->bitmaps) {
    j->rc = j->want_jpeg ? ist_stitch_bitmaps_jpeg(ctx, j->bitmaps, j->n_bitmaps, j->direction, j->mode, j->gap, &j->lim, j->filter, j->quality, j->subsampling,
                                                   &j->plan, &j->pixels, &j->png_len)
          : j->want_png ? ist_stitch_bitmaps_png_preview(ctx, j->bitmaps, j->n_bitmaps, j->direction, j->mode, j->gap, &j->lim, j->filter, &j->plan, &j->pixels, &j->png_len,
                                                         j->want_preview ? &j->pv : NULL)
                        : ist_stitch_bitmaps_rgba8(ctx, j->bitmaps, j->n_bitmaps, j->direction, j->mode, j->gap, &j->lim, j->filter, &j->plan, &j->pixels);
    if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
    return;
  }
  for (int i = 0; i < j->im.n; i++)
    if (!j->im.data[i]) { j->rc = IST_E_DECODE; snprintf(j->err, sizeof j->err, "\xe5\x9b\xbe\xe7\x89\x87%d\xe8\xa7\xa3\xe7\xa0\x81\xe5\xbc\x82\xe5\xb8\xb8", i); return; }
  if (j->want_jpeg)
    j->rc = ist_stitch_jpeg(ctx, j->im.descs, j->im.data, j->im.pitch, j->im.n, j->direction, j->mode, j->gap, &j->lim, j->filter, j->quality, j->subsampling,
                            &j->plan, &j->pixels, &j->png_len);
  else if (j->ndev > 0 && !j->want_png)
    j->rc = ist_stitch_rgba8_multi(j->devices, j->ndev, j->im.descs, j->im.data, j->im.pitch, j->im.n, j->direction, j->mode, j->gap, &j->lim,
                                   j->filter, j->split, &j->plan, &j->pixels);
  else if (j->want_png)
    j->rc = ist_stitch_png_preview(ctx, j->im.descs, j->im.data, j->im.pitch, j->im.n, j->direction, j->mode, j->gap, &j->lim,
                                   j->filter, &j->plan, &j->pixels, &j->png_len, j->want_preview ? &j->pv : NULL);
  else
    j->rc = ist_stitch_rgba8(ctx, j->im.descs, j->im.data, j->im.pitch, j->im.n, j->direction, j->mode, j->gap, &j->lim,
                             j->filter, &j->plan, &j->pixels);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
}

static napi_value make_error(napi_env env, int code, const char* why) {
  char msg[512], codebuf[16];
  strcpy(msg, "\xe6\x8b\xbc\xe5\x9b\xbe\xe5\xa4\xb1\xe8\xb4\xa5\xef\xbc\x9a");
  strncat(msg, why && *why ? why : "unknown", sizeof(msg) - strlen(msg) - 1);
  snprintf(codebuf, sizeof codebuf, "%d", code);
  napi_value m, c, e;
  napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &m);
  napi_create_string_utf8(env, codebuf, NAPI_AUTO_LENGTH, &c);
  napi_create_error(env, c, m, &e);
  return e;
}

static void stitch_complete(napi_env env, napi_status status, void* data) {
  stitch_job* j = (stitch_job*)data;
  (void)status;
  if (j->rc < 0) napi_reject_deferred(env, j->deferred, make_error(env, j->rc, j->err));
  else if (j->rc == IST_NOTHING_TO_DO) { napi_value u; napi_get_null(env, &u); napi_resolve_deferred(env, j->deferred, u); }
  else {
    napi_value r = stitch_result(env, j);
    if (r) napi_resolve_deferred(env, j->deferred, r);
    else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not wrap the output buffer"));
  }
  napi_delete_async_work(env, j->work);
  stitch_job_free(env, j);
}

static stitch_job* stitch_parse(napi_env env, napi_callback_info info, int want_refs) {
  size_t argc = 11; napi_value argv[11];
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 6) {
    napi_throw_type_error(env, NULL, "stitch(images, direction, mode, gap, limits, filter, asPng, devices, split, previewWidth, previewHeight)");
    return NULL;
  }
  stitch_job* j = (stitch_job*)calloc(1, sizeof *j);
  if (!images_parse(env, argv[0], &j->im, want_refs)) { images_free(env, &j->im); free(j); return NULL; }
  int32_t v = 0;
  napi_get_value_int32(env, argv[1], &v); j->direction = v;
  napi_get_value_int32(env, argv[2], &v); j->mode = v;
  napi_get_value_double(env, argv[3], &j->gap);
  limits_parse(env, argv[4], &j->lim);
  napi_get_value_int32(env, argv[5], &v); j->filter = v;
  if (argc > 6) { bool b = false; napi_get_value_bool(env, argv[6], &b); j->want_png = b ? 1 : 0; j->want_jpeg = jpeg_parse(env, argv[6], &j->quality, &j->subsampling); }
  if (argc > 7) {                                       /* devices: number[] */
    bool is_arr = false; uint32_t n = 0;
    if (napi_is_array(env, argv[7], &is_arr) == napi_ok && is_arr) {
      napi_get_array_length(env, argv[7], &n);
      if (n > 64) { napi_throw_range_error(env, NULL, "devices: at most 64 entries"); images_free(env, &j->im); free(j); return NULL; }
      for (uint32_t i = 0; i < n; i++) { napi_value e; int32_t d = -1; napi_get_element(env, argv[7], i, &e); napi_get_value_int32(env, e, &d); j->devices[i] = d; }
      j->ndev = (int)n;
    }
  }
  if (argc > 8) { napi_get_value_int32(env, argv[8], &v); j->split = v; }
  if (argc > 10 && j->want_png) j->want_preview = preview_parse(env, argv[9], argv[10], &j->pv);
  return j;
}

/* stitch(...) -> Promise: runs on the libuv pool, the event loop keeps turning (the reference yields between images
 * with `await _sleep(0)`, index.js:1567) */
static napi_value js_stitch(napi_env env, napi_callback_info info) {
  stitch_job* j = stitch_parse(env, info, 1);
  if (!j) return NULL;
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, "imagestitch.stitch", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, stitch_execute, stitch_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

/* stitchFiles(files: Buffer[], direction, mode, gap, limits, filter) -> Promise<{width,height,png,plan}>
 * the device-resident pipeline (ist_stitch_files_png): only file bytes go in, only PNG bytes come out */
typedef struct {
  int n; const uint8_t** files; int64_t* lens; napi_ref* refs;
  int direction, mode, filter; double gap; ist_limits lim;
  ist_plan plan; uint8_t* png; int64_t png_len; int rc; char err[256];
  int want_preview; ist_preview pv;
  napi_deferred deferred; napi_async_work work;
} files_job;

static void files_execute(napi_env env, void* data) {
  (void)env;
  files_job* j = (files_job*)data;
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  j->rc = ist_stitch_files_png_preview(ctx, j->files, j->lens, j->n, j->direction, j->mode, j->gap, &j->lim, j->filter, &j->plan, &j->png, &j->png_len,
                                       j->want_preview ? &j->pv : NULL);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
}

static void files_complete(napi_env env, napi_status status, void* data) {
  files_job* j = (files_job*)data;
  (void)status;
  if (j->rc < 0) napi_reject_deferred(env, j->deferred, make_error(env, j->rc, j->err));
  else if (j->rc == IST_NOTHING_TO_DO) { napi_value u; napi_get_null(env, &u); napi_resolve_deferred(env, j->deferred, u); }
  else {
    napi_value o, buf;
    napi_create_object(env, &o);
    if (napi_create_external_buffer(env, (size_t)j->png_len, j->png, free_pixels, NULL, &buf) != napi_ok) {
      ist_free(j->png); if (j->want_preview) ist_free(j->pv.pixels);
      napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not wrap the PNG buffer"));
    } else {
      if (j->want_preview && j->pv.pixels) { napi_value pv = preview_to_js(env, &j->pv); if (pv) napi_set_named_property(env, o, "preview", pv); }
      set_num(env, o, "width", (double)j->plan.canvas_w); set_num(env, o, "height", (double)j->plan.canvas_h);
      napi_set_named_property(env, o, "png", buf);
      napi_set_named_property(env, o, "plan", plan_to_js(env, &j->plan));
      napi_resolve_deferred(env, j->deferred, o);
    }
    ist_plan_free(&j->plan);
  }
  napi_delete_async_work(env, j->work);
  for (int i = 0; i < j->n; i++) if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
  free(j->files); free(j->lens); free(j->refs); free(j);
}

static napi_value js_stitch_files(napi_env env, napi_callback_info info) {
  size_t argc = 8; napi_value argv[8];
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 6) { napi_throw_type_error(env, NULL, "stitchFiles(files, direction, mode, gap, limits, filter, previewWidth, previewHeight)"); return NULL; }
  bool is_arr = false; uint32_t n = 0;
  if (napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) { napi_throw_type_error(env, NULL, "files must be an array of Buffers"); return NULL; }
  napi_get_array_length(env, argv[0], &n);
  files_job* j = (files_job*)calloc(1, sizeof *j);
  j->n = (int)n;
  j->files = (const uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*)); j->lens = (int64_t*)calloc(n ? n : 1, sizeof(int64_t)); j->refs = (napi_ref*)calloc(n ? n : 1, sizeof(napi_ref));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e; void* p = NULL; size_t len = 0; bool isbuf = false, ta = false;
    napi_get_element(env, argv[0], i, &e);
    napi_is_buffer(env, e, &isbuf); napi_is_typedarray(env, e, &ta);
    if (isbuf) napi_get_buffer_info(env, e, &p, &len);
    else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, e, &tt, &len, &p, &ab, &off); }
    if (!p) { napi_throw_type_error(env, NULL, "files[i] must be a Buffer / Uint8Array"); for (uint32_t k = 0; k < i; k++) napi_delete_reference(env, j->refs[k]); free(j->files); free(j->lens); free(j->refs); free(j); return NULL; }
    j->files[i] = (const uint8_t*)p; j->lens[i] = (int64_t)len;
    napi_create_reference(env, e, 1, &j->refs[i]);
  }
  int32_t v = 0;
  napi_get_value_int32(env, argv[1], &v); j->direction = v;
  napi_get_value_int32(env, argv[2], &v); j->mode = v;
  napi_get_value_double(env, argv[3], &j->gap);
  limits_parse(env, argv[4], &j->lim);
  napi_get_value_int32(env, argv[5], &v); j->filter = v;
  if (argc > 7) j->want_preview = preview_parse(env, argv[6], argv[7], &j->pv);
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, "imagestitch.stitchFiles", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, files_execute, files_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_stitch_sync(napi_env env, napi_callback_info info) {
  stitch_job* j = stitch_parse(env, info, 0);
  if (!j) return NULL;
  stitch_execute(env, j);
  napi_value out = NULL;
  if (j->rc < 0) { napi_throw(env, make_error(env, j->rc, j->err)); }
  else if (j->rc == IST_NOTHING_TO_DO) napi_get_null(env, &out);
  else out = stitch_result(env, j);
  stitch_job_free(env, j);
  return out;
}

/* render(canvasW, canvasH, clearRGBA(Uint8Array 4), ops(Float64Array 18/op), images, filter, region|null) -> Buffer */
/* stitchBatch(requests) / stitchBatchSync(requests): requests[k] = [images, direction, mode, gap, limits, filter] (what stitch takes, minus
 * the device-group arguments: a batch runs on one GPU).  N x Page.onStitch (index.js:1186-1633) through ist_stitch_rgba8_batch.
 * Result: an array with {width,height,data,plan} per request, null for a request without images. */
typedef struct {
  int n;
  images_t* im;
  ist_limits* lim;
  ist_stitch_request* reqs;
  ist_plan* plans;
  uint8_t** pixels;
  int want_png; int64_t* lens;            /* stitchPngBatch (1) / stitchJpegBatch (2): pixels[k] holds request k's file, lens[k] bytes */
  int* quality; int* subsampling;         /* stitchJpegBatch: requests[k][6], requests[k][7] */
  int rc; char err[256];
  napi_deferred deferred; napi_async_work work;
} batch_job;

static void batch_free(napi_env env, batch_job* j) {
  if (!j) return;
  for (int k = 0; k < j->n; k++) {
    if (j->im) images_free(env, &j->im[k]);
    if (j->plans) ist_plan_free(&j->plans[k]);
    if (j->pixels && j->pixels[k]) ist_free(j->pixels[k]);
  }
  free(j->im); free(j->lim); free(j->reqs); free(j->plans); free(j->pixels); free(j->lens); free(j->quality); free(j->subsampling); free(j);
}

static batch_job* batch_parse(napi_env env, napi_callback_info info, int want_refs) {
  size_t argc = 1; napi_value argv[1];
  bool is_arr = false; uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "stitchBatch([[images, direction, mode, gap, limits, filter], ...])");
    return NULL;
  }
  napi_get_array_length(env, argv[0], &n);
  batch_job* j = (batch_job*)calloc(1, sizeof *j);
  j->n = (int)n;
  j->im = (images_t*)calloc(n ? n : 1, sizeof(images_t));
  j->lim = (ist_limits*)calloc(n ? n : 1, sizeof(ist_limits));
  j->reqs = (ist_stitch_request*)calloc(n ? n : 1, sizeof(ist_stitch_request));
  j->plans = (ist_plan*)calloc(n ? n : 1, sizeof(ist_plan));
  j->pixels = (uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*));
  j->lens = (int64_t*)calloc(n ? n : 1, sizeof(int64_t));
  j->quality = (int*)calloc(n ? n : 1, sizeof(int));
  j->subsampling = (int*)calloc(n ? n : 1, sizeof(int));
  for (uint32_t k = 0; k < n; k++) {
    napi_value r, a[6]; bool ra = false; uint32_t m = 0;
    napi_get_element(env, argv[0], k, &r);
    if (napi_is_array(env, r, &ra) != napi_ok || !ra || napi_get_array_length(env, r, &m) != napi_ok || m < 6) {
      napi_throw_type_error(env, NULL, "stitchBatch: requests[k] must be [images, direction, mode, gap, limits, filter]");
      batch_free(env, j); return NULL;
    }
    for (uint32_t i = 0; i < 6; i++) napi_get_element(env, r, i, &a[i]);
    if (!images_parse(env, a[0], &j->im[k], want_refs)) { batch_free(env, j); return NULL; }
    ist_stitch_request* q = &j->reqs[k];
    int32_t v = 0;
    napi_get_value_int32(env, a[1], &v); q->direction = v;
    napi_get_value_int32(env, a[2], &v); q->mode = v;
    napi_get_value_double(env, a[3], &q->gap);
    limits_parse(env, a[4], &j->lim[k]);
    napi_get_value_int32(env, a[5], &v); q->filter = v;
    j->quality[k] = 90; j->subsampling[k] = IST_JPEG_420;
    if (m >= 8) {
      napi_value e;
      napi_get_element(env, r, 6, &e); if (napi_get_value_int32(env, e, &v) == napi_ok) j->quality[k] = v;
      napi_get_element(env, r, 7, &e); if (napi_get_value_int32(env, e, &v) == napi_ok) j->subsampling[k] = v;
    }
    q->images = j->im[k].descs; q->src = j->im[k].data; q->src_pitch = j->im[k].pitch; q->n_images = j->im[k].n; q->limits = &j->lim[k];
  }
  return j;
}

static void batch_execute(napi_env env, void* data) {
  (void)env;
  batch_job* j = (batch_job*)data;
  if (j->n == 0) { j->rc = IST_OK; return; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  for (int k = 0; k < j->n; k++)
    for (int i = 0; i < j->im[k].n; i++)
      if (!j->im[k].data[i]) {
        j->rc = IST_E_DECODE;
        snprintf(j->err, sizeof j->err, "request %d: \xe5\x9b\xbe\xe7\x89\x87%d\xe8\xa7\xa3\xe7\xa0\x81\xe5\xbc\x82\xe5\xb8\xb8", k, i);
        return;
      }
  j->rc = j->want_png == 2 ? ist_stitch_jpeg_batch(ctx, j->reqs, j->n, j->quality, j->subsampling, j->plans, j->pixels, j->lens)
          : j->want_png  ? ist_stitch_png_batch(ctx, j->reqs, j->n, j->plans, j->pixels, j->lens)
                         : ist_stitch_rgba8_batch(ctx, j->reqs, j->n, j->plans, j->pixels);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
}

/* the results array; the pixel blocks move into external Buffers (freed by ist_free when they are collected) */
static napi_value batch_result(napi_env env, batch_job* j) {
  napi_value arr;
  if (napi_create_array_with_length(env, (size_t)j->n, &arr) != napi_ok) return NULL;
  for (int k = 0; k < j->n; k++) {
    napi_value e;
    if (!j->pixels[k]) { napi_get_null(env, &e); napi_set_element(env, arr, (uint32_t)k, e); continue; }
    const ist_plan* p = &j->plans[k];
    napi_value buf;
    const size_t bytes = j->want_png ? (size_t)j->lens[k] : (size_t)p->canvas_w * (size_t)p->canvas_h * 4;
    if (napi_create_external_buffer(env, bytes, j->pixels[k], free_pixels, NULL, &buf) != napi_ok) return NULL;
    j->pixels[k] = NULL;                                  /* the Buffer owns it now */
    napi_create_object(env, &e);
    set_num(env, e, "width", (double)p->canvas_w);
    set_num(env, e, "height", (double)p->canvas_h);
    napi_set_named_property(env, e, j->want_png == 2 ? "jpeg" : j->want_png ? "png" : "data", buf);
    napi_set_named_property(env, e, "plan", plan_to_js(env, p));
    napi_set_element(env, arr, (uint32_t)k, e);
  }
  return arr;
}

static void batch_complete(napi_env env, napi_status status, void* data) {
  batch_job* j = (batch_job*)data;
  (void)status;
  if (j->rc < 0) napi_reject_deferred(env, j->deferred, make_error(env, j->rc, j->err));
  else {
    napi_value r = batch_result(env, j);
    if (r) napi_resolve_deferred(env, j->deferred, r);
    else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not wrap the output buffers"));
  }
  napi_delete_async_work(env, j->work);
  batch_free(env, j);
}

static napi_value batch_async(napi_env env, napi_callback_info info, int want_png) {
  batch_job* j = batch_parse(env, info, 1);
  if (!j) return NULL;
  j->want_png = want_png;
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, want_png == 2 ? "imagestitch.stitchJpegBatch" : want_png ? "imagestitch.stitchPngBatch" : "imagestitch.stitchBatch", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, batch_execute, batch_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value batch_sync(napi_env env, napi_callback_info info, int want_png) {
  batch_job* j = batch_parse(env, info, 0);
  if (!j) return NULL;
  j->want_png = want_png;
  batch_execute(env, j);
  napi_value out = NULL;
  if (j->rc < 0) napi_throw(env, make_error(env, j->rc, j->err));
  else {
    out = batch_result(env, j);
    if (!out) napi_throw(env, make_error(env, IST_E_NOMEM, "could not wrap the output buffers"));
  }
  batch_free(env, j);
  return out;
}

static napi_value js_stitch_batch(napi_env env, napi_callback_info info) { return batch_async(env, info, 0); }
static napi_value js_stitch_batch_sync(napi_env env, napi_callback_info info) { return batch_sync(env, info, 0); }
/* stitchPngBatch / stitchPngBatchSync: the same requests, a PNG file per request (the form setPngLevel chose) */
static napi_value js_stitch_png_batch(napi_env env, napi_callback_info info) { return batch_async(env, info, 1); }
static napi_value js_stitch_png_batch_sync(napi_env env, napi_callback_info info) { return batch_sync(env, info, 1); }
/* stitchJpegBatch / stitchJpegBatchSync: requests[k] = [..., quality, subsampling], a JPEG file per request (ist_stitch_jpeg_batch) */
static napi_value js_stitch_jpeg_batch(napi_env env, napi_callback_info info) { return batch_async(env, info, 2); }
static napi_value js_stitch_jpeg_batch_sync(napi_env env, napi_callback_info info) { return batch_sync(env, info, 2); }

static napi_value js_render(napi_env env, napi_callback_info info) {
  size_t argc = 8; napi_value argv[8];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 6) { napi_throw_type_error(env, NULL, "render(canvasW, canvasH, clear, ops, images, filter, region)"); return NULL; }
  double cw = 0, ch = 0; int32_t filter = 1;
  napi_get_value_double(env, argv[0], &cw);
  napi_get_value_double(env, argv[1], &ch);
  uint8_t clear[4] = {0, 0, 0, 0};
  { bool ta = false; napi_is_typedarray(env, argv[2], &ta);
    if (ta) { napi_typedarray_type tt; size_t len; void* p; napi_value ab; size_t off;
      napi_get_typedarray_info(env, argv[2], &tt, &len, &p, &ab, &off);
      if (len >= 4 && p) memcpy(clear, p, 4); } }
  napi_typedarray_type tt; size_t len = 0; void* p = NULL; napi_value ab; size_t off;
  bool ta = false; napi_is_typedarray(env, argv[3], &ta);
  if (!ta) { napi_throw_type_error(env, NULL, "ops must be a Float64Array"); return NULL; }
  napi_get_typedarray_info(env, argv[3], &tt, &len, &p, &ab, &off);
  if (tt != napi_float64_array || len % 18) { napi_throw_type_error(env, NULL, "ops must be a Float64Array with 18 doubles per op"); return NULL; }
  const int n_ops = (int)(len / 18);
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
  images_t im;
  if (!images_parse(env, argv[4], &im, 0)) { images_free(env, &im); free(ops); return NULL; }
  napi_get_value_int32(env, argv[5], &filter);
  ist_region reg = {0, 0, (int32_t)cw, (int32_t)ch};
  int have_region = 0;
  if (argc > 6) {
    napi_valuetype t; napi_typeof(env, argv[6], &t);
    if (t == napi_object) {
      int64_t v;
      if (get_named_i64(env, argv[6], "x", &v)) reg.x = (int32_t)v;
      if (get_named_i64(env, argv[6], "y", &v)) reg.y = (int32_t)v;
      if (get_named_i64(env, argv[6], "w", &v)) reg.w = (int32_t)v;
      if (get_named_i64(env, argv[6], "h", &v)) reg.h = (int32_t)v;
      have_region = 1;
    }
  }
  if (reg.w < 1 || reg.h < 1) { images_free(env, &im); free(ops); napi_throw_range_error(env, NULL, "empty region"); return NULL; }
  if (argc > 7) {                 /* asPng: wx.canvasToTempFilePath({fileType:'png'}) - the canvas stays on the device */
    bool as_png = false; napi_get_value_bool(env, argv[7], &as_png);
    if (as_png) {
      uint8_t* png = NULL; int64_t len = 0;
      ist_ctx* c2 = get_ctx();
      int rc2 = c2 ? ist_render_png(c2, (int64_t)cw, (int64_t)ch, clear, ops, n_ops, im.descs, im.data, im.pitch, im.n, filter, &png, &len)
                   : IST_E_NO_DEVICE;
      images_free(env, &im); free(ops);
      if (rc2 == IST_E_NO_DEVICE && !c2) { napi_throw(env, make_error(env, rc2, g_ctx_err)); return NULL; }
      if (rc2 < 0) return throw_ist(env, rc2);
      napi_value buf;
      if (napi_create_external_buffer(env, (size_t)len, png, free_pixels, NULL, &buf) != napi_ok) { ist_free(png); napi_throw_error(env, NULL, "out of memory"); return NULL; }
      return buf;
    }
  }
  const size_t bytes = (size_t)reg.w * (size_t)reg.h * 4;
  void* out_data = NULL; napi_value out;
  if (napi_create_buffer(env, bytes, &out_data, &out) != napi_ok) { images_free(env, &im); free(ops); napi_throw_error(env, NULL, "out of memory"); return NULL; }
  ist_ctx* ctx = get_ctx();
  int rc = ctx ? ist_render_rgba8(ctx, (int64_t)cw, (int64_t)ch, clear, ops, n_ops, im.descs, im.data, im.pitch, im.n, filter,
                                  have_region ? &reg : NULL, (uint8_t*)out_data, (size_t)reg.w * 4)
               : IST_E_NO_DEVICE;
  images_free(env, &im); free(ops);
  if (rc == IST_E_NO_DEVICE && !ctx) { napi_throw(env, make_error(env, rc, g_ctx_err)); return NULL; }
  if (rc < 0) return throw_ist(env, rc);
  return out;
}

/* encodePng(data: Uint8Array RGBA, width, height) -> Buffer (PNG file bytes) */
static napi_value js_encode_png(napi_env env, napi_callback_info info) {
  size_t argc = 3; napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "encodePng(data, width, height)"); return NULL; }
  bool ta = false, isbuf = false; void* p = NULL; size_t len = 0;
  napi_is_buffer(env, argv[0], &isbuf); napi_is_typedarray(env, argv[0], &ta);
  if (isbuf) napi_get_buffer_info(env, argv[0], &p, &len);
  else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, argv[0], &tt, &len, &p, &ab, &off); }
  double w = 0, h = 0;
  napi_get_value_double(env, argv[1], &w); napi_get_value_double(env, argv[2], &h);
  if (!p || w < 1 || h < 1 || (double)len < w * h * 4) { napi_throw_range_error(env, NULL, "data is smaller than width*height*4"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  uint8_t* png = NULL; int64_t n = 0;
  const int rc = ist_png_encode_rgba8(ctx, (const uint8_t*)p, (size_t)w * 4, (int64_t)w, (int64_t)h, &png, &n);
  if (rc < 0) return throw_ist(env, rc);
  napi_value buf;
  if (napi_create_external_buffer(env, (size_t)n, png, free_pixels, NULL, &buf) != napi_ok) { ist_free(png); napi_throw_error(env, NULL, "out of memory"); return NULL; }
  return buf;
}

/* encodeJpeg(data: Uint8Array RGBA, width, height, quality, subsampling: IST_JPEG_*) -> Buffer (JFIF file bytes; alpha is not read) */
static napi_value js_encode_jpeg(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 5) { napi_throw_type_error(env, NULL, "encodeJpeg(data, width, height, quality, subsampling)"); return NULL; }
  bool ta = false, isbuf = false; void* p = NULL; size_t len = 0;
  napi_is_buffer(env, argv[0], &isbuf); napi_is_typedarray(env, argv[0], &ta);
  if (isbuf) napi_get_buffer_info(env, argv[0], &p, &len);
  else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, argv[0], &tt, &len, &p, &ab, &off); }
  double w = 0, h = 0; int32_t quality = 0, subsampling = -1;
  napi_get_value_double(env, argv[1], &w); napi_get_value_double(env, argv[2], &h);
  napi_get_value_int32(env, argv[3], &quality); napi_get_value_int32(env, argv[4], &subsampling);
  if (!p || w < 1 || h < 1 || (double)len < w * h * 4) { napi_throw_range_error(env, NULL, "data is smaller than width*height*4"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  uint8_t* jpg = NULL; int64_t n = 0;
  const int rc = ist_jpeg_encode_rgba8(ctx, (const uint8_t*)p, (size_t)w * 4, (int64_t)w, (int64_t)h, quality, subsampling, &jpg, &n);
  if (rc < 0) return throw_ist(env, rc);
  napi_value buf;
  if (napi_create_external_buffer(env, (size_t)n, jpg, free_pixels, NULL, &buf) != napi_ok) { ist_free(jpg); napi_throw_error(env, NULL, "out of memory"); return NULL; }
  return buf;
}

/* decodeImage(file: Buffer) -> {width, height, orientation, data}: PNG (host) or JPEG (host Huffman + GPU reconstruction) */
static napi_value js_decode_image(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool ta = false, isbuf = false; void* p = NULL; size_t len = 0;
  if (argc < 1) { napi_throw_type_error(env, NULL, "decodeImage(buffer)"); return NULL; }
  napi_is_buffer(env, argv[0], &isbuf); napi_is_typedarray(env, argv[0], &ta);
  if (isbuf) napi_get_buffer_info(env, argv[0], &p, &len);
  else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, argv[0], &tt, &len, &p, &ab, &off); }
  if (!p) { napi_throw_type_error(env, NULL, "decodeImage expects a Buffer / Uint8Array"); return NULL; }
  int32_t w = 0, h = 0, orient = 0;
  int rc = ist_image_info((const uint8_t*)p, (int64_t)len, &w, &h, &orient);
  if (rc < 0) return throw_ist(env, rc);
  const int is_jpeg = len >= 2 && ((const uint8_t*)p)[0] == 0xFF && ((const uint8_t*)p)[1] == 0xD8;
  ist_ctx* ctx = is_jpeg ? get_ctx() : NULL;
  if (is_jpeg && !ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  void* out_data = NULL; napi_value buf, o;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  rc = ist_image_decode_rgba8(ctx, (const uint8_t*)p, (int64_t)len, (uint8_t*)out_data, (size_t)w * 4, (int64_t)h);
  if (rc < 0) return throw_ist(env, rc);
  napi_create_object(env, &o);
  set_num(env, o, "width", w); set_num(env, o, "height", h); set_num(env, o, "orientation", orient ? orient : 1);
  napi_value op; napi_get_boolean(env, is_jpeg != 0, &op); napi_set_named_property(env, o, "opaque", op);
  napi_set_named_property(env, o, "data", buf);
  return o;
}

/* decodePng(file: Buffer) -> {width, height, data: Buffer RGBA8}   (host decode, no GPU needed) */
static napi_value js_decode_png(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool ta = false, isbuf = false; void* p = NULL; size_t len = 0;
  if (argc < 1) { napi_throw_type_error(env, NULL, "decodePng(buffer)"); return NULL; }
  napi_is_buffer(env, argv[0], &isbuf); napi_is_typedarray(env, argv[0], &ta);
  if (isbuf) napi_get_buffer_info(env, argv[0], &p, &len);
  else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, argv[0], &tt, &len, &p, &ab, &off); }
  if (!p) { napi_throw_type_error(env, NULL, "decodePng expects a Buffer / Uint8Array"); return NULL; }
  int32_t w = 0, h = 0;
  int rc = ist_png_info((const uint8_t*)p, (int64_t)len, &w, &h);
  if (rc < 0) return throw_ist(env, rc);
  void* out_data = NULL; napi_value buf, o;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  rc = ist_png_decode_rgba8((const uint8_t*)p, (int64_t)len, (uint8_t*)out_data, (size_t)w * 4, (int64_t)h);
  if (rc < 0) return throw_ist(env, rc);
  napi_create_object(env, &o);
  set_num(env, o, "width", w); set_num(env, o, "height", h);
  napi_set_named_property(env, o, "data", buf);
  return o;
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

/* setPngLevel(level): 0 stored deflate blocks, 1 compressed on the GPU (ist_ctx_set_png_level) - applies to every PNG
 * this process exports afterwards */
static napi_value js_set_png_level(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t level = 0;
  if (argc < 1 || napi_get_value_int32(env, argv[0], &level) != napi_ok) { napi_throw_type_error(env, NULL, "setPngLevel(level)"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  const int rc = ist_ctx_set_png_level(ctx, level);
  if (rc < 0) return throw_ist(env, rc);
  napi_value v; napi_get_undefined(env, &v); return v;
}

/* setPngColor(color): 0 RGBA (colour type 6), 1 RGB (colour type 2, alpha not read; level 1 only) - ist_ctx_set_png_color; applies
 * to every PNG this process exports afterwards */
static napi_value js_set_png_color(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t color = 0;
  if (argc < 1 || napi_get_value_int32(env, argv[0], &color) != napi_ok) { napi_throw_type_error(env, NULL, "setPngColor(color)"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  const int rc = ist_ctx_set_png_color(ctx, color);
  if (rc < 0) return throw_ist(env, rc);
  napi_value v; napi_get_undefined(env, &v); return v;
}

/* ---- resident bitmaps --------------------------------------------------------------------------------------------------- */
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
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) { napi_throw_type_error(env, NULL, "uploadBitmap([image])"); return NULL; }
  images_t im;
  if (!images_parse(env, argv[0], &im, 0)) { images_free(env, &im); return NULL; }
  if (im.n != 1) { images_free(env, &im); napi_throw_type_error(env, NULL, "uploadBitmap takes one image"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { images_free(env, &im); napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  ist_bitmap* b = ist_bitmap_upload(ctx, &im.descs[0], im.data[0], im.pitch[0]);
  images_free(env, &im);
  if (!b) return throw_ist(env, upload_fail_code());
  napi_value h = bitmap_wrap(env, b);
  if (!h) napi_throw_error(env, NULL, "could not wrap the bitmap");
  return h;
}

/* decodeBitmaps(files: Buffer[]) -> Promise<handle[]> (ist_bitmaps_decode: all or nothing) */
typedef struct {
  int n; const uint8_t** files; int64_t* lens; napi_ref* refs;
  ist_bitmap** out; int rc; char err[256];
  napi_deferred deferred; napi_async_work work;
} decode_job;

static void decode_job_free(napi_env env, decode_job* j) {
  for (int i = 0; i < j->n; i++) {
    if (j->refs[i]) napi_delete_reference(env, j->refs[i]);
    if (j->out[i]) ist_bitmap_release(j->out[i]);
  }
  free(j->files); free(j->lens); free(j->refs); free(j->out); free(j);
}

static void decode_execute(napi_env env, void* data) {
  (void)env;
  decode_job* j = (decode_job*)data;
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  j->rc = j->n ? ist_bitmaps_decode(ctx, j->files, j->lens, j->n, j->out) : IST_OK;
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
}

static void decode_complete(napi_env env, napi_status status, void* data) {
  decode_job* j = (decode_job*)data;
  (void)status;
  napi_value arr = NULL;
  if (j->rc < 0) napi_reject_deferred(env, j->deferred, make_error(env, j->rc, j->err));
  else if (napi_create_array_with_length(env, (size_t)j->n, &arr) == napi_ok) {
    int ok = 1;
    for (int i = 0; i < j->n && ok; i++) {
      napi_value h = bitmap_wrap(env, j->out[i]);
      j->out[i] = NULL;                                   /* the handle owns the reference now (or released it) */
      ok = h && napi_set_element(env, arr, (uint32_t)i, h) == napi_ok;
    }
    if (ok) napi_resolve_deferred(env, j->deferred, arr);
    else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not wrap the bitmaps"));
  } else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not make the result array"));
  napi_delete_async_work(env, j->work);
  decode_job_free(env, j);
}

static napi_value js_decode_bitmaps(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  bool is_arr = false; uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 1 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "decodeBitmaps(files: Buffer[])"); return NULL;
  }
  napi_get_array_length(env, argv[0], &n);
  decode_job* j = (decode_job*)calloc(1, sizeof *j);
  j->n = (int)n;
  j->files = (const uint8_t**)calloc(n ? n : 1, sizeof(uint8_t*)); j->lens = (int64_t*)calloc(n ? n : 1, sizeof(int64_t));
  j->refs = (napi_ref*)calloc(n ? n : 1, sizeof(napi_ref)); j->out = (ist_bitmap**)calloc(n ? n : 1, sizeof(ist_bitmap*));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e; void* p = NULL; size_t len = 0; bool isbuf = false, ta = false;
    napi_get_element(env, argv[0], i, &e);
    napi_is_buffer(env, e, &isbuf); napi_is_typedarray(env, e, &ta);
    if (isbuf) napi_get_buffer_info(env, e, &p, &len);
    else if (ta) { napi_typedarray_type tt; napi_value ab; size_t off; napi_get_typedarray_info(env, e, &tt, &len, &p, &ab, &off); }
    if (!p) { napi_throw_type_error(env, NULL, "files[i] must be a Buffer / Uint8Array"); decode_job_free(env, j); return NULL; }
    j->files[i] = (const uint8_t*)p; j->lens[i] = (int64_t)len;
    napi_create_reference(env, e, 1, &j->refs[i]);
  }
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, "imagestitch.decodeBitmaps", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, decode_execute, decode_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_bitmap_desc(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) { napi_throw_type_error(env, NULL, "bitmapDesc(handle)"); return NULL; }
  ist_bitmap* b = bitmap_of(env, argv[0]);
  if (!b) return NULL;
  ist_image_desc d;
  const int rc = ist_bitmap_desc(b, &d);
  if (rc < 0) return throw_ist(env, rc);
  napi_value o, op;
  napi_create_object(env, &o);
  set_num(env, o, "width", d.width); set_num(env, o, "height", d.height); set_num(env, o, "orientation", d.orientation);
  set_num(env, o, "bmpWidth", d.bmp_width > 0 ? d.bmp_width : d.width); set_num(env, o, "bmpHeight", d.bmp_height > 0 ? d.bmp_height : d.height);
  napi_get_boolean(env, d.opaque != 0, &op); napi_set_named_property(env, o, "opaque", op);
  set_num(env, o, "fileSize", (double)d.file_size);
  return o;
}

/* bitmapDownload(handle) -> Buffer (bmpWidth * bmpHeight * 4 bytes, dense rows) */
static napi_value js_bitmap_download(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) { napi_throw_type_error(env, NULL, "bitmapDownload(handle)"); return NULL; }
  ist_bitmap* b = bitmap_of(env, argv[0]);
  if (!b) return NULL;
  ist_image_desc d;
  ist_bitmap_desc(b, &d);
  const int64_t w = d.bmp_width > 0 ? d.bmp_width : d.width, h = d.bmp_height > 0 ? d.bmp_height : d.height;
  void* out_data = NULL; napi_value buf;
  if (napi_create_buffer(env, (size_t)w * (size_t)h * 4, &out_data, &buf) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  const int rc = ist_bitmap_download(b, (uint8_t*)out_data, (size_t)w * 4, h);
  if (rc < 0) return throw_ist(env, rc);
  return buf;
}

/* bitmapPreview(handle, boxWidth, boxHeight) -> {width, height, data}: the stored pixels shrunk to fit the box (ist_preview_fit, then
 * ist_bitmap_preview: reduced in GPU memory, only the preview crosses PCIe) */
static napi_value js_bitmap_preview(napi_env env, napi_callback_info info) {
  size_t argc = 3; napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "bitmapPreview(handle, width, height)"); return NULL; }
  ist_bitmap* b = bitmap_of(env, argv[0]);
  if (!b) return NULL;
  ist_preview pv;
  if (!preview_parse(env, argv[1], argv[2], &pv)) { napi_throw_type_error(env, NULL, "bitmapPreview(handle, width, height): the box sides must be numbers"); return NULL; }
  ist_ctx* ctx = get_ctx();
  if (!ctx) { napi_throw(env, make_error(env, IST_E_NO_DEVICE, g_ctx_err)); return NULL; }
  ist_image_desc d;
  ist_bitmap_desc(b, &d);
  int rc = ist_preview_fit(d.bmp_width > 0 ? d.bmp_width : d.width, d.bmp_height > 0 ? d.bmp_height : d.height, pv.box_w, pv.box_h, &pv.width, &pv.height);
  if (rc < 0) return throw_ist(env, rc);
  void* out_data = NULL; napi_value buf, o;
  if (napi_create_buffer(env, (size_t)pv.width * (size_t)pv.height * 4, &out_data, &buf) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  rc = ist_bitmap_preview(ctx, b, pv.width, pv.height, (uint8_t*)out_data, (size_t)pv.width * 4);
  if (rc < 0) return throw_ist(env, rc);
  napi_create_object(env, &o);
  set_num(env, o, "width", (double)pv.width);
  set_num(env, o, "height", (double)pv.height);
  napi_set_named_property(env, o, "data", buf);
  return o;
}

/* thumbnails(handles, cellWidth, cellHeight, mode, orient) -> Promise<[{width, height, data}]> (ist_bitmaps_thumbs: the grid of chosen
 * images, index.wxml:4-22 - every bitmap cropped or fitted, turned and shrunk in one launch pair per form, one copy down).  Every
 * data Buffer is a view of ONE pinned block, given back to the pool when the last of them is collected.  The bitmaps are retained
 * HERE, on the JS thread, as stitchBitmaps retains them. */
typedef struct {
  int n; ist_bitmap** bitmaps; ist_thumb_spec spec; ist_thumb_item* items; uint8_t* pixels;
  int rc; char err[256];
  napi_deferred deferred; napi_async_work work;
} thumbs_job;
typedef struct { uint8_t* pixels; int live; } thumbs_block;

static void thumbs_job_free(thumbs_job* j) {
  for (int i = 0; i < j->n; i++) if (j->bitmaps[i]) ist_bitmap_release(j->bitmaps[i]);
  if (j->pixels) ist_free(j->pixels);
  free(j->bitmaps); free(j->items); free(j);
}

static void thumbs_view_gone(napi_env env, void* data, void* hint) {
  (void)env; (void)data;
  thumbs_block* blk = (thumbs_block*)hint;               /* (finalizers run on the JS thread: no lock) */
  if (--blk->live == 0) { ist_free(blk->pixels); free(blk); }
}

static void thumbs_execute(napi_env env, void* data) {
  (void)env;
  thumbs_job* j = (thumbs_job*)data;
  ist_ctx* ctx = get_ctx();
  if (!ctx) { j->rc = IST_E_NO_DEVICE; snprintf(j->err, sizeof j->err, "%s", g_ctx_err); return; }
  j->rc = ist_bitmaps_thumbs(ctx, j->bitmaps, j->n, &j->spec, j->items, &j->pixels);
  if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", ist_last_error());
}

static void thumbs_complete(napi_env env, napi_status status, void* data) {
  thumbs_job* j = (thumbs_job*)data;
  (void)status;
  napi_value arr = NULL;
  if (j->rc < 0) napi_reject_deferred(env, j->deferred, make_error(env, j->rc, j->err));
  else if (napi_create_array_with_length(env, (size_t)j->n, &arr) == napi_ok) {
    thumbs_block* blk = (thumbs_block*)calloc(1, sizeof *blk);
    blk->pixels = j->pixels; blk->live = 1;               /* (this function's own hold, dropped below) */
    j->pixels = NULL;
    int ok = 1;
    for (int i = 0; i < j->n && ok; i++) {
      const ist_thumb_item* t = &j->items[i];
      napi_value o, buf;
      blk->live++;
      if (napi_create_external_buffer(env, (size_t)t->width * (size_t)t->height * 4, blk->pixels + t->offset, thumbs_view_gone, blk, &buf) != napi_ok) { blk->live--; ok = 0; break; }
      napi_create_object(env, &o);
      set_num(env, o, "width", (double)t->width);
      set_num(env, o, "height", (double)t->height);
      napi_set_named_property(env, o, "data", buf);
      ok = napi_set_element(env, arr, (uint32_t)i, o) == napi_ok;
    }
    if (--blk->live == 0) { ist_free(blk->pixels); free(blk); }
    if (ok) napi_resolve_deferred(env, j->deferred, arr);
    else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not wrap the thumbnails"));
  } else napi_reject_deferred(env, j->deferred, make_error(env, IST_E_NOMEM, "could not make the result array"));
  napi_delete_async_work(env, j->work);
  thumbs_job_free(j);
}

static napi_value js_thumbnails(napi_env env, napi_callback_info info) {
  size_t argc = 5; napi_value argv[5];
  bool is_arr = false; uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 5 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "thumbnails(bitmaps, cellWidth, cellHeight, mode, orient)"); return NULL;
  }
  napi_get_array_length(env, argv[0], &n);
  thumbs_job* j = (thumbs_job*)calloc(1, sizeof *j);
  j->bitmaps = (ist_bitmap**)calloc(n ? n : 1, sizeof(ist_bitmap*));
  j->items = (ist_thumb_item*)calloc(n ? n : 1, sizeof(ist_thumb_item));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e; napi_valuetype t = napi_undefined;
    napi_get_element(env, argv[0], i, &e);
    napi_typeof(env, e, &t);
    j->n = (int)i + 1;
    if (t == napi_null || t == napi_undefined) continue;   /* a missing image: '图片N解码异常' from the library */
    ist_bitmap* b = bitmap_of(env, e);
    if (!b) { thumbs_job_free(j); return NULL; }
    ist_bitmap_retain(b);
    j->bitmaps[i] = b;
  }
  double w = 0, h = 0; int32_t v = 0; bool orient = true;
  napi_get_value_double(env, argv[1], &w); napi_get_value_double(env, argv[2], &h);
  j->spec.cell_w = w >= 1 && w <= 2147483647.0 ? (int32_t)w : 0;      /* (0: the library's 'the cell must be at least 1 x 1') */
  j->spec.cell_h = h >= 1 && h <= 2147483647.0 ? (int32_t)h : 0;
  napi_get_value_int32(env, argv[3], &v); j->spec.mode = v;
  napi_get_value_bool(env, argv[4], &orient); j->spec.apply_orientation = orient ? 1 : 0;
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, "imagestitch.thumbnails", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, thumbs_execute, thumbs_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

/* bitmapRelease(handle): drops the handle's reference (a released handle: nothing) */
static napi_value js_bitmap_release(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) { napi_throw_type_error(env, NULL, "bitmapRelease(handle)"); return NULL; }
  bitmap_ref* r = bitmap_ref_of(env, argv[0]);
  if (!r) return NULL;
  if (r->b) { ist_bitmap_release(r->b); r->b = NULL; }
  napi_value u; napi_get_undefined(env, &u); return u;
}

/* stitchBitmaps(handles, direction, mode, gap, limits, filter, asPng): every bitmap is retained HERE, on the JS thread, so that a
 * release() or a collection between this call and the work's execution cannot free it */
static stitch_job* stitch_bitmaps_parse(napi_env env, napi_callback_info info) {
  size_t argc = 9; napi_value argv[9];
  bool is_arr = false; uint32_t n = 0;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 6 || napi_is_array(env, argv[0], &is_arr) != napi_ok || !is_arr) {
    napi_throw_type_error(env, NULL, "stitchBitmaps(bitmaps, direction, mode, gap, limits, filter, asPng, previewWidth, previewHeight)");
    return NULL;
  }
  napi_get_array_length(env, argv[0], &n);
  stitch_job* j = (stitch_job*)calloc(1, sizeof *j);
  j->bitmaps = (ist_bitmap**)calloc(n ? n : 1, sizeof(ist_bitmap*));
  for (uint32_t i = 0; i < n; i++) {
    napi_value e; napi_valuetype t = napi_undefined;
    napi_get_element(env, argv[0], i, &e);
    napi_typeof(env, e, &t);
    if (t == napi_null || t == napi_undefined) { j->n_bitmaps = (int)i + 1; continue; }   /* a missing image: '图片N解码异常' from the library */
    ist_bitmap* b = bitmap_of(env, e);
    if (!b) { stitch_job_free(env, j); return NULL; }
    ist_bitmap_retain(b);
    j->bitmaps[i] = b;
    j->n_bitmaps = (int)i + 1;
  }
  int32_t v = 0;
  napi_get_value_int32(env, argv[1], &v); j->direction = v;
  napi_get_value_int32(env, argv[2], &v); j->mode = v;
  napi_get_value_double(env, argv[3], &j->gap);
  limits_parse(env, argv[4], &j->lim);
  napi_get_value_int32(env, argv[5], &v); j->filter = v;
  if (argc > 6) { bool b = false; napi_get_value_bool(env, argv[6], &b); j->want_png = b ? 1 : 0; j->want_jpeg = jpeg_parse(env, argv[6], &j->quality, &j->subsampling); }
  if (argc > 8 && j->want_png) j->want_preview = preview_parse(env, argv[7], argv[8], &j->pv);
  return j;
}

static napi_value js_stitch_bitmaps(napi_env env, napi_callback_info info) {
  stitch_job* j = stitch_bitmaps_parse(env, info);
  if (!j) return NULL;
  napi_value promise, name;
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  napi_create_string_utf8(env, "imagestitch.stitchBitmaps", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_async_work(env, NULL, name, stitch_execute, stitch_complete, j, &j->work));
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_stitch_bitmaps_sync(napi_env env, napi_callback_info info) {
  stitch_job* j = stitch_bitmaps_parse(env, info);
  if (!j) return NULL;
  stitch_execute(env, j);
  napi_value out = NULL;
  if (j->rc < 0) napi_throw(env, make_error(env, j->rc, j->err));
  else if (j->rc == IST_NOTHING_TO_DO) napi_get_null(env, &out);
  else out = stitch_result(env, j);
  stitch_job_free(env, j);
  return out;
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
      {"decodePng", NULL, js_decode_png, NULL, NULL, NULL, napi_default, NULL},
      {"decodeImage", NULL, js_decode_image, NULL, NULL, NULL, napi_default, NULL},
      {"deviceCount", NULL, js_device_count, NULL, NULL, NULL, napi_default, NULL},
      {"lastError", NULL, js_last_error, NULL, NULL, NULL, napi_default, NULL},
      {"abiVersion", NULL, js_abi_version, NULL, NULL, NULL, napi_default, NULL},
      {"uploadBitmap", NULL, js_upload_bitmap, NULL, NULL, NULL, napi_default, NULL},
      {"decodeBitmaps", NULL, js_decode_bitmaps, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapDesc", NULL, js_bitmap_desc, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapDownload", NULL, js_bitmap_download, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapPreview", NULL, js_bitmap_preview, NULL, NULL, NULL, napi_default, NULL},
      {"thumbnails", NULL, js_thumbnails, NULL, NULL, NULL, napi_default, NULL},
      {"bitmapRelease", NULL, js_bitmap_release, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBitmaps", NULL, js_stitch_bitmaps, NULL, NULL, NULL, napi_default, NULL},
      {"stitchBitmapsSync", NULL, js_stitch_bitmaps_sync, NULL, NULL, NULL, napi_default, NULL},
      {"debugBitmapBytes", NULL, js_debug_bitmap_bytes, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
