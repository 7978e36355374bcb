// The C ABI of include/tuatara_hip.h: extern "C", plain pointers and sizes, no exceptions across it.
#include "engine.h"
#include "page_table.h"
#include "tables_rule.h"
#include "barcodes_rule.h"
#include "marks_rule.h"

namespace ttr {

thread_local std::string g_last_error;

}  // namespace ttr

using namespace ttr;

void hand_out(std::vector<Result>& results, int n, ttr_result** out) {
  for (int i = 0; i < n; ++i) { out[i] = new ttr_result(); out[i]->r = std::move(results[i]); }
}

static void run_locked(ttr_engine* e, const uint8_t* d_pages, int n, int h, int w, ttr_result** out) {
  std::vector<Result> res;
  e->e->run_pages(d_pages, n, h, w, res);
  hand_out(res, n, out);
}

// the stage entry points' crop rectangle of one heat-map rect: adjust_result_coordinates + boundingRect, clamped to the image (tuatara.cpp:406-418)
static RRect stage_crop_rect(const float* r5, float ratio, int h, int w, int* rect5) {
  const RRect r{r5[0], r5[1], r5[2], r5[3], r5[4]};
  const RRect b = adjust_coordinates(r, 1.f / ratio, 1.f / ratio);
  int xywh[4];
  bounding_rect(b, xywh);
  rect5[0] = std::max(xywh[0], 0); rect5[1] = std::max(xywh[1], 0);
  rect5[2] = std::min(xywh[0] + xywh[2], w); rect5[3] = std::min(xywh[1] + xywh[3], h);
  return b;
}

// the crop calls' rule for one rect on an h x w page: the clamped crop rectangle rc[0..4), the packer's coefficients coef8 and the turned quad; returns the
// rect in image pixels.  BOUNDING at turn 0 is ttr_pack_crops's crop (rc alone: the plain packer reads no coefficients), RECTIFIED at turn 0 ttr_pack_crops_rectified's
static RRect oriented_crop(const float* r5, float ratio, int h, int w, int crop_mode, int turn, int* rc, int64_t* coef8, float* quad8) {
  const RRect b = stage_crop_rect(r5, ratio, h, w, rc);
  Pt2f q[4], qt[4]; double cf[6]; int64_t fx[6];
  const int kind = deskew_quad(b, q, cf);                       // Q: the deskewed quad (crop_mode 1) ...
  if (crop_mode == TTR_CROP_BOUNDING) box_edge_quad(rc[0], rc[1], rc[2], rc[3], q);   // ... or the clamped boundingRect's pixel edges
  if (turn == 0 && crop_mode == TTR_CROP_RECTIFIED) {           // ttr_pack_crops_rectified's crop
    coef8[0] = kind;
    deskew_fixed(cf, fx);
  } else {
    coef8[0] = 1;
    turn_coef(q, turn, fx);
  }
  for (int k = 0; k < 6; ++k) coef8[1 + k] = fx[k];
  for (int k = 0; k < 4; ++k) qt[k] = q[(k + turn) & 3];
  if (quad8) for (int k = 0; k < 4; ++k) { quad8[2 * k] = qt[k].x; quad8[2 * k + 1] = qt[k].y; }
  return b;
}

// the stage calls of the table kernels: n host images, each with its own row stride kept, one after another in staging_img at offsets rounded up to 256
// bytes -> their pages (checked: sizes, strides, one canvas) and the device page table of slot 0, both enqueued on the engine's stream
static std::vector<Engine::Page> stage_host_pages(Engine& E, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n) {
  if (n <= 0 || !images || !hs || !ws) throw std::runtime_error("null argument");
  std::vector<Engine::Page> pages((size_t)n);
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const long long stride = row_strides ? (long long)row_strides[i] : (long long)ws[i] * 3;
    if (!images[i] || hs[i] <= 0 || ws[i] <= 0 || stride < (long long)ws[i] * 3 || stride > 0x7fffffffLL) throw std::runtime_error("Error reading image from file");
    off[i + 1] = (off[i] + (size_t)hs[i] * (size_t)stride + 255) & ~(size_t)255;
  }
  E.staging_img.ensure(off[n]);
  for (int i = 0; i < n; ++i) {
    const int stride = row_strides ? row_strides[i] : ws[i] * 3;
    pages[i] = Engine::Page{E.staging_img.as<uint8_t>() + off[i], hs[i], ws[i], stride, CanvasGeom{}};
  }
  E.check_pages(pages);
  for (int i = 0; i < n; ++i)
    TTR_HIP_CHECK(hipMemcpy2DAsync(E.staging_img.as<uint8_t>() + off[i], (size_t)pages[i].stride, images[i], (size_t)pages[i].stride, (size_t)ws[i] * 3, hs[i], hipMemcpyHostToDevice, E.stream));
  E.upload_page_table(pages, 0);
  return pages;
}

// ---- the shared bodies of the host-staged stage calls: all of their work goes onto E.stream, and each ends with a wait (the caller's arrays and the calls'
// own host vectors are pageable: they live until that wait)

// the image arguments of the calls that take one host image with row_stride 0 = packed rows (tuatara.cpp:344-347's message)
static void check_host_image(const uint8_t* img, int h, int w, int row_stride) {
  if (!img || h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error("Error reading image from file");
}

// the decode calls, host logits [n][26][95]: E.logits and the RecOut block made large enough, the logits' upload enqueued; returns the pass over them, for
// parseq_decode (no crops; no constraint until the call names one)
static Engine::RecPass stage_logits(Engine& E, const float* logits, int n) {
  const size_t bytes = (size_t)n * Engine::kLogitWords * 4;
  E.logits.ensure(bytes);
  Engine::RecPass p;
  p.N = n; p.logits = E.logits.as<float>(); p.out = E.rec_out(n);
  TTR_HIP_CHECK(hipMemcpyAsync(E.logits.p, logits, bytes, hipMemcpyHostToDevice, E.stream));
  return p;
}

// ... and their end: each RecOut field the caller gave a place for, then the wait (known: no range guard here or in the crop calls, unlike fetch_logits - none of
// their kernels watches a range word)
static void fetch_decoded(Engine& E, const Engine::RecOut& o, int n, int32_t* ids, float* probs, float* conf) {
  if (ids) TTR_HIP_CHECK(hipMemcpyAsync(ids, o.ids, (size_t)n * 26 * 4, hipMemcpyDeviceToHost, E.stream));
  if (probs) TTR_HIP_CHECK(hipMemcpyAsync(probs, o.prob, (size_t)n * 26 * 4, hipMemcpyDeviceToHost, E.stream));
  if (conf) TTR_HIP_CHECK(hipMemcpyAsync(conf, o.conf, (size_t)n * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
}

// the crop calls: n crops under the finished host rects [n][5] and coef [n][8] (the rect packer alone reads and uploads coef), cut from one host image, uploaded
// here with its rows image->row_stride bytes apart, or - image == nullptr - from the pages of slot 0's table as stage_host_pages left them; crops_out [n][32][128][3]
enum CropPacker { kPackPlain, kPackRect };
static void pack_stage(Engine& E, const Engine::HostImage* image, const std::vector<int>& rects, const std::vector<int64_t>& coef, CropPacker packer, uint8_t* crops_out) {
  const int n = (int)(rects.size() / 5);
  const bool rect = packer == kPackRect;
  if (image) E.staging_img.ensure((size_t)image->h * image->w * 3);
  E.rects_dev.ensure(rects.size() * 4);
  if (rect) E.coef_dev.ensure(coef.size() * 8);
  E.crops.ensure((size_t)n * Engine::kCropBytes);
  if (image) TTR_HIP_CHECK(hipMemcpy2DAsync(E.staging_img.p, (size_t)image->w * 3, image->data, (size_t)image->row_stride, (size_t)image->w * 3, image->h, hipMemcpyHostToDevice, E.stream));
  TTR_HIP_CHECK(hipMemcpyAsync(E.rects_dev.p, rects.data(), rects.size() * 4, hipMemcpyHostToDevice, E.stream));
  if (rect) TTR_HIP_CHECK(hipMemcpyAsync(E.coef_dev.p, coef.data(), coef.size() * 8, hipMemcpyHostToDevice, E.stream));
  const uint8_t* src = E.staging_img.as<uint8_t>();
  const PageRow* table = E.page_table[0].as<PageRow>();
  if (image && rect) launch_pack_crops_rect(src, 0, image->w * 3, image->h, image->w, E.rects_dev.as<int>(), E.coef_dev.as<int64_t>(), E.crops.as<uint8_t>(), n, E.stream);
  else if (image) launch_pack_crops(src, 0, image->w * 3, E.rects_dev.as<int>(), E.crops.as<uint8_t>(), n, E.stream);
  else if (rect) launch_pack_crops_rect_pages(table, E.rects_dev.as<int>(), E.coef_dev.as<int64_t>(), E.crops.as<uint8_t>(), n, E.stream);
  else launch_pack_crops_pages(table, E.rects_dev.as<int>(), E.crops.as<uint8_t>(), n, E.stream);
  TTR_HIP_CHECK(hipMemcpyAsync(crops_out, E.crops.p, (size_t)n * Engine::kCropBytes, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
}

// the recogniser calls, host crops [n][32][128][3]: the buffers of a forward made large enough (the AR logits' only where they are asked for), the crops' upload
// enqueued; returns the pass over them, under the engine's own set until the call names another
static Engine::RecPass stage_crops(Engine& E, const uint8_t* crops, int n, bool with_ar) {
  E.crops.ensure((size_t)n * Engine::kCropBytes);
  E.logits.ensure((size_t)n * Engine::kLogitWords * 4);
  Engine::RecPass p;
  p.crops = E.crops.as<uint8_t>(); p.N = n; p.logits = E.logits.as<float>(); p.out = E.rec_out(n); p.mask = E.charset;
  if (with_ar) { E.ar_logits.ensure((size_t)n * Engine::kLogitWords * 4); p.ar = E.ar_logits.as<float>(); }
  TTR_HIP_CHECK(hipMemcpyAsync(E.crops.p, crops, (size_t)n * Engine::kCropBytes, hipMemcpyHostToDevice, E.stream));
  return p;
}

// ... and their end: the logits, the AR logits and the ids where there is a place for them, then the range guard's word of the forward, the wait and its verdict under the call's name
static void fetch_logits(Engine& E, const Engine::RecOut& o, int n, float* logits, float* ar_logits, int32_t* ids, const char* what) {
  TTR_HIP_CHECK(hipMemcpyAsync(logits, E.logits.p, (size_t)n * Engine::kLogitWords * 4, hipMemcpyDeviceToHost, E.stream));
  if (ar_logits) TTR_HIP_CHECK(hipMemcpyAsync(ar_logits, E.ar_logits.p, (size_t)n * Engine::kLogitWords * 4, hipMemcpyDeviceToHost, E.stream));
  if (ids) TTR_HIP_CHECK(hipMemcpyAsync(ids, o.ids, (size_t)n * 26 * 4, hipMemcpyDeviceToHost, E.stream));
  E.range_fetch(Engine::kRangeStage);
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  E.range_verify(Engine::kRangeStage, what);
}

extern "C" {

void ttr_config_default(ttr_config* c) {
  c->precision = TTR_PREC_F16X4; c->device = 0; c->canvas_size = 1024; c->mag_ratio = 1.0f;
  c->text_threshold = 0.7f; c->link_threshold = 0.4f; c->low_text = 0.4f; c->min_area = 10;
  c->strict_crops = 0; c->max_components = 4096; c->verbose = 0; c->crop_mode = TTR_CROP_BOUNDING;
  c->orient = TTR_ORIENT_OFF; c->orient_page = 0; c->lines = 0; c->chars = 0; c->blocks = 0; c->mixed_batches = 0;
}

const char* ttr_last_error(void) { return g_last_error.c_str(); }

const char* ttr_version(void) { return "tuatara-mi355x 0.1 (gfx950)"; }

ttr_engine* ttr_create(const char* weights_dir, const ttr_config* cfg) {
  TTR_GUARD_BEGIN
  if (!weights_dir || !*weights_dir) throw std::runtime_error("Please provide a value for weights_dir");  // tuatara.cpp:315-318
  ttr_config c;
  if (cfg) c = *cfg; else ttr_config_default(&c);
  if (c.max_components <= 0) c.max_components = 4096;
  std::unique_ptr<ttr_engine> h(new ttr_engine());
  h->e.reset(new Engine(weights_dir, c));
  return h.release();
  TTR_GUARD_END(nullptr)
}

void ttr_destroy(ttr_engine* e) { delete e; }

int ttr_pages_to_data_dev(ttr_engine* e, const uint8_t* d_pages, int n, int h, int w, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || !out) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  run_locked(e, d_pages, n, h, w, out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_stream_push(ttr_engine* e, const uint8_t* d_pages, int n, int h, int w, ttr_result** out_prev, int* n_prev) {
  TTR_GUARD_BEGIN
  if (!e || !out_prev || !n_prev) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  int np = 0;
  e->e->stream_push(d_pages, n, h, w, res, np);
  hand_out(res, np, out_prev);
  *n_prev = np;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_canvas_geometry(const ttr_engine* e, int h, int w, int* H, int* W, float* ratio) {
  TTR_GUARD_BEGIN
  ttr_config c;
  if (e) c = e->e->cfg; else ttr_config_default(&c);
  if (h <= 0 || w <= 0) throw std::runtime_error("Error reading image from file");
  const CanvasGeom g = e ? e->e->page_geometry(h, w) : canvas_geometry(h, w, c.canvas_size, c.mag_ratio);   // (tiled pages: the page canvas c32(h) x c32(w), ratio 1)
  if (g.target_h <= 0 || g.target_w <= 0) throw std::runtime_error("image too thin to resize");
  if (H) *H = g.h32;
  if (W) *W = g.w32;
  if (ratio) *ratio = g.ratio;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_pages_to_data_dev_v(ttr_engine* e, const ttr_page* pages, int n, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || !out || (n > 0 && !pages)) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  e->e->run_pages_v(pages, n, res);
  hand_out(res, n, out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_stream_push_v(ttr_engine* e, const ttr_page* pages, int n, ttr_result** out_prev, int* n_prev) {
  TTR_GUARD_BEGIN
  if (!e || !out_prev || !n_prev || (n > 0 && !pages)) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  int np = 0;
  e->e->stream_push_v(pages, n, res, np);
  hand_out(res, np, out_prev);
  *n_prev = np;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_last_images_batches(ttr_engine* e, int32_t* pages_per_batch, int cap) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  const std::vector<int32_t>& b = e->e->last_batches;
  if (pages_per_batch) for (int i = 0; i < (int)b.size() && i < cap; ++i) pages_per_batch[i] = b[i];
  return (int)b.size();
  TTR_GUARD_END(-1)
}

int ttr_stream_flush(ttr_engine* e, ttr_result** out_prev, int* n_prev) {
  TTR_GUARD_BEGIN
  if (!e || !out_prev || !n_prev) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  int np = 0;
  e->e->stream_flush(res, np);
  hand_out(res, np, out_prev);
  *n_prev = np;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_image_to_data(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || !out) throw std::runtime_error("null argument");
  if (!img || h <= 0 || w <= 0) throw std::runtime_error("Error reading image from file");  // tuatara.cpp:344-347
  Engine& E = *e->e;
  EngineScope lk(E);
  run_locked(e, E.stage_page("ttr_image_to_data", img, h, w, row_stride, 0, 0, 0, nullptr, false).data, 1, h, w, out);   // (checked above, under the reference's text)
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_images_to_data(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || !out || n < 0 || (n > 0 && (!images || !hs || !ws))) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  std::vector<Engine::HostImage> imgs((size_t)n);
  for (int i = 0; i < n; ++i) imgs[i] = Engine::HostImage{images[i], hs[i], ws[i], row_strides ? (std::ptrdiff_t)row_strides[i] : (std::ptrdiff_t)ws[i] * 3};
  std::vector<Result> res;
  std::vector<int> failed;
  std::string first;
  E.run_images(imgs, res, failed, first);
  hand_out(res, n, out);
  if (!failed.empty()) {   // partial failure: every other image's result stands; the failed ones are empty (header)
    std::string msg = std::to_string(failed.size()) + " of " + std::to_string(n) + " images failed (indices";
    for (size_t k = 0; k < failed.size() && k < 16; ++k) msg += " " + std::to_string(failed[k]);
    if (failed.size() > 16) msg += " ...";
    g_last_error = msg + "): " + first;
    return (int)failed.size();
  }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_result_count(const ttr_result* r) { return r ? (int)r->r.text.size() : 0; }

const char* ttr_result_text(const ttr_result* r, int i) { return r->r.text[i].c_str(); }

const float* ttr_result_bbox(const ttr_result* r, int i) { return &r->r.bbox[4 * (size_t)i]; }

const int32_t* ttr_result_ids(const ttr_result* r, int i) { return &r->r.ids[26 * (size_t)i]; }

const float* ttr_result_quad(const ttr_result* r, int i) { return &r->r.quad[8 * (size_t)i]; }

const float* ttr_result_quads(const ttr_result* r) { return r && !r->r.quad.empty() ? r->r.quad.data() : nullptr; }

float ttr_result_conf(const ttr_result* r, int i) { return r->r.conf[(size_t)i]; }

const float* ttr_result_prob(const ttr_result* r, int i) { return &r->r.prob[26 * (size_t)i]; }

const float* ttr_result_confs(const ttr_result* r) { return r && !r->r.conf.empty() ? r->r.conf.data() : nullptr; }

const float* ttr_result_probs_all(const ttr_result* r) { return r && !r->r.prob.empty() ? r->r.prob.data() : nullptr; }

int ttr_results_gather_conf(ttr_result* const* rs, int n, float* conf, float* probs) {
  if (!rs || n < 0) return -1;
  size_t oc = 0, op = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    if (conf && !r.conf.empty()) memcpy(conf + oc, r.conf.data(), r.conf.size() * 4);
    if (probs && !r.prob.empty()) memcpy(probs + op, r.prob.data(), r.prob.size() * 4);
    oc += r.conf.size(); op += r.prob.size();
  }
  return (int)oc;
}

int ttr_result_orient(const ttr_result* r, int i) { return r && !r->r.orient.empty() ? r->r.orient[(size_t)i] : 0; }

const int32_t* ttr_result_orients(const ttr_result* r) { return r && !r->r.orient.empty() ? r->r.orient.data() : nullptr; }

int ttr_result_orient_candidates(const ttr_result* r) { return r ? r->r.orient_k : 1; }

const float* ttr_result_orient_confs(const ttr_result* r) {   // (off: K = 1, the candidate confs are the confs)
  if (!r) return nullptr;
  const std::vector<float>& v = r->r.orient_k > 1 ? r->r.orient_conf : r->r.conf;
  return v.empty() ? nullptr : v.data();
}

int ttr_result_page_orient(const ttr_result* r) { return r ? r->r.page_orient : 0; }

int ttr_results_gather_orient(ttr_result* const* rs, int n, int32_t* turns, float* cand_conf, int32_t* page_turns) {
  if (!rs || n < 0) return -1;
  int k = 0;
  for (int i = 0; i < n; ++i) {   // (an empty result - an image that failed - has no candidates to disagree with)
    if (!rs[i] || rs[i]->r.text.empty()) continue;
    if (k && rs[i]->r.orient_k != k) return -1;
    k = rs[i]->r.orient_k;
  }
  size_t ot = 0, oc = 0;
  for (int i = 0; i < n; ++i) {
    if (page_turns) page_turns[i] = rs[i] ? rs[i]->r.page_orient : 0;
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    const size_t cnt = r.text.size();
    if (turns) {
      if (r.orient.size() == cnt) { if (cnt) memcpy(turns + ot, r.orient.data(), cnt * 4); }
      else std::fill(turns + ot, turns + ot + cnt, 0);
    }
    const std::vector<float>& cc = r.orient_k > 1 ? r.orient_conf : r.conf;
    if (cand_conf) {
      if (cc.size() == cnt * r.orient_k) { if (cnt) memcpy(cand_conf + oc, cc.data(), cc.size() * 4); }
      else std::fill(cand_conf + oc, cand_conf + oc + cnt * r.orient_k, 0.f);
    }
    ot += cnt; oc += cnt * r.orient_k;
  }
  return (int)ot;
}

int ttr_orient_select(const float* conf, const int32_t* ids, int n, int k, int per_page, int32_t* turns, int32_t* page_turn) {
  if (n < 0 || (k != 1 && k != 2 && k != 4) || !page_turn || (n > 0 && (!conf || !ids || !turns))) return -1;
  orient_select(conf, ids, n, k, per_page != 0, turns, page_turn);
  return 0;
}

int ttr_result_line_count(const ttr_result* r) { return r ? r->r.n_lines : 0; }

const int32_t* ttr_result_lines(const ttr_result* r) { return r && !r->r.line.empty() ? r->r.line.data() : nullptr; }

const int32_t* ttr_result_words(const ttr_result* r) { return r && !r->r.word.empty() ? r->r.word.data() : nullptr; }

const int32_t* ttr_result_reading_order(const ttr_result* r) { return r && !r->r.order.empty() ? r->r.order.data() : nullptr; }

const int32_t* ttr_result_line_first(const ttr_result* r) { return r && r->r.n_lines > 0 ? r->r.line_first.data() : nullptr; }

const float* ttr_result_line_bboxes(const ttr_result* r) { return r && !r->r.line_bbox.empty() ? r->r.line_bbox.data() : nullptr; }

static int copy_out(const std::string& t, char* buf, size_t cap) {
  if (buf && cap >= t.size() && !t.empty()) memcpy(buf, t.data(), t.size());
  return (int)t.size();
}

int ttr_result_line_text(const ttr_result* r, int l, char* buf, size_t cap) {
  if (!r || l < 0 || l >= r->r.n_lines) return 0;
  return copy_out(r->r.line_text(l), buf, cap);
}

int ttr_result_page_text(const ttr_result* r, char* buf, size_t cap) {
  if (!r || r->r.n_lines <= 0) return 0;
  return copy_out(r->r.page_text(), buf, cap);
}

int ttr_results_gather_lines(ttr_result* const* rs, int n, int32_t* n_lines, int32_t* line, int32_t* word, int32_t* order, int32_t* line_first,
                             float* line_bboxes) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, ol = 0, of = 0;
  for (int i = 0; i < n; ++i) {
    static const Result none;
    const Result& r = rs[i] ? rs[i]->r : none;
    const size_t cnt = r.text.size(), nl = (size_t)r.n_lines;
    if (n_lines) n_lines[i] = r.n_lines;
    const bool has = nl > 0 && r.line.size() == cnt;
    auto put = [&](int32_t* dst, const std::vector<int32_t>& v) {
      if (!dst) return;
      if (has) std::copy(v.begin(), v.end(), dst + oi); else std::fill(dst + oi, dst + oi + cnt, -1);
    };
    put(line, r.line); put(word, r.word); put(order, r.order);
    if (line_first) { if (has) std::copy(r.line_first.begin(), r.line_first.end(), line_first + of); else line_first[of] = 0; }
    if (line_bboxes && has) std::copy(r.line_bbox.begin(), r.line_bbox.end(), line_bboxes + 4 * ol);
    oi += cnt; ol += has ? nl : 0; of += (has ? nl : 0) + 1;
  }
  return (int)ol;
}

int ttr_lines_from_quads(const float* quads, int n, int32_t* line, int32_t* word, int32_t* n_lines) {
  if (n < 0 || !n_lines || (n > 0 && (!quads || !line || !word))) return -1;
  std::vector<int32_t> cuv((size_t)n * 6);
  for (int i = 0; i < n; ++i) if (!lines_cuv(quads + 8 * (size_t)i, cuv.data() + 6 * (size_t)i)) return -1;
  lines_from_cuv(cuv.data(), n, line, word, n_lines);
  return 0;
}

int ttr_group_lines(ttr_engine* e, const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines) {
  TTR_GUARD_BEGIN
  if (!e || pages < 0 || (pages > 0 && !first) || (pages > 0 && first[pages] > 0 && !quads)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_group_lines");
  E.group_lines(quads, first, pages, line, word, n_lines);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_result_char_count(const ttr_result* r, int i) {
  if (!r || r->r.char_first.empty() || i < 0 || (size_t)i + 1 >= r->r.char_first.size()) return 0;
  return r->r.char_first[(size_t)i + 1] - r->r.char_first[(size_t)i];
}

const int32_t* ttr_result_char_first(const ttr_result* r) { return r && !r->r.char_first.empty() ? r->r.char_first.data() : nullptr; }

const float* ttr_result_char_quads(const ttr_result* r) { return r && !r->r.char_quad.empty() ? r->r.char_quad.data() : nullptr; }

const float* ttr_result_char_bboxes(const ttr_result* r) { return r && !r->r.char_bbox.empty() ? r->r.char_bbox.data() : nullptr; }

const int32_t* ttr_result_char_cuts(const ttr_result* r) { return r && !r->r.char_cuts.empty() ? r->r.char_cuts.data() : nullptr; }

const int32_t* ttr_result_char_modes(const ttr_result* r) { return r && !r->r.char_mode.empty() ? r->r.char_mode.data() : nullptr; }

const uint8_t* ttr_result_char_profiles(const ttr_result* r) { return r && !r->r.char_profile.empty() ? r->r.char_profile.data() : nullptr; }

int ttr_results_gather_chars(ttr_result* const* rs, int n, int32_t* char_first, float* char_quads, float* char_bboxes, int32_t* cuts, int32_t* modes,
                             uint8_t* profiles) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, oc = 0, of = 0;
  for (int i = 0; i < n; ++i) {
    static const Result none;
    const Result& r = rs[i] ? rs[i]->r : none;
    const size_t cnt = r.text.size();
    const bool has = cnt > 0 && r.char_first.size() == cnt + 1;
    const size_t nc = has ? (size_t)r.char_first[cnt] : 0;
    if (char_first) { if (has) std::copy(r.char_first.begin(), r.char_first.end(), char_first + of); else std::fill(char_first + of, char_first + of + cnt + 1, 0); }
    if (char_quads && nc) std::copy(r.char_quad.begin(), r.char_quad.end(), char_quads + 8 * oc);
    if (char_bboxes && nc) std::copy(r.char_bbox.begin(), r.char_bbox.end(), char_bboxes + 4 * oc);
    if (cuts) { if (has) std::copy(r.char_cuts.begin(), r.char_cuts.end(), cuts + 27 * oi); else std::fill(cuts + 27 * oi, cuts + 27 * (oi + cnt), -1); }
    if (modes) { if (has) std::copy(r.char_mode.begin(), r.char_mode.end(), modes + oi); else std::fill(modes + oi, modes + oi + cnt, 0); }
    if (profiles) { if (has) std::copy(r.char_profile.begin(), r.char_profile.end(), profiles + 128 * oi); else std::fill(profiles + 128 * oi, profiles + 128 * (oi + cnt), (uint8_t)0); }
    oi += cnt; oc += nc; of += cnt + 1;
  }
  return (int)oc;
}

int ttr_char_cuts_from_profile(const uint8_t* q128, int K, int qlow, int32_t* cuts27, int32_t* mode) {
  if (!q128 || !cuts27 || !mode || K < 0 || K > kCharsMax) return -1;
  chars_cuts_from_profile(q128, K, qlow, cuts27, mode);
  return 0;
}

int ttr_chars_from_map(const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars, int n,
                       int32_t* cuts, int32_t* modes, uint8_t* profiles) {
  if (n < 0 || (n > 0 && (!tnorm || H2 <= 0 || W2 <= 0 || !quads || !turns || !nchars || !cuts || !modes || !profiles))) return -1;
  const double k = chars_scale(ratio);
  const int qlow = (int)(low_text * 255.f);
  for (int c = 0; c < n; ++c) {
    int64_t fx[6];
    if (turns[c] < 0 || turns[c] > 3 || nchars[c] < 0 || nchars[c] > kCharsMax || !chars_coef(quads + 8 * (size_t)c, turns[c], k, fx)) return -1;
    chars_profile(tnorm, H2, W2, fx, profiles + 128 * (size_t)c);
    chars_cuts_from_profile(profiles + 128 * (size_t)c, nchars[c], qlow, cuts + 27 * (size_t)c, modes + c);
  }
  return 0;
}

int ttr_char_quads_from_cuts(const float* quad, int turn, const int32_t* cuts27, int K, float* quads_out, float* bboxes_out) {
  if (!quad || turn < 0 || turn > 3 || K < 0 || K > kCharsMax || (K > 0 && (!cuts27 || !quads_out || !bboxes_out))) return -1;
  chars_quads_from_cuts(quad, turn, cuts27, K, quads_out, bboxes_out);
  return 0;
}

int ttr_char_cuts(ttr_engine* e, const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars,
                  int n, int32_t* cuts, int32_t* modes, uint8_t* profiles) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && (!tnorm || !quads || !turns || !nchars))) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_char_cuts");
  E.char_cuts(tnorm, H2, W2, ratio, low_text, quads, turns, nchars, n, cuts, modes, profiles);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_result_block_count(const ttr_result* r) { return r ? r->r.n_blocks : 0; }

int ttr_result_block_mode(const ttr_result* r) { return r && r->r.n_blocks > 0 ? r->r.block_mode : 0; }

const int32_t* ttr_result_line_blocks(const ttr_result* r) { return r && !r->r.line_block.empty() ? r->r.line_block.data() : nullptr; }

const int32_t* ttr_result_line_pos(const ttr_result* r) { return r && !r->r.line_pos.empty() ? r->r.line_pos.data() : nullptr; }

const int32_t* ttr_result_blocks(const ttr_result* r) { return r && !r->r.block.empty() ? r->r.block.data() : nullptr; }

const int32_t* ttr_result_block_order(const ttr_result* r) { return r && !r->r.block_order.empty() ? r->r.block_order.data() : nullptr; }

const int32_t* ttr_result_block_first(const ttr_result* r) { return r && r->r.n_blocks > 0 ? r->r.block_first.data() : nullptr; }

const float* ttr_result_block_bboxes(const ttr_result* r) { return r && !r->r.block_bbox.empty() ? r->r.block_bbox.data() : nullptr; }

int ttr_result_block_text(const ttr_result* r, int b, char* buf, size_t cap) {
  if (!r || b < 0 || b >= r->r.n_blocks) return 0;
  return copy_out(r->r.block_text(b), buf, cap);
}

int ttr_result_page_text_blocks(const ttr_result* r, char* buf, size_t cap) {
  if (!r || r->r.n_blocks <= 0) return 0;
  return copy_out(r->r.page_text_blocks(), buf, cap);
}

int ttr_results_gather_blocks(ttr_result* const* rs, int n, int32_t* n_blocks, int32_t* modes, int32_t* blocks, int32_t* line_blocks, int32_t* line_pos,
                              int32_t* block_order, int32_t* block_first, float* block_bboxes) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, ol = 0, ob = 0, of = 0;
  for (int i = 0; i < n; ++i) {
    static const Result none;
    const Result& r = rs[i] ? rs[i]->r : none;
    const size_t cnt = r.text.size(), nb = (size_t)r.n_blocks;
    const bool has = nb > 0 && r.block.size() == cnt;
    const size_t nl = has ? r.line_block.size() : 0;
    if (n_blocks) n_blocks[i] = has ? r.n_blocks : 0;
    if (modes) modes[i] = has ? r.block_mode : 0;
    if (blocks) { if (has) std::copy(r.block.begin(), r.block.end(), blocks + oi); else std::fill(blocks + oi, blocks + oi + cnt, -1); }
    if (has) {
      if (line_blocks) std::copy(r.line_block.begin(), r.line_block.end(), line_blocks + ol);
      if (line_pos) std::copy(r.line_pos.begin(), r.line_pos.end(), line_pos + ol);
      if (block_order) std::copy(r.block_order.begin(), r.block_order.end(), block_order + ol);
      if (block_bboxes) std::copy(r.block_bbox.begin(), r.block_bbox.end(), block_bboxes + 4 * ob);
    }
    if (block_first) { if (has) std::copy(r.block_first.begin(), r.block_first.end(), block_first + of); else block_first[of] = 0; }
    oi += cnt; ol += nl; ob += has ? nb : 0; of += (has ? nb : 0) + 1;
  }
  return (int)ob;
}

int ttr_blocks_from_quads(const float* quads, int n, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block, int32_t* pos, int32_t* n_blocks,
                          int32_t* mode) {
  if (n < 0 || (n > 0 && !quads)) return -1;
  std::vector<int32_t> cuv((size_t)n * 6), ln((size_t)n), wd((size_t)n), bl((size_t)n), ps((size_t)n);
  for (int i = 0; i < n; ++i) if (!lines_cuv(quads + 8 * (size_t)i, cuv.data() + 6 * (size_t)i)) return -1;
  int32_t nl = 0, nb = 0, md = 1;
  lines_from_cuv(cuv.data(), n, ln.data(), wd.data(), &nl);
  blocks_from_lines(cuv.data(), n, ln.data(), wd.data(), nl, bl.data(), ps.data(), &nb, &md);
  if (line) std::copy(ln.begin(), ln.end(), line);
  if (word) std::copy(wd.begin(), wd.end(), word);
  if (block) std::copy(bl.begin(), bl.end(), block);
  if (pos) std::copy(ps.begin(), ps.end(), pos);
  if (n_lines) *n_lines = nl;
  if (n_blocks) *n_blocks = nb;
  if (mode) *mode = md;
  return 0;
}

int ttr_group_blocks(ttr_engine* e, const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block,
                     int32_t* pos, int32_t* n_blocks, int32_t* mode) {
  TTR_GUARD_BEGIN
  if (!e || pages < 0 || (pages > 0 && !first) || (pages > 0 && first[pages] > 0 && !quads)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_group_blocks");
  E.group_blocks(quads, first, pages, line, word, n_lines, block, pos, n_blocks, mode);
  return 0;
  TTR_GUARD_END(-1)
}

void ttr_result_free(ttr_result* r) { delete r; }

const float* ttr_result_bboxes(const ttr_result* r) { return r && !r->r.bbox.empty() ? r->r.bbox.data() : nullptr; }

const int32_t* ttr_result_ids_all(const ttr_result* r) { return r && !r->r.ids.empty() ? r->r.ids.data() : nullptr; }

int ttr_results_gather(ttr_result* const* rs, int n, int32_t* counts, float* bboxes, int32_t* ids, char* texts, size_t texts_cap, size_t* texts_need) {
  if (!rs || n < 0) return -1;
  size_t total = 0, need = 0;
  for (int i = 0; i < n; ++i) {
    const size_t c = rs[i] ? rs[i]->r.text.size() : 0;
    if (counts) counts[i] = (int32_t)c;
    total += c;
    if (rs[i]) for (const auto& t : rs[i]->r.text) need += t.size() + 1;
  }
  if (texts_need) *texts_need = need;
  size_t ob = 0, oi = 0, ot = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    if (bboxes && !r.bbox.empty()) { memcpy(bboxes + ob, r.bbox.data(), r.bbox.size() * 4); ob += r.bbox.size(); }
    if (ids && !r.ids.empty()) { memcpy(ids + oi, r.ids.data(), r.ids.size() * 4); oi += r.ids.size(); }
    if (texts && texts_cap >= need) for (const auto& t : r.text) { memcpy(texts + ot, t.data(), t.size()); ot += t.size(); texts[ot++] = '\n'; }
  }
  return (int)total;
}

int ttr_result_texts(const ttr_result* r, char* buf, size_t cap) {
  if (!r) return 0;
  size_t need = 0;
  for (const auto& t : r->r.text) need += t.size() + 1;
  if (!buf || cap < need) return (int)need;
  size_t o = 0;
  for (const auto& t : r->r.text) { memcpy(buf + o, t.data(), t.size()); o += t.size(); buf[o++] = '\n'; }
  return (int)need;
}

int ttr_craft_heatmap(ttr_engine* e, const uint8_t* canvas, int H, int W, float* heat_out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_craft_heatmap");
  E.canvas.ensure((size_t)H * W * 3);
  E.heat.ensure((size_t)H * W / 4 * 2 * 4);
  TTR_HIP_CHECK(hipMemcpyAsync(E.canvas.p, canvas, (size_t)H * W * 3, hipMemcpyHostToDevice, E.stream));
  E.craft_forward(E.canvas.as<uint8_t>(), 1, H, W, E.heat.as<float>());
  TTR_HIP_CHECK(hipMemcpyAsync(heat_out, E.heat.p, (size_t)H * W / 4 * 2 * 4, hipMemcpyDeviceToHost, E.stream));
  E.range_fetch(Engine::kRangeStage);
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  E.range_verify(Engine::kRangeStage, "ttr_craft_heatmap");
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_ccl_boxes(ttr_engine* e, const float* heat, int H2, int W2, float* rects5, int max_rects, int* n) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_ccl_boxes");
  E.heat.ensure((size_t)H2 * W2 * 2 * 4);
  TTR_HIP_CHECK(hipMemcpyAsync(E.heat.p, heat, (size_t)H2 * W2 * 2 * 4, hipMemcpyHostToDevice, E.stream));
  E.ccl_launch(E.heat.as<float>(), 0, 1, 1, 0, H2, W2);
  std::vector<std::vector<RRect>> dets;
  dets.assign(1, std::vector<RRect>());
  E.ccl_collect(0, 1, 0, H2, W2, dets);
  const std::vector<RRect>& det = dets[0];
  *n = (int)det.size();
  for (int i = 0; i < (int)det.size() && i < max_rects; ++i) {
    rects5[5 * i] = det[i].cx; rects5[5 * i + 1] = det[i].cy; rects5[5 * i + 2] = det[i].w; rects5[5 * i + 3] = det[i].h; rects5[5 * i + 4] = det[i].angle;
  }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_resize_canvas(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, uint8_t* canvas, size_t cap, int* H, int* W, float* ratio) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_resize_canvas");
  const CanvasGeom g = canvas_geometry(h, w, E.cfg.canvas_size, E.cfg.mag_ratio);
  *H = g.h32; *W = g.w32; *ratio = g.ratio;
  const size_t need = (size_t)g.h32 * g.w32 * 3;
  if (cap < need) throw std::runtime_error("canvas buffer too small");
  E.canvas.ensure(need);
  const Engine::StagedPage pg = E.stage_page("ttr_resize_canvas", img, h, w, row_stride, 0, 0, 0, nullptr, false);   // (this call has never checked its image)
  launch_resize_pad_u8(pg.data, h, w, pg.stride, E.canvas.as<uint8_t>(), g.target_h, g.target_w, g.h32, g.w32, 1, E.stream);
  TTR_HIP_CHECK(hipMemcpyAsync(canvas, E.canvas.p, need, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_pack_crops(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* rects5, int n, float ratio, uint8_t* crops_out,
                   float* boxes_out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_pack_crops");
  if (n <= 0) return 0;
  std::vector<int> rects((size_t)n * 5, 0);
  std::vector<int64_t> coef((size_t)n * 8, 0);
  for (int i = 0; i < n; ++i) {
    const RRect b = oriented_crop(rects5 + 5 * (size_t)i, ratio, h, w, TTR_CROP_BOUNDING, 0, &rects[5 * (size_t)i], &coef[8 * (size_t)i], nullptr);
    if (boxes_out) { float* o = boxes_out + 5 * (size_t)i; o[0] = b.cx; o[1] = b.cy; o[2] = b.w; o[3] = b.h; o[4] = b.angle; }
  }
  const Engine::HostImage image{img, h, w, row_stride};   // (known: no image check here, and row_stride is taken as given - 0 does not mean packed rows, as it does for ttr_pack_regions)
  pack_stage(E, &image, rects, coef, kPackPlain, crops_out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_pack_crops_rectified(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* rects5, int n, float ratio, uint8_t* crops_out,
                             float* quads_out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_pack_crops_rectified");
  if (n <= 0) return 0;
  std::vector<int> rects((size_t)n * 5, 0);
  std::vector<int64_t> coef((size_t)n * 8, 0);
  for (int i = 0; i < n; ++i)
    oriented_crop(rects5 + 5 * (size_t)i, ratio, h, w, TTR_CROP_RECTIFIED, 0, &rects[5 * (size_t)i], &coef[8 * (size_t)i], quads_out ? quads_out + 8 * (size_t)i : nullptr);
  const Engine::HostImage image{img, h, w, row_stride};   // (known: as ttr_pack_crops - no image check, row_stride as given)
  pack_stage(E, &image, rects, coef, kPackRect, crops_out);   // (always the rect packer: a rect at a multiple of 90 degrees is its kind-0 crop)
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_pack_crops_oriented(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* rects5, int n, float ratio, int crop_mode, int turn,
                            uint8_t* crops_out, float* quads_out) {
  TTR_GUARD_BEGIN
  if (crop_mode != TTR_CROP_BOUNDING && crop_mode != TTR_CROP_RECTIFIED) throw std::runtime_error("crop_mode must be 0 or 1");
  if (turn < 0 || turn > 3) throw std::runtime_error("turn must be 0..3");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_pack_crops_oriented");
  if (n <= 0) return 0;
  std::vector<int> rects((size_t)n * 5, 0);
  std::vector<int64_t> coef((size_t)n * 8, 0);
  for (int i = 0; i < n; ++i)
    oriented_crop(rects5 + 5 * (size_t)i, ratio, h, w, crop_mode, turn, &rects[5 * (size_t)i], &coef[8 * (size_t)i], quads_out ? quads_out + 8 * (size_t)i : nullptr);
  const Engine::HostImage image{img, h, w, row_stride};   // (known: as ttr_pack_crops - no image check, row_stride as given)
  pack_stage(E, &image, rects, coef, turn == 0 && crop_mode == TTR_CROP_BOUNDING ? kPackPlain : kPackRect, crops_out);   // (plain: ttr_pack_crops's crop, by its packer)
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_resize_canvas_batch(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n, uint8_t* canvases,
                            size_t cap, int* H, int* W, float* ratios) {
  TTR_GUARD_BEGIN
  if (!e || !canvases || !H || !W) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_resize_canvas_batch");
  const std::vector<Engine::Page> pages = stage_host_pages(E, images, hs, ws, row_strides, n);
  const CanvasGeom& g = pages[0].g;
  *H = g.h32; *W = g.w32;
  if (ratios) for (int i = 0; i < n; ++i) ratios[i] = pages[i].g.ratio;
  const size_t need = (size_t)n * g.h32 * g.w32 * 3;
  if (cap < need) throw std::runtime_error("canvas buffer too small");
  E.canvas.ensure(need);
  launch_resize_pad_pages(E.page_table[0].as<PageRow>(), E.canvas.as<uint8_t>(), g.h32, g.w32, 1, n, E.stream);
  TTR_HIP_CHECK(hipMemcpyAsync(canvases, E.canvas.p, need, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_pack_crops_batch(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n_pages,
                         const float* rects5, const int32_t* page_of, int n, int crop_mode, int turn, uint8_t* crops_out, float* quads_out) {
  TTR_GUARD_BEGIN
  if (crop_mode != TTR_CROP_BOUNDING && crop_mode != TTR_CROP_RECTIFIED) throw std::runtime_error("crop_mode must be 0 or 1");
  if (turn < 0 || turn > 3) throw std::runtime_error("turn must be 0..3");
  if (!e || (n > 0 && (!rects5 || !page_of || !crops_out))) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_pack_crops_batch");
  if (n <= 0) return 0;
  for (int i = 0; i < n; ++i)
    if (page_of[i] < 0 || page_of[i] >= n_pages) throw std::runtime_error("ttr_pack_crops_batch: page_of[" + std::to_string(i) + "] is not a page of the batch");
  const std::vector<Engine::Page> pages = stage_host_pages(E, images, hs, ws, row_strides, n_pages);
  std::vector<int> rects((size_t)n * 5, 0);
  std::vector<int64_t> coef((size_t)n * 8, 0);
  for (int i = 0; i < n; ++i) {
    const Engine::Page& P = pages[(size_t)page_of[i]];
    oriented_crop(rects5 + 5 * (size_t)i, P.g.ratio, P.h, P.w, crop_mode, turn, &rects[5 * (size_t)i], &coef[8 * (size_t)i], quads_out ? quads_out + 8 * (size_t)i : nullptr);
    rects[5 * (size_t)i + 4] = page_of[i];
  }
  pack_stage(E, nullptr, rects, coef, turn == 0 && crop_mode == TTR_CROP_BOUNDING ? kPackPlain : kPackRect, crops_out);   // (the pages are staged: stage_host_pages checked each image and stride)
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_parseq_logits(ttr_engine* e, const uint8_t* crops, int n, float* logits, float* ar_logits, int32_t* ids) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_parseq_logits");
  if (n <= 0) return 0;
  // (not ttr_parseq_logits_patterns with nothing given: where the engine has a pattern that call compiles and stages a table of its own, this one reads under pattern_own)
  Engine::RecPass p = stage_crops(E, crops, n, ar_logits != nullptr);
  if (E.pattern_decode == TTR_PATTERN_BEST && E.pattern_own.delta) p.best = E.pat_best_out(n);   // (the ids are then the likeliest member's; the logits are the same bits)
  E.parseq_forward(p);
  fetch_logits(E, p.out, n, logits, ar_logits, ids, "ttr_parseq_logits");
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_logits_confidence(ttr_engine* e, const float* logits, int n, int32_t* ids, float* probs, float* conf) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && !logits)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_logits_confidence");
  if (n == 0) return 0;
  const Engine::RecPass p = stage_logits(E, logits, n);
  E.parseq_decode(p);
  fetch_decoded(E, p.out, n, ids, probs, conf);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_logits_confidence_masked(ttr_engine* e, const float* logits, int n, const uint32_t mask[3], int32_t* ids, float* probs, float* conf) {
  TTR_GUARD_BEGIN
  if (!e || !mask || n < 0 || (n > 0 && !logits)) throw std::runtime_error("null argument");
  if (!(mask[0] & 1u)) throw std::runtime_error("ttr_logits_confidence_masked: bit 0 (the end of the text) must be set");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_logits_confidence_masked");
  if (n == 0) return 0;
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = ClassMask::from_allowed(mask);
  E.parseq_decode(p);
  fetch_decoded(E, p.out, n, ids, probs, conf);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_region_from_rect(int x0, int y0, int x1, int y1, float quad[8]) {
  TTR_GUARD_BEGIN
  if (!quad) throw std::runtime_error("null argument");
  if (x1 <= x0 || y1 <= y0) throw std::runtime_error("ttr_region_from_rect: the rectangle is empty");
  Pt2f q[4];
  box_edge_quad(x0, y0, x1, y1, q);
  for (int k = 0; k < 4; ++k) { quad[2 * k] = q[k].x; quad[2 * k + 1] = q[k].y; }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_region_geometry(const float quad[8], int h, int w, int64_t fixed[6], float bbox[4], int* inside) {
  TTR_GUARD_BEGIN
  if (!quad) throw std::runtime_error("null argument");
  if (!region_quad_ok(quad)) throw std::runtime_error("regions: a coordinate is not finite or has |x| >= 32768");
  if (fixed) region_coef(quad, fixed);
  if (bbox) region_bbox(quad, bbox);
  if (inside) *inside = region_inside(quad, h, w) ? 1 : 0;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_regions_to_data_dev(ttr_engine* e, const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets,
                            ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || (n_pages > 0 && !out)) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  e->e->run_regions(pages, n_pages, regions, n, sets, n_sets, res);
  hand_out(res, n_pages, out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_regions_to_data_dev_p(ttr_engine* e, const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets,
                              const char* const* patterns, int n_patterns, const int32_t* pattern_of, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || (n_pages > 0 && !out)) throw std::runtime_error("null argument");
  EngineScope lk(*e->e);
  std::vector<Result> res;
  e->e->run_regions(pages, n_pages, regions, n, sets, n_sets, res, patterns, n_patterns, pattern_of);
  hand_out(res, n_pages, out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_image_regions_to_data(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const ttr_region* regions, int n, const uint32_t* sets,
                              int n_sets, ttr_result** out) {
  return ttr_image_regions_to_data_p(e, img, h, w, row_stride, regions, n, sets, n_sets, nullptr, 0, nullptr, out);
}

int ttr_image_regions_to_data_p(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const ttr_region* regions, int n, const uint32_t* sets,
                                int n_sets, const char* const* patterns, int n_patterns, const int32_t* pattern_of, ttr_result** out) {
  TTR_GUARD_BEGIN
  if (!e || !out) throw std::runtime_error("null argument");
  check_host_image(img, h, w, row_stride);
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("regions");                    // (before the staging buffer, which streamed batches may still read, is touched)
  // the copy is enqueued first (a refused call costs a copy, changes nothing: the staging image is scratch of the synchronous entry points)
  const Engine::StagedPage pg = E.stage_page("regions", img, h, w, row_stride, 0, 0, 0, nullptr, false);   // (checked above, under the reference's text)
  const ttr_page page{pg.data, h, w, pg.stride};
  std::vector<Result> res;
  struct Drain { Engine& E; ~Drain() { (void)hipStreamSynchronize(E.stream); } } drain{E};   // (the caller's image is pageable: the copy ends inside the call, refused or not)
  E.run_regions(&page, 1, regions, n, sets, n_sets, res, patterns, n_patterns, pattern_of);
  hand_out(res, 1, out);
  return 0;
  TTR_GUARD_END(-1)
}

const int32_t* ttr_result_sets(const ttr_result* r) { return r && !r->r.set.empty() ? r->r.set.data() : nullptr; }

int ttr_pack_regions(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* quads, int n, uint8_t* crops_out) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && (!quads || !crops_out))) throw std::runtime_error("null argument");
  check_host_image(img, h, w, row_stride);
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_pack_regions");
  if (n == 0) return 0;
  std::vector<int> rects((size_t)n * 5, 0);
  std::vector<int64_t> coef((size_t)n * 8, 0);
  for (int i = 0; i < n; ++i) {
    if (!region_quad_ok(quads + 8 * (size_t)i)) throw std::runtime_error("ttr_pack_regions: region " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
    rects[5 * (size_t)i + 2] = 1; rects[5 * (size_t)i + 3] = 1;   // (kind 1 reads the coefficients alone; the rectangle only has to be non-empty)
    coef[8 * (size_t)i] = 1;
    region_coef(quads + 8 * (size_t)i, &coef[8 * (size_t)i + 1]);
  }
  const Engine::HostImage image{img, h, w, row_stride ? row_stride : w * 3};   // (known: the one crop call that checks its image, and whose row_stride 0 means packed rows)
  pack_stage(E, &image, rects, coef, kPackRect, crops_out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_parseq_logits_sets(ttr_engine* e, const uint8_t* crops, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, float* logits,
                           float* ar_logits, int32_t* ids) {
  return ttr_parseq_logits_patterns(e, crops, n, sets, n_sets, set_of, nullptr, 0, nullptr, logits, ar_logits, ids);
}

int ttr_parseq_logits_patterns(ttr_engine* e, const uint8_t* crops, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                               const char* const* patterns, int n_patterns, const int32_t* pattern_of, float* logits, float* ar_logits, int32_t* ids) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && (!crops || !logits))) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  const char* what = n_patterns > 0 || pattern_of ? "ttr_parseq_logits_patterns" : "ttr_parseq_logits_sets";
  E.refuse_while_streaming(what);
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (set_of || n_sets > 0 || !(n_patterns > 0 || pattern_of)) E.resolve_row_masks(what, set_of, n, sets, n_sets, table, one);   // (the patterns twin takes set_of == NULL: the engine's own set)
  Engine::PatRows pats;
  const bool with_pats = E.resolve_row_patterns(what, patterns, n_patterns, pattern_of, n, table, one, pats);
  if (n == 0) return 0;
  Engine::RecPass p = stage_crops(E, crops, n, ar_logits != nullptr);
  p.mask = one;   // (one shared mask: by value, the engine's own path)
  const bool best = with_pats && E.pattern_decode == TTR_PATTERN_BEST;   // (the ids are then the likeliest members'; the logits are the same bits)
  if (best) p.best = E.pat_best_out(n);
  if (with_pats) p.pat = E.stage_row_patterns(pats, 0, best ? &p.best.ext : nullptr);
  p.row_masks = E.stage_row_masks(table, 0);
  E.parseq_forward(p);
  fetch_logits(E, p.out, n, logits, ar_logits, ids, what);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_logits_confidence_sets(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* ids,
                               float* probs, float* conf) {
  TTR_GUARD_BEGIN
  if (!e || !set_of || n < 0 || (n > 0 && !logits)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_logits_confidence_sets");
  std::vector<uint32_t> table;
  ClassMask one{};
  E.resolve_row_masks("ttr_logits_confidence_sets", set_of, n, sets, n_sets, table, one);
  if (n == 0) return 0;
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = one; p.row_masks = E.stage_row_masks(table, 0);
  E.parseq_decode(p);
  fetch_decoded(E, p.out, n, ids, probs, conf);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_charset_mask(const char* allow, const char* deny, uint32_t mask[3]) {
  TTR_GUARD_BEGIN
  if (!mask) throw std::runtime_error("null argument");
  static const Tokenizer tok;
  return charset_mask(tok, allow, deny, mask);
  TTR_GUARD_END(-1)
}

int ttr_engine_set_charset(ttr_engine* e, const char* allow, const char* deny) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_engine_set_charset");
  uint32_t m[3];
  charset_mask(E.tok, allow, deny, m);            // (throws before anything changes: a failed call leaves the previous set in place)
  const ClassMask cm = ClassMask::from_allowed(m);
  if (cm.restricts() && E.prec == kBF16)
    throw std::runtime_error("ttr_engine_set_charset: a character set needs an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which take no class mask");
  if (!E.pattern_src.empty()) {                  // the stored pattern under the new set (DESIGN.md "Patterns"): compiled first - a set that empties its language leaves both as they were
    try { E.set_engine_pattern(E.pattern_src.c_str(), cm); }
    catch (const std::runtime_error& ex) { throw std::runtime_error(std::string("ttr_engine_set_charset: the engine's pattern does not survive this set: ") + ex.what()); }
  }
  E.charset = cm;
  return 0;
  TTR_GUARD_END(-1)
}

struct ttr_pattern { ttr::Pattern p; };

int ttr_pattern_compile(const char* pattern, const uint32_t* mask, ttr_pattern** out) {
  TTR_GUARD_BEGIN
  if (!out) throw std::runtime_error("null argument");
  *out = nullptr;
  if (mask && !(mask[0] & 1u)) throw std::runtime_error("ttr_pattern_compile: the mask's bit 0 (the end of the text) must be set");
  static const Tokenizer tok;
  std::unique_ptr<ttr_pattern> p(new ttr_pattern{pattern_compile(tok, pattern, mask)});
  *out = p.release();
  return 0;
  TTR_GUARD_END(-1)
}

void ttr_pattern_free(ttr_pattern* p) { delete p; }

int ttr_pattern_states(const ttr_pattern* p) { return p ? p->p.states : -1; }

int ttr_pattern_min_length(const ttr_pattern* p) { return p ? (int)p->p.mind[(size_t)p->p.start] : -1; }

int ttr_pattern_table(const ttr_pattern* p, const uint16_t** delta, const uint8_t** mind, int* start, int* done) {
  if (!p) return -1;
  if (delta) *delta = p->p.delta.data();
  if (mind) *mind = p->p.mind.data();
  if (start) *start = p->p.start;
  if (done) *done = p->p.done;
  return p->p.rows();
}

int ttr_pattern_matches(const ttr_pattern* p, const char* text) {
  if (!p || !text) return -1;
  static const Tokenizer tok;
  return pattern_matches(tok, p->p, text);
}

int ttr_engine_set_pattern(ttr_engine* e, const char* pattern) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_engine_set_pattern");
  if (pattern && *pattern) {
    if (E.wide != 0.f) throw std::runtime_error("ttr_engine_set_pattern: a pattern does not combine with wide words (a pattern spans the whole text, a piece reads a part of it): ttr_engine_set_wide(e, 0) first");
    if (E.prec == kBF16)
      throw std::runtime_error("ttr_engine_set_pattern: a pattern needs an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which know no automaton");
    if (E.cfg.orient != TTR_ORIENT_OFF)
      throw std::runtime_error("ttr_engine_set_pattern: a pattern does not combine with word orientation (every turn would be forced into the pattern, and their confidences no longer tell them apart): create the engine with orient = TTR_ORIENT_OFF");
    if (E.alts) throw std::runtime_error("ttr_engine_set_pattern: a pattern does not combine with character alternatives: ttr_engine_set_alternatives(e, 0) first");
    if (E.lex_v) throw std::runtime_error("ttr_engine_set_pattern: a pattern does not combine with a lexicon: ttr_engine_set_lexicon(e, NULL, 0, 0) first");
  }
  try { E.set_engine_pattern(pattern, E.charset); }
  catch (const std::runtime_error& ex) { throw std::runtime_error(std::string("ttr_engine_set_pattern: ") + ex.what()); }
  return 0;
  TTR_GUARD_END(-1)
}

const char* ttr_engine_get_pattern(const ttr_engine* e) { return e ? e->e->pattern_src.c_str() : nullptr; }

// the final decode under patterns alone, greedy (logp == nullptr) or best
static void decode_patterns_stage(Engine& E, const char* what, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                                  const char* const* patterns, int n_patterns, const int32_t* pattern_of, int32_t* ids, float* probs, float* conf, float* logp) {
  E.refuse_while_streaming(what);
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (set_of || n_sets > 0) E.resolve_row_masks(what, set_of, n, sets, n_sets, table, one);
  Engine::PatRows pats;
  const bool with_pats = E.resolve_row_patterns(what, patterns, n_patterns, pattern_of, n, table, one, pats);
  if (logp && E.prec == kBF16) throw std::runtime_error(std::string(what) + ": the best decode needs an f16x4 or f32 engine, as patterns do");
  if (n == 0) return;
  if (!with_pats) {   // (no row has a pattern: every row a DONE state under its mask, so that the kernel this stage is about still runs)
    uint32_t m[3];
    std::map<std::vector<uint32_t>, int> start;
    pats.start_of.resize((size_t)n);
    pats.extent_of.assign(2 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) {
      const uint32_t* b = table.empty() ? one.blocked : &table[4 * (size_t)i];
      ClassMask{{b[0], b[1], b[2]}}.allowed(m);
      const std::vector<uint32_t> key(m, m + 3);
      auto it = start.find(key);
      if (it == start.end()) it = start.emplace(key, pats.t.add(pattern_none(m), what)).first;
      pats.start_of[(size_t)i] = it->second;
      pats.extent_of[2 * (size_t)i] = it->second;
    }
  }
  Engine::RecPass p = stage_logits(E, logits, n);
  if (logp) {   // best mode reads each row's class mask itself (the lexicon's table): the masks travel as in ttr_logits_confidence_sets
    p.best = E.pat_best_out(n);
    p.mask = one; p.row_masks = E.stage_row_masks(table, 0);
  }
  p.pat = E.stage_row_patterns(pats, 0, logp ? &p.best.ext : nullptr);
  E.parseq_decode(p);
  if (logp) TTR_HIP_CHECK(hipMemcpyAsync(logp, p.best.logp, (size_t)n * 4, hipMemcpyDeviceToHost, E.stream));
  fetch_decoded(E, p.out, n, ids, probs, conf);
}

int ttr_logits_decode_patterns(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                               const char* const* patterns, int n_patterns, const int32_t* pattern_of, int32_t* ids, float* probs, float* conf) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && !logits)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  decode_patterns_stage(E, "ttr_logits_decode_patterns", logits, n, sets, n_sets, set_of, patterns, n_patterns, pattern_of, ids, probs, conf, nullptr);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_logits_decode_patterns_best(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                                    const char* const* patterns, int n_patterns, const int32_t* pattern_of, int32_t* ids, float* probs, float* conf, float* logp) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && (!logits || !logp))) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  float none = 0.f;
  decode_patterns_stage(E, "ttr_logits_decode_patterns_best", logits, n, sets, n_sets, set_of, patterns, n_patterns, pattern_of, ids, probs, conf, n > 0 ? logp : &none);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_set_pattern_decode(ttr_engine* e, int mode) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (mode != TTR_PATTERN_GREEDY && mode != TTR_PATTERN_BEST)
    throw std::runtime_error("ttr_engine_set_pattern_decode: mode " + std::to_string(mode) + " is neither TTR_PATTERN_GREEDY (0) nor TTR_PATTERN_BEST (1)");
  E.refuse_while_streaming("ttr_engine_set_pattern_decode");
  if (mode == TTR_PATTERN_BEST && E.prec == kBF16)
    throw std::runtime_error("ttr_engine_set_pattern_decode: the best decode needs an f16x4 or f32 engine, as patterns do (the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip)");
  E.pattern_decode = mode;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_pattern_decode(const ttr_engine* e) { return e ? e->e->pattern_decode : -1; }

const float* ttr_result_pattern_logp(const ttr_result* r) { return r && !r->r.pattern_logp.empty() ? r->r.pattern_logp.data() : nullptr; }

int ttr_results_gather_pattern_logp(ttr_result* const* rs, int n, float* logp) {
  if (!rs || n < 0) return -1;
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) return -1;
    const Result& r = rs[i]->r;
    const size_t cnt = r.text.size();
    if (logp) {
      if (r.pattern_logp.size() == cnt) std::copy(r.pattern_logp.begin(), r.pattern_logp.end(), logp + total);
      else std::fill(logp + total, logp + total + cnt, -INFINITY);
    }
    total += cnt;
  }
  return (int)total;
}

int ttr_pattern_best_from_lp(const ttr_pattern* p, const float* lp, int32_t* path, int32_t* len, float* logp) {
  if (!p || !lp) return -1;
  return pattern_best_from_lp(p->p, lp, path, len, logp);
}

int ttr_engine_get_charset(const ttr_engine* e, uint32_t mask[3]) {
  TTR_GUARD_BEGIN
  if (!e || !mask) throw std::runtime_error("null argument");
  const Engine& E = *e->e;
  E.charset.allowed(mask);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_set_alternatives(ttr_engine* e, int k) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (k != 0 && (k < 2 || k > 8)) throw std::runtime_error("ttr_engine_set_alternatives: k must be 0 (off) or lie in 2..8, got " + std::to_string(k));
  E.refuse_while_streaming("ttr_engine_set_alternatives");
  if (k && E.wide != 0.f) throw std::runtime_error("ttr_engine_set_alternatives: character alternatives do not combine with wide words (an item's positions span several rows): ttr_engine_set_wide(e, 0) first");
  if (k && E.prec == kBF16)
    throw std::runtime_error("ttr_engine_set_alternatives: character alternatives need an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which take no class mask");
  if (k && !E.pattern_src.empty())
    throw std::runtime_error("ttr_engine_set_alternatives: character alternatives do not combine with a pattern, and one is set: ttr_engine_set_pattern(e, NULL) first");
  if (k && E.cfg.orient != TTR_ORIENT_OFF)
    throw std::runtime_error("ttr_engine_set_alternatives: character alternatives do not combine with word orientation (the chosen turn's logits are gone by the time of the choice): create the engine with orient = TTR_ORIENT_OFF");
  E.alts = k;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_alternatives(const ttr_engine* e) { return e ? e->e->alts : 0; }

// ---- wide words (DESIGN.md "Wide words")
int ttr_engine_set_wide(ttr_engine* e, float max_aspect) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (!wide_aspect_ok(max_aspect)) throw std::runtime_error("ttr_engine_set_wide: max_aspect must be 0 (off) or a finite value in [2, 64]");
  E.refuse_while_streaming("ttr_engine_set_wide");
  if (max_aspect != 0.f) {
    if (E.cfg.crop_mode != TTR_CROP_RECTIFIED)
      throw std::runtime_error("ttr_engine_set_wide: wide words need crop_mode = TTR_CROP_RECTIFIED (a piece is a kind-1 crop of the word's quad): create the engine with it");
    if (E.cfg.orient != TTR_ORIENT_OFF) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with word orientation: create the engine with orient = TTR_ORIENT_OFF");
    if (E.cfg.chars) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with character boxes: create the engine with chars = 0");
    if (E.alts) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with character alternatives: ttr_engine_set_alternatives(e, 0) first");
    if (E.lex_v) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with a lexicon: ttr_engine_set_lexicon(e, NULL, 0, 0) first");
    if (!E.pattern_src.empty()) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with a pattern: ttr_engine_set_pattern(e, NULL) first");
    if (E.comm) throw std::runtime_error("ttr_engine_set_wide: wide words are read by one engine alone, and a communicator is attached: ttr_engine_attach_comm(e, NULL) first");
    if (E.curved) throw std::runtime_error("ttr_engine_set_wide: wide words do not combine with curved words (a piece is a straight cut of the quad): ttr_engine_set_curved(e, 0) first");
  }
  E.wide = max_aspect;
  return 0;
  TTR_GUARD_END(-1)
}

float ttr_engine_wide(const ttr_engine* e) { return e ? e->e->wide : 0.f; }

// ---- tiled pages (DESIGN.md "Tiled pages")
int ttr_engine_set_tiled(ttr_engine* e, int overlap) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_engine_set_tiled");
  if (overlap != 0) {
    try { (void)tile_plan(32, 32, E.cfg.canvas_size, overlap, E.cfg.mag_ratio); }   // the conditions on (canvas_size, overlap, mag_ratio), by name
    catch (const std::exception& ex) { throw std::runtime_error(std::string("ttr_engine_set_tiled: ") + ex.what()); }
    if (E.comm) throw std::runtime_error("ttr_engine_set_tiled: tiled pages are read by one engine alone, and a communicator is attached: ttr_engine_attach_comm(e, NULL) first");
  }
  E.tiled = overlap;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_tiled(const ttr_engine* e) { return e ? e->e->tiled : 0; }

int ttr_result_tiles(const ttr_result* r) { return r ? r->r.tiles : 0; }

int ttr_tile_plan(int h, int w, int canvas_size, int overlap, float mag_ratio, int* ny, int* nx, int* oy, int* ox, int* ey, int* ex, int* Hc, int* Wc, int* H2, int* W2) {
  TTR_GUARD_BEGIN
  const TilePlan p = tile_plan(h, w, canvas_size, overlap, mag_ratio);
  if (ny) *ny = p.ny;
  if (nx) *nx = p.nx;
  for (int k = 0; k < kTileMaxAxis; ++k) {
    if (oy) oy[k] = k < p.ny ? p.oy[k] : 0;
    if (ey) ey[k] = k < p.ny ? p.ey[k] : 0;
    if (ox) ox[k] = k < p.nx ? p.ox[k] : 0;
    if (ex) ex[k] = k < p.nx ? p.ex[k] : 0;
  }
  if (Hc) *Hc = p.Hc;
  if (Wc) *Wc = p.Wc;
  if (H2) *H2 = p.H2;
  if (W2) *W2 = p.W2;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_stitch_tiles(const float* tiles, int pages, int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2, float* out) {
  TTR_GUARD_BEGIN
  if (!tiles || !out) throw std::runtime_error("null argument");
  if (pages < 1) throw std::runtime_error("ttr_stitch_tiles: pages must be positive");
  stitch_tiles(tiles, pages, tile_plan_from_origins(ny, nx, oy, ox, Hc, Wc, H2, W2), out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_stitch_heat(ttr_engine* e, const float* tiles, int pages, int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2, float* out) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_stitch_heat");
  E.stitch_heat(tiles, pages, tile_plan_from_origins(ny, nx, oy, ox, Hc, Wc, H2, W2), out);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_craft_heatmap_tiled(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int overlap, float* heat_out, size_t cap, int* H2, int* W2) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_craft_heatmap_tiled");
  if (!heat_out) {   // sizes only
    const TilePlan p = tile_plan(h, w, E.cfg.canvas_size, overlap, E.cfg.mag_ratio);
    if (H2) *H2 = p.H2;
    if (W2) *W2 = p.W2;
    return 0;
  }
  E.craft_heatmap_tiled(img, h, w, row_stride, overlap, heat_out, cap, H2, W2, nullptr, 0);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_tile_canvases(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int overlap, uint8_t* canvases, size_t cap) {
  TTR_GUARD_BEGIN
  if (!e || !canvases) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_tile_canvases");
  E.craft_heatmap_tiled(img, h, w, row_stride, overlap, nullptr, 0, nullptr, nullptr, canvases, cap);
  return 0;
  TTR_GUARD_END(-1)
}

const int32_t* ttr_result_piece_first(const ttr_result* r) { return r && !r->r.piece_first.empty() ? r->r.piece_first.data() : nullptr; }

const int32_t* ttr_result_piece_ids(const ttr_result* r) { return r && !r->r.piece_ids.empty() ? r->r.piece_ids.data() : nullptr; }

const float* ttr_result_piece_probs(const ttr_result* r) { return r && !r->r.piece_prob.empty() ? r->r.piece_prob.data() : nullptr; }

const float* ttr_result_piece_confs(const ttr_result* r) { return r && !r->r.piece_conf.empty() ? r->r.piece_conf.data() : nullptr; }

const float* ttr_result_piece_quads(const ttr_result* r) { return r && !r->r.piece_quad.empty() ? r->r.piece_quad.data() : nullptr; }

const int32_t* ttr_result_piece_cuts(const ttr_result* r) { return r && !r->r.piece_cuts.empty() ? r->r.piece_cuts.data() : nullptr; }

int ttr_results_gather_pieces(ttr_result* const* rs, int n, int32_t* first, int32_t* ids, float* probs, float* confs, float* quads, int32_t* cuts) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, op = 0, of = 0;   // items, pieces, first entries so far
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) { if (first) first[of] = 0; of += 1; continue; }
    const Result& r = rs[i]->r;
    const size_t cnt = r.text.size();
    const bool has = cnt > 0 && r.piece_first.size() == cnt + 1;
    const size_t np = has ? (size_t)r.piece_first[cnt] : 0;
    if (first) { if (has) std::copy(r.piece_first.begin(), r.piece_first.end(), first + of); else std::fill(first + of, first + of + cnt + 1, 0); }
    if (ids && np) std::copy(r.piece_ids.begin(), r.piece_ids.end(), ids + 26 * op);
    if (probs && np) std::copy(r.piece_prob.begin(), r.piece_prob.end(), probs + 26 * op);
    if (confs && np) std::copy(r.piece_conf.begin(), r.piece_conf.end(), confs + op);
    if (quads && np) std::copy(r.piece_quad.begin(), r.piece_quad.end(), quads + 8 * op);
    if (cuts) { if (has) std::copy(r.piece_cuts.begin(), r.piece_cuts.end(), cuts + 17 * oi); else std::fill(cuts + 17 * oi, cuts + 17 * (oi + cnt), -1); }
    oi += cnt; op += np; of += cnt + 1;
  }
  return (int)op;
}

int ttr_wide_plan(const float quad[8], float max_aspect, int64_t frame[6]) {
  TTR_GUARD_BEGIN
  if (!quad || !frame) throw std::runtime_error("null argument");
  if (!wide_aspect_ok(max_aspect) || max_aspect == 0.f) throw std::runtime_error("ttr_wide_plan: max_aspect must be a finite value in [2, 64]");
  if (!region_quad_ok(quad)) throw std::runtime_error("ttr_wide_plan: a coordinate is not finite or has |x| >= 32768");
  return wide_plan(quad, max_aspect, frame);
  TTR_GUARD_END(-1)
}

int ttr_wide_profile(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], int n, uint16_t* q) {
  TTR_GUARD_BEGIN
  if (!img || !frame || !q) throw std::runtime_error("null argument");
  if (h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error("ttr_wide_profile: bad image size");
  if (n < 1 || n > kWideMaxPieces) throw std::runtime_error("ttr_wide_profile: n must lie in 1..16");
  wide_profile(img, h, w, row_stride ? row_stride : w * 3, frame, n, q);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_wide_cuts_from_profile(const uint16_t* q, int n, int32_t cuts[17]) {
  TTR_GUARD_BEGIN
  if (!q || !cuts) throw std::runtime_error("null argument");
  if (n < 1 || n > kWideMaxPieces) throw std::runtime_error("ttr_wide_cuts_from_profile: n must lie in 1..16");
  wide_cuts_from_profile(q, n, cuts);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_wide_piece_coef(const int64_t frame[6], int c0, int c1, int64_t row[8]) {
  TTR_GUARD_BEGIN
  if (!frame || !row) throw std::runtime_error("null argument");
  if (c0 < 0 || c1 <= c0 || c1 > kWideMaxU) throw std::runtime_error("ttr_wide_piece_coef: the columns must satisfy 0 <= c0 < c1 <= 2048");
  wide_piece_coef(frame, c0, c1, row);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_wide_piece_quads(const float quad[8], const int32_t* cuts, int n, float* quads) {
  TTR_GUARD_BEGIN
  if (!quad || !cuts || !quads) throw std::runtime_error("null argument");
  if (n < 1 || n > kWideMaxPieces) throw std::runtime_error("ttr_wide_piece_quads: n must lie in 1..16");
  wide_piece_quads(quad, cuts, n, quads);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_wide_cuts(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, float max_aspect, int use_table, int32_t* n_out,
                  int32_t* cuts, uint16_t* profiles, int64_t* coef) {
  TTR_GUARD_BEGIN
  if (!e || nq < 0 || (nq > 0 && !quads)) throw std::runtime_error("null argument");
  check_host_image(img, h, w, row_stride);
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_wide_cuts");
  E.wide_cuts(img, h, w, row_stride, quads, nq, max_aspect, use_table != 0, n_out, cuts, profiles, coef);
  return 0;
  TTR_GUARD_END(-1)
}

// ---- curved words (DESIGN.md "Curved words")
int ttr_engine_set_curved(ttr_engine* e, int on) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (on != 0 && on != 1) throw std::runtime_error("ttr_engine_set_curved: on must be 0 or 1, got " + std::to_string(on));
  E.refuse_while_streaming("ttr_engine_set_curved");
  if (on) {
    if (E.cfg.crop_mode != TTR_CROP_RECTIFIED)
      throw std::runtime_error("ttr_engine_set_curved: curved words need crop_mode = TTR_CROP_RECTIFIED (the spine is sought inside the word's quad): create the engine with it");
    if (E.cfg.orient != TTR_ORIENT_OFF) throw std::runtime_error("ttr_engine_set_curved: curved words do not combine with word orientation (a twin is a straight crop of the quad): create the engine with orient = TTR_ORIENT_OFF");
    if (E.cfg.chars) throw std::runtime_error("ttr_engine_set_curved: curved words do not combine with character boxes (they are cut across the straight quad): create the engine with chars = 0");
    if (E.wide != 0.f) throw std::runtime_error("ttr_engine_set_curved: curved words do not combine with wide words (a piece is a straight cut of the quad): ttr_engine_set_wide(e, 0) first");
    if (E.comm) throw std::runtime_error("ttr_engine_set_curved: curved words are read by one engine alone, and a communicator is attached: ttr_engine_attach_comm(e, NULL) first");
  }
  E.curved = on != 0;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_curved(const ttr_engine* e) { return e && e->e->curved ? 1 : 0; }

const int32_t* ttr_result_curved(const ttr_result* r) { return r && !r->r.curved.empty() ? r->r.curved.data() : nullptr; }

const float* ttr_result_outlines(const ttr_result* r) { return r && !r->r.outline.empty() ? r->r.outline.data() : nullptr; }

const int64_t* ttr_result_spine_knots(const ttr_result* r) { return r && !r->r.spine_knots.empty() ? r->r.spine_knots.data() : nullptr; }

int ttr_results_gather_curved(ttr_result* const* rs, int n, int32_t* curved, float* outlines, int64_t* knots) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, flagged = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    const size_t cnt = r.text.size();
    const bool has = cnt > 0 && r.curved.size() == cnt;
    if (curved) { if (has) std::copy(r.curved.begin(), r.curved.end(), curved + oi); else std::fill(curved + oi, curved + oi + cnt, 0); }
    if (outlines) { if (has) std::copy(r.outline.begin(), r.outline.end(), outlines + 36 * oi); else std::fill(outlines + 36 * oi, outlines + 36 * (oi + cnt), 0.f); }
    if (knots) { if (has) std::copy(r.spine_knots.begin(), r.spine_knots.end(), knots + 36 * oi); else std::fill(knots + 36 * oi, knots + 36 * (oi + cnt), (int64_t)0); }
    if (has) for (int32_t f : r.curved) flagged += f != 0;
    oi += cnt;
  }
  return (int)flagged;
}

static void curve_image_ok(const char* what, const uint8_t* img, int h, int w, int row_stride) {
  if (!img) throw std::runtime_error("null argument");
  if (h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error(std::string(what) + ": bad image size");
}

int ttr_curve_frame(const float quad[8], int64_t frame[6]) {
  TTR_GUARD_BEGIN
  if (!quad || !frame) throw std::runtime_error("null argument");
  if (!region_quad_ok(quad)) throw std::runtime_error("ttr_curve_frame: a coordinate is not finite or has |x| >= 32768");
  curve_frame(quad, frame);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_curve_columns(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], const int64_t* table, int32_t* stats) {
  TTR_GUARD_BEGIN
  if (!frame || !stats) throw std::runtime_error("null argument");
  curve_image_ok("ttr_curve_columns", img, h, w, row_stride);
  curve_columns(img, h, w, row_stride ? row_stride : w * 3, frame, table, stats);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_curve_knots(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], int32_t* flag, int32_t hb[2], int32_t* spine, int64_t* knots, int64_t* knots1) {
  TTR_GUARD_BEGIN
  if (!frame) throw std::runtime_error("null argument");
  curve_image_ok("ttr_curve_knots", img, h, w, row_stride);
  CurveWord cw;
  curve_word(img, h, w, row_stride ? row_stride : w * 3, frame, &cw, knots1);
  if (flag) *flag = cw.flag;
  if (hb) { hb[0] = cw.hb[0]; hb[1] = cw.hb[1]; }
  if (spine) memcpy(spine, cw.spine, sizeof cw.spine);
  if (knots) memcpy(knots, cw.table, sizeof cw.table);
  return cw.flag;
  TTR_GUARD_END(-1)
}

int ttr_curve_crop(const uint8_t* img, int h, int w, int row_stride, const int64_t* knots, uint8_t* crop) {
  TTR_GUARD_BEGIN
  if (!knots || !crop) throw std::runtime_error("null argument");
  curve_image_ok("ttr_curve_crop", img, h, w, row_stride);
  curve_crop(img, h, w, row_stride ? row_stride : w * 3, knots, crop);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_curve_outline(const float quad[8], int flag, const int64_t* knots, float* outline) {
  TTR_GUARD_BEGIN
  if (!quad || !outline || (flag && !knots)) throw std::runtime_error("null argument");
  curve_outline(quad, flag, knots, outline);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_curve_crops(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, int use_table, int32_t* flag, int32_t* hb,
                    int32_t* spine, int64_t* knots, uint8_t* crops) {
  TTR_GUARD_BEGIN
  if (!e || nq < 0 || (nq > 0 && !quads)) throw std::runtime_error("null argument");
  if (!img || h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error("Error reading image from file");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_curve_crops");
  E.curve_crops(img, h, w, row_stride, quads, nq, use_table != 0, flag, hb, spine, knots, crops);
  return 0;
  TTR_GUARD_END(-1)
}

// ---- what the page layers that read a page's ink share: tables, deskew, local ink, selection marks, barcodes (DESIGN.md "Adding a page layer")
// One setter: the guard, the lock, the range refusal (`ranges` behind the function's name, when the layer is being turned on), the streaming refusal, the
// communicator refusal (`alone`: what one engine alone does; null = the layer runs with a communicator), then the store
static int engine_set(ttr_engine* e, const char* fn, bool on, bool ok, const std::string& ranges, const char* alone, const std::function<void(Engine&)>& store) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (on && !ok) throw std::runtime_error(std::string(fn) + ": " + ranges);
  E.refuse_while_streaming(fn);
  if (on && alone && E.comm) throw std::runtime_error(std::string(fn) + ": " + alone + " by one engine alone, and a communicator is attached: ttr_engine_attach_comm(e, NULL) first");
  store(E);
  return 0;
  TTR_GUARD_END(-1)
}

// the checks of the one-page calls: the image (a side of side_cap px or more is refused), the words' quads, and - page_layer_in_ok - both around the layer's own
// range refusal (null = in range)
static void page_image_ok(const char* what, const uint8_t* img, int h, int w, int row_stride, int side_cap) {
  if (!img) throw std::runtime_error("null argument");
  if (h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error(std::string(what) + ": bad image size");
  if (h >= side_cap || w >= side_cap) throw std::runtime_error(std::string(what) + ": a page side of " + std::to_string(side_cap) + " px or more");
}
static void page_quads_ok(const char* what, const float* quads, int nq) {
  for (int i = 0; i < nq; ++i)
    if (!region_quad_ok(quads + 8 * (size_t)i)) throw std::runtime_error(std::string(what) + ": quad " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
}
static void page_layer_in_ok(const char* what, const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, const char* bad_args) {
  if (nq < 0 || (nq > 0 && !quads)) throw std::runtime_error("null argument");
  page_image_ok(what, img, h, w, row_stride, 32768);
  if (bad_args) throw std::runtime_error(std::string(what) + ": " + bad_args);
  page_quads_ok(what, quads, nq);
}
static std::string ink_ranges(int radius, int drop, int polarity) {
  return "drop in 1..255 and polarity in 0..2, got " + std::to_string(radius) + ", " + std::to_string(drop) + " and " + std::to_string(polarity);
}
static void ink_in_ok(const char* what, const uint8_t* img, int h, int w, int row_stride, int radius, int drop, int polarity) {
  page_image_ok(what, img, h, w, row_stride, 32768);
  if (!ink_args_ok(radius, drop, polarity)) throw std::runtime_error(std::string(what) + ": radius must lie in 1..64, " + ink_ranges(radius, drop, polarity));
}

// A layer's three one-page entry points share one body: the host rule under the fixed ink rule, the host rule under the local one (the layer's own check
// then receives 128 in the place of the ink, and fires before the ink rule's), or the engine's stage call
enum PageVia { kViaHost, kViaHostLocal, kViaEngine };
static int layer_ink(PageVia via, const InkRule& rule) { return via == kViaHostLocal ? 128 : rule.ink; }

static std::vector<int32_t> quad_centres(const float* quads, int nq) {   // 64 x the quads' centres [nq][2]
  std::vector<int32_t> centres((size_t)nq * 2);
  for (int i = 0; i < nq; ++i) tables_word_centre(quads + 8 * (size_t)i, &centres[2 * (size_t)i]);
  return centres;
}

// ttr_results_gather_tables / _marks / _barcodes: every result's items (text.size() of them) of each vector into its array (null = not wanted), -1 where a result
// has none - which the first vector decides; returns how many items the last vector places
using ItemVec = std::vector<int32_t> Result::*;
static int items_gather(ttr_result* const* rs, int n, std::initializer_list<std::pair<ItemVec, int32_t*>> outs) {
  if (!rs || n < 0) return -1;
  size_t oi = 0, inside = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    const size_t cnt = r.text.size();
    const bool has = cnt > 0 && (r.*outs.begin()->first).size() == cnt;
    for (const auto& o : outs)
      if (o.second) { if (has) std::copy((r.*o.first).begin(), (r.*o.first).end(), o.second + oi); else std::fill(o.second + oi, o.second + oi + cnt, -1); }
    if (has) for (int32_t c : r.*(outs.end() - 1)->first) inside += c >= 0;
    oi += cnt;
  }
  return (int)inside;
}

// ---- tables (DESIGN.md "Tables")
int ttr_engine_set_tables(ttr_engine* e, int min_len, int ink) {
  return engine_set(e, "ttr_engine_set_tables", min_len != 0, tables_args_ok(min_len, ink),
                    "min_len must be 0 (off) or lie in 16..4096 and ink in 1..255, got " + std::to_string(min_len) + " and " + std::to_string(ink), "tables are found", [&](Engine& E) {
                      E.tables_min_len = min_len;
                      if (min_len) E.tables_ink = ink;
                    });
}

int ttr_engine_tables(const ttr_engine* e, int* ink) {
  if (!e) return 0;
  if (ink) *ink = e->e->tables_ink;
  return e->e->tables_min_len;
}

int ttr_result_table_mode(const ttr_result* r) { return r ? r->r.table_mode : 0; }
int ttr_result_ruling_count(const ttr_result* r) { return r ? (int)(r->r.rulings.size() / 6) : 0; }
const int32_t* ttr_result_rulings(const ttr_result* r) { return r && !r->r.rulings.empty() ? r->r.rulings.data() : nullptr; }
int ttr_result_table_count(const ttr_result* r) { return r ? (int)(r->r.tables.size() / 8) : 0; }
const int32_t* ttr_result_tables(const ttr_result* r) { return r && !r->r.tables.empty() ? r->r.tables.data() : nullptr; }
const int32_t* ttr_result_table_lines(const ttr_result* r, int* n) {
  if (n) *n = r ? (int)r->r.table_lines.size() : 0;
  return r && !r->r.table_lines.empty() ? r->r.table_lines.data() : nullptr;
}
int ttr_result_cell_count(const ttr_result* r) { return r ? (int)(r->r.cells.size() / 9) : 0; }
const int32_t* ttr_result_cells(const ttr_result* r) { return r && !r->r.cells.empty() ? r->r.cells.data() : nullptr; }
const int32_t* ttr_result_item_table(const ttr_result* r) { return r && !r->r.item_table.empty() ? r->r.item_table.data() : nullptr; }
const int32_t* ttr_result_item_cell(const ttr_result* r) { return r && !r->r.item_cell.empty() ? r->r.item_cell.data() : nullptr; }

int ttr_result_cell_text(const ttr_result* r, int c, char* buf, int cap) {
  TTR_GUARD_BEGIN
  if (!r || c < 0 || c >= (int)(r->r.cells.size() / 9) || cap < 0 || (cap > 0 && !buf)) throw std::runtime_error("ttr_result_cell_text: bad cell or buffer");
  const Result& R = r->r;
  std::vector<int> members;
  for (size_t k = 0; k < R.item_cell.size(); ++k) if (R.item_cell[k] == c) members.push_back((int)k);
  std::string text;
  if (!members.empty()) {   // the cell's items through the host line rule (DESIGN.md "Text lines")
    const int m = (int)members.size();
    std::vector<int32_t> cuv((size_t)m * 6), line(m), word(m), order(m), first(m + 1);
    for (int k = 0; k < m; ++k)
      if (!lines_cuv(&R.quad[(size_t)members[k] * 8], &cuv[(size_t)k * 6])) throw std::runtime_error("ttr_result_cell_text: a quad outside the line rule's domain");
    int32_t nl = 0;
    lines_from_cuv(cuv.data(), m, line.data(), word.data(), &nl);
    if (!lines_reading_order(line.data(), word.data(), m, nl, order.data(), first.data())) throw std::runtime_error("ttr_result_cell_text: the line rule gave no numbering");
    for (int l = 0; l < nl; ++l) {
      if (l) text += '\n';
      for (int k = first[l]; k < first[l + 1]; ++k) { if (k > first[l]) text += ' '; text += R.text[(size_t)members[(size_t)order[k]]]; }
    }
  }
  if (cap > 0) { const size_t n = std::min(text.size(), (size_t)cap - 1); memcpy(buf, text.data(), n); buf[n] = 0; }
  return (int)text.size();
  TTR_GUARD_END(-1)
}

int ttr_results_gather_tables(ttr_result* const* rs, int n, int32_t* item_table, int32_t* item_cell) {
  return items_gather(rs, n, {{&Result::item_table, item_table}, {&Result::item_cell, item_cell}});
}

struct TablesOut { int32_t *mode, *counts, *rulings, *tables, *lines, *cells, *item_table, *item_cell; };

static int tables_call(const char* what, PageVia via, ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_len, const InkRule& rule, const float* quads,
                       int nq, const TablesOut& o) {
  TTR_GUARD_BEGIN
  if (via == kViaEngine && !e) throw std::runtime_error("null argument");
  const int ink = layer_ink(via, rule);
  page_layer_in_ok(what, img, h, w, row_stride, quads, nq, tables_args_ok(min_len, ink) ? nullptr :
                   ("min_len must lie in 16..4096 and ink in 1..255, got " + std::to_string(min_len) + " and " + std::to_string(ink)).c_str());
  if (via == kViaHostLocal) ink_in_ok(what, img, h, w, row_stride, rule.radius, rule.drop, rule.polarity);
  std::vector<int32_t> side(kTabSideInts), items((size_t)nq * 2);
  if (via == kViaEngine) {
    Engine& E = *e->e;
    EngineScope lk(E);
    E.refuse_while_streaming(what);
    E.tables_stage(img, h, w, row_stride, 0, 0, min_len, ink, quads, nq, side.data(), items.data(), nullptr, nullptr);
  } else {
    tables_from_page(img, h, w, row_stride ? row_stride : w * 3, min_len, rule, side.data());
    tables_words(side.data(), quad_centres(quads, nq).data(), nq, items.data());
  }
  if (o.mode) *o.mode = side[0];
  int32_t c4[4];
  tables_export(side.data(), c4, o.rulings, o.tables, o.lines, o.cells);
  if (o.counts) { std::copy(c4, c4 + 4, o.counts); o.counts[4] = side[0] == 1 ? side[5] : 0; o.counts[5] = side[0] == 1 ? side[6] : 0; }
  for (int i = 0; i < nq; ++i) {
    if (o.item_table) o.item_table[i] = items[2 * (size_t)i];
    if (o.item_cell) o.item_cell[i] = items[2 * (size_t)i + 1];
  }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_tables_from_page(const uint8_t* img, int h, int w, int row_stride, int min_len, int ink, const float* quads, int nq, int32_t* mode, int32_t* counts,
                         int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell) {
  return tables_call("ttr_tables_from_page", kViaHost, nullptr, img, h, w, row_stride, min_len, ink, quads, nq,
                     {mode, counts, rulings, tables, lines, cells, item_table, item_cell});
}

int ttr_tables_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_len, int radius, int drop, int polarity, const float* quads, int nq, int32_t* mode,
                             int32_t* counts, int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell) {
  return tables_call("ttr_tables_from_page_ink", kViaHostLocal, nullptr, img, h, w, row_stride, min_len, InkRule::local(radius, drop, polarity), quads, nq,
                     {mode, counts, rulings, tables, lines, cells, item_table, item_cell});
}

int ttr_tables_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_len, int ink, const float* quads, int nq, int32_t* mode,
                    int32_t* counts, int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell) {
  return tables_call("ttr_tables_page", kViaEngine, e, img, h, w, row_stride, min_len, ink, quads, nq,
                     {mode, counts, rulings, tables, lines, cells, item_table, item_cell});
}

// ---- deskew (DESIGN.md "Deskew")
static_assert(sizeof(ttr_skew) == sizeof(DeskewRec) && offsetof(ttr_skew, score0) == offsetof(DeskewRec, score0) && offsetof(ttr_skew, mode) == offsetof(DeskewRec, mode),
              "ttr_skew is the engine's record");

int ttr_engine_set_deskew(ttr_engine* e, int max_slope, int gain, int ink) {
  return engine_set(e, "ttr_engine_set_deskew", max_slope != 0, dsk_args_ok(max_slope, gain, ink),
                    "max_slope must be 0 (off) or lie in 1..128, gain in 256..65535 and ink in 1..255, got " + std::to_string(max_slope) + ", " + std::to_string(gain) + " and " +
                        std::to_string(ink),
                    "pages are straightened", [&](Engine& E) {
                      if (max_slope) (void)E.deskew_consts_dev();   // the (C, S) table: formed here, on the host, and handed to the kernels
                      E.deskew_M = max_slope;
                      if (max_slope) { E.deskew_gain = gain; E.deskew_ink = ink; }
                    });
}

int ttr_engine_deskew(const ttr_engine* e, int* gain, int* ink) {
  if (!e) return 0;
  if (gain) *gain = e->e->deskew_gain;
  if (ink) *ink = e->e->deskew_ink;
  return e->e->deskew_M;
}

int ttr_result_skew(const ttr_result* r, ttr_skew* rec) {
  if (!r || !r->r.skew_on) return 0;
  if (rec) memcpy(rec, &r->r.skew, sizeof *rec);
  return 1;
}

int ttr_skew_to_page(const ttr_skew* rec, const float* xy_in, int n, float* xy_out) {
  if (!rec || n < 0 || (n > 0 && (!xy_in || !xy_out))) return -1;
  DeskewRec d;
  memcpy(&d, rec, sizeof d);
  deskew_to_page(d, xy_in, n, xy_out);
  return 0;
}

int ttr_result_to_page(const ttr_result* r, const float* xy_in, int n, float* xy_out) {
  if (!r || n < 0 || (n > 0 && (!xy_in || !xy_out))) return -1;
  if (!r->r.skew_on) { if (xy_out != xy_in) memmove(xy_out, xy_in, (size_t)n * 8); return 0; }
  deskew_to_page(r->r.skew, xy_in, n, xy_out);
  return 0;
}

int ttr_results_gather_skew(ttr_result* const* rs, int n, ttr_skew* recs) {
  if (!rs || n < 0) return -1;
  int turned = 0;
  for (int i = 0; i < n; ++i) {
    const bool has = rs[i] && rs[i]->r.skew_on;
    if (recs) { if (has) memcpy(recs + i, &rs[i]->r.skew, sizeof(ttr_skew)); else memset(recs + i, 0, sizeof(ttr_skew)); }
    turned += has && rs[i]->r.skew.mode == 1;
  }
  return turned;
}

static int deskew_call(const char* what, PageVia via, ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, const InkRule& rule,
                       uint8_t* out_img, ttr_skew* rec, uint64_t* scores) {
  TTR_GUARD_BEGIN
  if (via == kViaEngine && !e) throw std::runtime_error("null argument");
  const int ink = layer_ink(via, rule);
  page_image_ok(what, img, h, w, row_stride, kDskSideCap);
  if (!dsk_args_ok(max_slope, gain, ink))
    throw std::runtime_error(std::string(what) + ": max_slope must lie in 1..128, gain in 256..65535 and ink in 1..255, got " + std::to_string(max_slope) + ", " + std::to_string(gain) +
                             " and " + std::to_string(ink));
  if (via == kViaHostLocal) ink_in_ok(what, img, h, w, row_stride, rule.radius, rule.drop, rule.polarity);
  DeskewRec r;
  if (via == kViaEngine) {
    Engine& E = *e->e;
    EngineScope lk(E);
    E.refuse_while_streaming(what);
    E.deskew_stage(img, h, w, row_stride, 0, 0, max_slope, gain, ink, out_img, &r, scores);
  } else deskew_from_page(img, h, w, row_stride ? row_stride : w * 3, max_slope, gain, rule, out_img, w * 3, &r, scores);
  if (rec) memcpy(rec, &r, sizeof r);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_deskew_from_page(const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int ink, uint8_t* out_img, ttr_skew* rec, uint64_t* scores) {
  return deskew_call("ttr_deskew_from_page", kViaHost, nullptr, img, h, w, row_stride, max_slope, gain, ink, out_img, rec, scores);
}

int ttr_deskew_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int radius, int drop, int polarity, uint8_t* out_img, ttr_skew* rec,
                             uint64_t* scores) {
  return deskew_call("ttr_deskew_from_page_ink", kViaHostLocal, nullptr, img, h, w, row_stride, max_slope, gain, InkRule::local(radius, drop, polarity), out_img, rec, scores);
}

int ttr_deskew_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int ink, uint8_t* out_img, ttr_skew* rec, uint64_t* scores) {
  return deskew_call("ttr_deskew_page", kViaEngine, e, img, h, w, row_stride, max_slope, gain, ink, out_img, rec, scores);
}

// ---- local ink (DESIGN.md "Local ink")
static_assert(sizeof(ttr_ink) == sizeof(InkRec) && offsetof(ttr_ink, sum) == offsetof(InkRec, sum) && offsetof(ttr_ink, w) == offsetof(InkRec, w), "ttr_ink is the engine's record");

int ttr_engine_set_ink(ttr_engine* e, int radius, int drop, int polarity) {
  return engine_set(e, "ttr_engine_set_ink", radius != 0, ink_args_ok(radius, drop, polarity), "radius must be 0 (off) or lie in 1..64, " + ink_ranges(radius, drop, polarity), nullptr,
                    [&](Engine& E) {
                      E.ink_radius = radius;
                      if (radius) { E.ink_drop = drop; E.ink_polarity = polarity; }
                    });
}

int ttr_engine_ink(const ttr_engine* e, int* drop, int* polarity) {
  if (!e) return 0;
  if (drop) *drop = e->e->ink_drop;
  if (polarity) *polarity = e->e->ink_polarity;
  return e->e->ink_radius;
}

int ttr_result_ink(const ttr_result* r, ttr_ink* rec) {
  if (!r || !r->r.ink_on) return 0;
  if (rec) memcpy(rec, &r->r.ink, sizeof *rec);
  return 1;
}

int ttr_results_gather_ink(ttr_result* const* rs, int n, ttr_ink* recs) {
  if (!rs || n < 0) return -1;
  int light = 0;
  for (int i = 0; i < n; ++i) {
    const bool has = rs[i] && rs[i]->r.ink_on;
    if (recs) { if (has) memcpy(recs + i, &rs[i]->r.ink, sizeof(ttr_ink)); else memset(recs + i, 0, sizeof(ttr_ink)); }
    light += has && rs[i]->r.ink.inverted == 1;
  }
  return light;
}

int ttr_ink_from_page(const uint8_t* img, int h, int w, int row_stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, ttr_ink* rec) {
  TTR_GUARD_BEGIN
  ink_in_ok("ttr_ink_from_page", img, h, w, row_stride, radius, drop, polarity);
  InkRec r;
  ink_from_page(img, h, w, row_stride ? row_stride : w * 3, radius, drop, polarity, bits, bitsT, &r);
  if (rec) memcpy(rec, &r, sizeof r);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_ink_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, ttr_ink* rec) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  ink_in_ok("ttr_ink_page", img, h, w, row_stride, radius, drop, polarity);
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_ink_page");
  InkRec r;
  E.ink_stage(img, h, w, row_stride, 0, 0, radius, drop, polarity, bits, bitsT, &r);
  if (rec) memcpy(rec, &r, sizeof r);
  return 0;
  TTR_GUARD_END(-1)
}

// ---- selection marks (DESIGN.md "Selection marks")
static std::string marks_ranges(int min_side, int max_side, int fill, int ink) {
  return "min_side must lie in 8..64, max_side in min_side..128, fill and ink in 1..255, got " + std::to_string(min_side) + ", " + std::to_string(max_side) + ", " +
         std::to_string(fill) + " and " + std::to_string(ink);
}

int ttr_engine_set_marks(ttr_engine* e, int min_side, int max_side, int fill, int ink) {
  return engine_set(e, "ttr_engine_set_marks", min_side != 0, marks_args_ok(min_side, max_side, fill, ink), "min_side must be 0 (off), or " + marks_ranges(min_side, max_side, fill, ink),
                    "selection marks are found", [&](Engine& E) {
                      E.marks_min = min_side;
                      if (min_side) { E.marks_max = max_side; E.marks_fill = fill; E.marks_ink = ink; }
                    });
}

int ttr_engine_marks(const ttr_engine* e, int* max_side, int* fill, int* ink) {
  if (!e) return 0;
  if (max_side) *max_side = e->e->marks_max;
  if (fill) *fill = e->e->marks_fill;
  if (ink) *ink = e->e->marks_ink;
  return e->e->marks_min;
}

int ttr_result_mark_mode(const ttr_result* r) { return r ? r->r.mark_mode : 0; }
int ttr_result_mark_count(const ttr_result* r) { return r ? (int)(r->r.marks.size() / kMarkRec) : 0; }
const int32_t* ttr_result_marks(const ttr_result* r) { return r && !r->r.marks.empty() ? r->r.marks.data() : nullptr; }
const int32_t* ttr_result_item_mark(const ttr_result* r) { return r && !r->r.item_mark.empty() ? r->r.item_mark.data() : nullptr; }

int ttr_results_gather_marks(ttr_result* const* rs, int n, int32_t* item_mark) { return items_gather(rs, n, {{&Result::item_mark, item_mark}}); }

struct MarksOut { int32_t *mode, *counts, *marks, *item_mark; };

static int marks_call(const char* what, PageVia via, ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, const InkRule& rule,
                      const float* quads, int nq, const MarksOut& o) {
  TTR_GUARD_BEGIN
  if (via == kViaEngine && !e) throw std::runtime_error("null argument");
  const int ink = layer_ink(via, rule);
  page_layer_in_ok(what, img, h, w, row_stride, quads, nq, marks_args_ok(min_side, max_side, fill, ink) ? nullptr : marks_ranges(min_side, max_side, fill, ink).c_str());
  if (via == kViaHostLocal) ink_in_ok(what, img, h, w, row_stride, rule.radius, rule.drop, rule.polarity);
  std::vector<int32_t> side(kMarkSideInts), items((size_t)nq);
  if (via == kViaEngine) {
    Engine& E = *e->e;
    EngineScope lk(E);
    E.refuse_while_streaming(what);
    E.marks_stage(img, h, w, row_stride, 0, 0, min_side, max_side, fill, ink, quads, nq, side.data(), items.data(), nullptr);
  } else {
    marks_from_page(img, h, w, row_stride ? row_stride : w * 3, min_side, max_side, fill, rule, side.data());
    marks_items(side.data(), quad_centres(quads, nq).data(), nq, items.data());
  }
  if (o.mode) *o.mode = side[0];
  if (o.counts) { o.counts[0] = side[1]; o.counts[1] = side[2]; o.counts[2] = side[3]; }
  if (o.marks) std::copy(side.begin() + kMarkHdr, side.begin() + kMarkHdr + (size_t)kMarkRec * side[1], o.marks);
  if (o.item_mark) std::copy(items.begin(), items.end(), o.item_mark);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_marks_from_page(const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int ink, const float* quads, int nq, int32_t* mode,
                        int32_t* counts, int32_t* marks, int32_t* item_mark) {
  return marks_call("ttr_marks_from_page", kViaHost, nullptr, img, h, w, row_stride, min_side, max_side, fill, ink, quads, nq, {mode, counts, marks, item_mark});
}

int ttr_marks_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int radius, int drop, int polarity, const float* quads,
                            int nq, int32_t* mode, int32_t* counts, int32_t* marks, int32_t* item_mark) {
  return marks_call("ttr_marks_from_page_ink", kViaHostLocal, nullptr, img, h, w, row_stride, min_side, max_side, fill, InkRule::local(radius, drop, polarity), quads, nq,
                    {mode, counts, marks, item_mark});
}

int ttr_marks_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int ink, const float* quads, int nq, int32_t* mode,
                   int32_t* counts, int32_t* marks, int32_t* item_mark) {
  return marks_call("ttr_marks_page", kViaEngine, e, img, h, w, row_stride, min_side, max_side, fill, ink, quads, nq, {mode, counts, marks, item_mark});
}

// ---- barcodes (DESIGN.md "Barcodes")
static std::string barcodes_ranges(int min_lines, int ink, int symbologies) {
  return "min_lines must lie in 4..256, ink in 1..255 and symbologies in 1..3, got " + std::to_string(min_lines) + ", " + std::to_string(ink) + " and " + std::to_string(symbologies);
}

int ttr_engine_set_barcodes(ttr_engine* e, int min_lines, int ink, int symbologies) {
  return engine_set(e, "ttr_engine_set_barcodes", min_lines != 0, barcodes_args_ok(min_lines, ink, symbologies), "min_lines must be 0 (off), or " + barcodes_ranges(min_lines, ink, symbologies),
                    "barcodes are read", [&](Engine& E) {
                      E.barcodes_min = min_lines;
                      if (min_lines) { E.barcodes_ink = ink; E.barcodes_sym = symbologies; }
                    });
}

int ttr_engine_barcodes(const ttr_engine* e, int* ink, int* symbologies) {
  if (!e) return 0;
  if (ink) *ink = e->e->barcodes_ink;
  if (symbologies) *symbologies = e->e->barcodes_sym;
  return e->e->barcodes_min;
}

int ttr_result_barcode_mode(const ttr_result* r) { return r ? r->r.barcode_mode : 0; }
int ttr_result_barcode_count(const ttr_result* r) { return r ? (int)(r->r.barcodes.size() / kBcRec) : 0; }
const int32_t* ttr_result_barcodes(const ttr_result* r) { return r && !r->r.barcodes.empty() ? r->r.barcodes.data() : nullptr; }
const int32_t* ttr_result_item_barcode(const ttr_result* r) { return r && !r->r.item_barcode.empty() ? r->r.item_barcode.data() : nullptr; }

int ttr_results_gather_barcodes(ttr_result* const* rs, int n, int32_t* item_barcode) { return items_gather(rs, n, {{&Result::item_barcode, item_barcode}}); }

struct BarcodesOut { int32_t *mode, *counts, *barcodes, *item_barcode, *hits, *line_counts; };   // (hits, line_counts: the host form's alone)

static int barcodes_call(const char* what, PageVia via, ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_lines, const InkRule& rule, int symbologies,
                         const float* quads, int nq, const BarcodesOut& o) {
  TTR_GUARD_BEGIN
  if (via == kViaEngine && !e) throw std::runtime_error("null argument");
  const int ink = layer_ink(via, rule);
  page_layer_in_ok(what, img, h, w, row_stride, quads, nq, barcodes_args_ok(min_lines, ink, symbologies) ? nullptr : barcodes_ranges(min_lines, ink, symbologies).c_str());
  if (via == kViaHostLocal) ink_in_ok(what, img, h, w, row_stride, rule.radius, rule.drop, rule.polarity);
  std::vector<int32_t> side(kBcSideInts), items((size_t)nq);
  if (via == kViaEngine) {
    Engine& E = *e->e;
    EngineScope lk(E);
    E.refuse_while_streaming(what);
    E.barcodes_stage(img, h, w, row_stride, 0, 0, min_lines, ink, symbologies, quads, nq, side.data(), items.data(), nullptr, nullptr);
  } else {
    barcodes_from_page(img, h, w, row_stride ? row_stride : w * 3, min_lines, rule, symbologies, side.data(), o.hits, o.line_counts);
    barcodes_items(side.data(), quad_centres(quads, nq).data(), nq, items.data());
  }
  if (o.mode) *o.mode = side[0];
  if (o.counts) std::copy(side.begin() + 1, side.begin() + 7, o.counts);
  if (o.barcodes) std::copy(side.begin() + kBcHdr, side.begin() + kBcHdr + (size_t)kBcRec * side[1], o.barcodes);
  if (o.item_barcode) std::copy(items.begin(), items.end(), o.item_barcode);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_barcodes_from_page(const uint8_t* img, int h, int w, int row_stride, int min_lines, int ink, int symbologies, const float* quads, int nq, int32_t* mode,
                           int32_t* counts, int32_t* barcodes, int32_t* item_barcode, int32_t* hits, int32_t* line_counts) {
  return barcodes_call("ttr_barcodes_from_page", kViaHost, nullptr, img, h, w, row_stride, min_lines, ink, symbologies, quads, nq,
                       {mode, counts, barcodes, item_barcode, hits, line_counts});
}

int ttr_barcodes_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_lines, int symbologies, int radius, int drop, int polarity, const float* quads,
                               int nq, int32_t* mode, int32_t* counts, int32_t* barcodes, int32_t* item_barcode) {
  return barcodes_call("ttr_barcodes_from_page_ink", kViaHostLocal, nullptr, img, h, w, row_stride, min_lines, InkRule::local(radius, drop, polarity), symbologies, quads, nq,
                       {mode, counts, barcodes, item_barcode, nullptr, nullptr});
}

int ttr_barcodes_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_lines, int ink, int symbologies, const float* quads, int nq, int32_t* mode,
                      int32_t* counts, int32_t* barcodes, int32_t* item_barcode) {
  return barcodes_call("ttr_barcodes_page", kViaEngine, e, img, h, w, row_stride, min_lines, ink, symbologies, quads, nq,
                       {mode, counts, barcodes, item_barcode, nullptr, nullptr});
}

int ttr_result_alt_k(const ttr_result* r) { return r ? r->r.alt_k : 0; }

const int32_t* ttr_result_alt_ids(const ttr_result* r, int i) { return r && !r->r.alt_ids.empty() ? &r->r.alt_ids[(size_t)26 * r->r.alt_k * (size_t)i] : nullptr; }

const float* ttr_result_alt_probs(const ttr_result* r, int i) { return r && !r->r.alt_prob.empty() ? &r->r.alt_prob[(size_t)26 * r->r.alt_k * (size_t)i] : nullptr; }

const int32_t* ttr_result_alt_ids_all(const ttr_result* r) { return r && !r->r.alt_ids.empty() ? r->r.alt_ids.data() : nullptr; }

const float* ttr_result_alt_probs_all(const ttr_result* r) { return r && !r->r.alt_prob.empty() ? r->r.alt_prob.data() : nullptr; }

int ttr_results_gather_alts(ttr_result* const* rs, int n, int32_t* ids, float* probs) {
  if (!rs || n < 0) return -1;
  int k = -1;
  for (int i = 0; i < n; ++i) {   // (an empty result - an image that failed, a page without words - has no alternatives to disagree with)
    if (!rs[i] || rs[i]->r.text.empty()) continue;
    if (k >= 0 && rs[i]->r.alt_k != k) return -1;
    k = rs[i]->r.alt_k;
  }
  size_t total = 0, o = 0;
  for (int i = 0; i < n; ++i) {
    if (!rs[i]) continue;
    const Result& r = rs[i]->r;
    total += r.text.size();
    if (ids && !r.alt_ids.empty()) memcpy(ids + o, r.alt_ids.data(), r.alt_ids.size() * 4);
    if (probs && !r.alt_prob.empty()) memcpy(probs + o, r.alt_prob.data(), r.alt_prob.size() * 4);
    o += r.alt_ids.size();
  }
  return (int)total;
}

int ttr_logits_alternatives(ttr_engine* e, const float* logits, int n, int k, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* alt_ids,
                            float* alt_probs) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && !logits) || (sets && n > 0 && !set_of)) throw std::runtime_error("null argument");
  if (k < 2 || k > 8) throw std::runtime_error("ttr_logits_alternatives: k must lie in 2..8, got " + std::to_string(k));
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_logits_alternatives");
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (sets) E.resolve_row_masks("ttr_logits_alternatives", set_of, n, sets, n_sets, table, one);
  if (n == 0) return 0;
  const Engine::AltOut a = E.alts_out(n, k);
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = one; p.row_masks = E.stage_row_masks(table, 0); p.alt = a;
  E.parseq_decode(p);
  const size_t side = Engine::alts_side_bytes(n, k) / 2;   // bytes of either half of the side block
  if (alt_ids) TTR_HIP_CHECK(hipMemcpyAsync(alt_ids, a.ids, side, hipMemcpyDeviceToHost, E.stream));
  if (alt_probs) TTR_HIP_CHECK(hipMemcpyAsync(alt_probs, a.prob, side, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));   // (the side block alone comes back: no RecOut field, so no fetch_decoded)
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_nbest_from_alts(const int32_t* alt_ids, const float* alt_probs, int k, int m, char* texts, size_t cap, float* scores, size_t* need) {
  TTR_GUARD_BEGIN
  if (!alt_ids || !alt_probs) throw std::runtime_error("ttr_nbest_from_alts: null argument");
  if (k < 2 || k > 8) throw std::runtime_error("ttr_nbest_from_alts: k must lie in 2..8, got " + std::to_string(k));
  if (m < 1 || m > 64) throw std::runtime_error("ttr_nbest_from_alts: m must lie in 1..64, got " + std::to_string(m));
  static const Tokenizer tok;
  const std::vector<Reading> rd = nbest_from_alts(tok, alt_ids, alt_probs, k, m);
  size_t bytes = 0;
  for (const Reading& r : rd) bytes += r.text.size() + 1;
  if (need) *need = bytes;
  size_t o = 0;
  for (size_t i = 0; i < rd.size(); ++i) {
    if (scores) scores[i] = rd[i].score;
    if (texts && cap >= bytes) { memcpy(texts + o, rd[i].text.data(), rd[i].text.size()); o += rd[i].text.size(); texts[o++] = '\n'; }
  }
  return (int)rd.size();
  TTR_GUARD_END(-1)
}

int ttr_lexicon_encode(const char* const* words, int n, uint8_t* records) {
  TTR_GUARD_BEGIN
  static const Tokenizer tok;
  lexicon_encode(tok, words, n, records);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_set_lexicon(ttr_engine* e, const char* const* words, int n_words, int m) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  const bool clear = !words && n_words == 0;
  if (!clear) {
    if (!words) throw std::runtime_error("ttr_engine_set_lexicon: null argument");
    if (n_words < 1 || n_words > kLexMaxWords) throw std::runtime_error("ttr_engine_set_lexicon: the number of words must lie in 1..1048576, got " + std::to_string(n_words));
    if (m < 1 || m > 8) throw std::runtime_error("ttr_engine_set_lexicon: m must lie in 1..8, got " + std::to_string(m));
  }
  E.refuse_while_streaming("ttr_engine_set_lexicon");
  if (clear) {                                    // (off is always accepted; the device records stay allocated for the next list)
    E.lex_v = 0; E.lex_m = 0; E.lex_words.clear();
    return 0;
  }
  if (E.wide != 0.f) throw std::runtime_error("ttr_engine_set_lexicon: lexicon matching does not combine with wide words (an entry spans the whole text, a piece reads a part of it): ttr_engine_set_wide(e, 0) first");
  if (E.prec == kBF16)
    throw std::runtime_error("ttr_engine_set_lexicon: lexicon matching needs an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which take no class mask");
  if (!E.pattern_src.empty())
    throw std::runtime_error("ttr_engine_set_lexicon: lexicon matching does not combine with a pattern, and one is set: ttr_engine_set_pattern(e, NULL) first");
  if (E.cfg.orient != TTR_ORIENT_OFF)
    throw std::runtime_error("ttr_engine_set_lexicon: lexicon matching does not combine with word orientation (the chosen turn's logits are gone by the time of the choice): create the engine with orient = TTR_ORIENT_OFF");
  std::vector<uint8_t> rec((size_t)n_words * kLexRecord);
  lexicon_encode(E.tok, words, n_words, rec.data());           // (throws before anything changes: a failed call leaves the previous lexicon in place)
  std::vector<std::string> copy((size_t)n_words);
  for (int i = 0; i < n_words; ++i) copy[(size_t)i] = words[i];
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));                // (no batch is in flight; a stage call's launches may still read the previous records)
  E.lex_v = 0; E.lex_m = 0; E.lex_words.clear();                // (a failed upload leaves no lexicon rather than half of one)
  E.lex_records.ensure(rec.size());
  TTR_HIP_CHECK(hipMemcpy(E.lex_records.p, rec.data(), rec.size(), hipMemcpyHostToDevice));
  E.lex_words.swap(copy);
  E.lex_v = n_words; E.lex_m = m;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_lexicon_size(const ttr_engine* e) { return e ? e->e->lex_v : 0; }

int ttr_engine_lexicon_m(const ttr_engine* e) { return e ? e->e->lex_m : 0; }

const char* ttr_engine_lexicon_word(const ttr_engine* e, int idx) { return e && idx >= 0 && idx < e->e->lex_v ? e->e->lex_words[(size_t)idx].c_str() : nullptr; }

int ttr_result_lex_m(const ttr_result* r) { return r ? r->r.lex_m : 0; }

const int32_t* ttr_result_lex_idx(const ttr_result* r, int i) { return r && i >= 0 && (size_t)i < r->r.lex_idx.size() / (size_t)std::max(r->r.lex_m, 1) ? &r->r.lex_idx[(size_t)r->r.lex_m * (size_t)i] : nullptr; }

const float* ttr_result_lex_logp(const ttr_result* r, int i) { return r && i >= 0 && (size_t)i < r->r.lex_logp.size() / (size_t)std::max(r->r.lex_m, 1) ? &r->r.lex_logp[(size_t)r->r.lex_m * (size_t)i] : nullptr; }

const int32_t* ttr_result_lex_idx_all(const ttr_result* r) { return r && !r->r.lex_idx.empty() ? r->r.lex_idx.data() : nullptr; }

const float* ttr_result_lex_logp_all(const ttr_result* r) { return r && !r->r.lex_logp.empty() ? r->r.lex_logp.data() : nullptr; }

int ttr_logits_lexicon(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* idx, float* logp) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && !logits) || (sets && n > 0 && !set_of)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_logits_lexicon");
  if (!E.lex_v) throw std::runtime_error("ttr_logits_lexicon: no lexicon is set (ttr_engine_set_lexicon)");
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (sets) E.resolve_row_masks("ttr_logits_lexicon", set_of, n, sets, n_sets, table, one);
  if (n == 0) return 0;
  const int M = E.lex_m;
  const Engine::LexOut l = E.lex_out(n, M);
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = one; p.row_masks = E.stage_row_masks(table, 0); p.lex = l;
  E.parseq_decode(p);
  if (idx) TTR_HIP_CHECK(hipMemcpyAsync(idx, l.idx, (size_t)n * M * 4, hipMemcpyDeviceToHost, E.stream));
  if (logp) TTR_HIP_CHECK(hipMemcpyAsync(logp, l.logp, (size_t)n * M * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));   // (as ttr_logits_alternatives: the side block alone)
  return 0;
  TTR_GUARD_END(-1)
}

// fuzzy alignment of the lexicon (DESIGN.md "Lexicon matching", Fuzzy alignment)
static void check_lex_fuzzy(const char* who, int band, float gap, int min_band) {
  if (band < min_band || band > kLexMaxBand) throw std::runtime_error(std::string(who) + ": the band must lie in " + std::to_string(min_band) + "..3, got " + std::to_string(band));
  if (band >= 0 && (!std::isfinite(gap) || gap > 0.f)) throw std::runtime_error(std::string(who) + ": the gap must be finite and <= 0 (the log-probability of one dropped or extra character)");
}

int ttr_engine_set_lexicon_fuzzy(ttr_engine* e, int band, float gap) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  check_lex_fuzzy("ttr_engine_set_lexicon_fuzzy", band, gap, -1);
  E.refuse_while_streaming("ttr_engine_set_lexicon_fuzzy");
  E.lex_band = band; E.lex_gap = band >= 0 ? gap : 0.f;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_engine_lexicon_fuzzy(const ttr_engine* e, int* band, float* gap) {
  if (!e) return -1;
  if (band) *band = e->e->lex_band;
  if (gap) *gap = e->e->lex_gap;
  return 0;
}

int ttr_result_lex_band(const ttr_result* r) { return r ? r->r.lex_band : -1; }

const int32_t* ttr_result_lex_edits(const ttr_result* r, int i) { return r && i >= 0 && (size_t)i < r->r.lex_edits.size() / (size_t)std::max(r->r.lex_m, 1) ? &r->r.lex_edits[(size_t)r->r.lex_m * (size_t)i] : nullptr; }

const int32_t* ttr_result_lex_edits_all(const ttr_result* r) { return r && !r->r.lex_edits.empty() ? r->r.lex_edits.data() : nullptr; }

int ttr_lexicon_fuzzy_from_lp(const float* lp, const uint8_t* records, int n, int band, float gap, float* logp, int32_t* edits) {
  return lexicon_fuzzy_from_lp(lp, records, n, band, gap, logp, edits);
}

int ttr_logits_lexicon_fuzzy(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int band, float gap,
                             int32_t* idx, float* logp, int32_t* edits) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && !logits) || (sets && n > 0 && !set_of)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  check_lex_fuzzy("ttr_logits_lexicon_fuzzy", band, gap, 0);
  E.refuse_while_streaming("ttr_logits_lexicon_fuzzy");
  if (!E.lex_v) throw std::runtime_error("ttr_logits_lexicon_fuzzy: no lexicon is set (ttr_engine_set_lexicon)");
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (sets) E.resolve_row_masks("ttr_logits_lexicon_fuzzy", set_of, n, sets, n_sets, table, one);
  if (n == 0) return 0;
  const int M = E.lex_m;
  const Engine::LexOut l = E.lex_out(n, M, band, gap);
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = one; p.row_masks = E.stage_row_masks(table, 0); p.lex = l;
  E.parseq_decode(p);
  if (idx) TTR_HIP_CHECK(hipMemcpyAsync(idx, l.idx, (size_t)n * M * 4, hipMemcpyDeviceToHost, E.stream));
  if (logp) TTR_HIP_CHECK(hipMemcpyAsync(logp, l.logp, (size_t)n * M * 4, hipMemcpyDeviceToHost, E.stream));
  if (edits) TTR_HIP_CHECK(hipMemcpyAsync(edits, l.edits, (size_t)n * M * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_debug_lexicon_tables(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, float* lp) {
  TTR_GUARD_BEGIN
  if (!e || n < 0 || (n > 0 && (!logits || !lp)) || (sets && n > 0 && !set_of)) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_debug_lexicon_tables");
  std::vector<uint32_t> table;
  ClassMask one = E.charset;
  if (sets) E.resolve_row_masks("ttr_debug_lexicon_tables", set_of, n, sets, n_sets, table, one);
  if (n == 0) return 0;
  Engine::RecPass p = stage_logits(E, logits, n);
  p.mask = one; p.row_masks = E.stage_row_masks(table, 0);
  E.parseq_decode(p);                                              // the masked argmax: the standard block the tables are formed from
  const size_t bytes = (size_t)n * 26 * 96 * 4;
  E.lex_part.ensure(bytes);                                        // (the scorer's partials are scratch between launches)
  launch_lexicon_tables(p.logits, n, p.out.ids, p.out.prob, E.lex_part.as<float>(), E.stream, p.mask, p.row_masks);
  TTR_HIP_CHECK(hipMemcpyAsync(lp, E.lex_part.p, bytes, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_confidence_from_probs(const int32_t* ids, const float* probs, int n_pos, float* char_conf, int* n_chars, float* conf) {
  if (!ids || !probs || n_pos < 0) return -1;
  const int k = confidence_from_probs(ids, probs, n_pos, char_conf, conf);
  if (n_chars) *n_chars = k;
  return k;
}

int ttr_decode_ids(const int32_t* ids, int n, char* buf) {
  TTR_GUARD_BEGIN
  static const Tokenizer tok;
  std::string s = tok.decode(ids, n);
  memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size();
  TTR_GUARD_END(-1)
}

void* ttr_dev_alloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }

void ttr_dev_free(void* p) { if (p) (void)hipFree(p); }

int ttr_dev_upload(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }

int ttr_dev_download(void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }

int ttr_dev_sync(ttr_engine* e) {   // every stream the engine enqueues work on (the recogniser of a streamed batch and the second detector lane have their own)
  if (!e) return -1;
  bool ok = hipStreamSynchronize(e->e->stream) == hipSuccess;
  ok = (hipStreamSynchronize(e->e->recog_stream) == hipSuccess) && ok;
  ok = (hipStreamSynchronize(e->e->lane_stream) == hipSuccess) && ok;
  return ok ? 0 : -1;
}

int ttr_set_profiling(ttr_engine* e, int on) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.profiling = on < 0 ? 0 : (on > 2 ? 2 : on);
  E.prof_recs.clear();
  for (int i = 0; i < 3; ++i) { E.prof_ms[i] = 0; E.prof_flops[i] = 0; E.prof_launches[i] = 0; }
  for (auto& k : E.prof_kinds) { k.ms = 0; k.alg = 0; k.exec = 0; k.launches = 0; k.bytes = 0; }
  return 0;
  TTR_GUARD_END(-1)
}

// The same records by kernel kind, as JSON text: [{"kind": name, "stage": 0|1|2, "launches": n, "ms": t, "alg_flops": a, "exec_flops": x, "alg_bytes": b}, ...]
// (alg_bytes: the detector layers' algorithmic HBM bytes - every operand read once, every result written once, at the engine's plane sizes; 0 where not tallied)
// (alg_flops: 2 x MACs of the layers, SURVEY.md section 8(d)'s figure; exec_flops: what the matrix cores execute for them).  Returns the
// text's length (without the terminator); the text is truncated to cap - 1 characters.
int ttr_get_profile_kinds(ttr_engine* e, char* buf, size_t cap) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.prof_collect();
  std::string s = "[";
  bool first = true;
  for (const auto& k : E.prof_kinds) {
    if (!k.launches) continue;
    std::string name;            // JSON string: quotes, backslashes and control characters escaped
    for (const char ch : k.name) {
      if (ch == '"' || ch == '\\') { name += '\\'; name += ch; }
      else if ((unsigned char)ch < 0x20) { char u[8]; snprintf(u, sizeof u, "\\u%04x", (unsigned)(unsigned char)ch); name += u; }
      else name += ch;
    }
    char line[320];
    snprintf(line, sizeof line, "\", \"stage\": %d, \"launches\": %lld, \"ms\": %.6f, \"alg_flops\": %.6e, \"exec_flops\": %.6e, \"alg_bytes\": %.6e}", k.stage, (long long)k.launches, k.ms, k.alg, k.exec, k.bytes);
    s += first ? "{\"kind\": \"" : ", {\"kind\": \"";
    s += name; s += line; first = false;
  }
  s += "]";
  if (buf && cap) { const size_t n = std::min(s.size(), cap - 1); memcpy(buf, s.data(), n); buf[n] = 0; }
  return (int)s.size();
  TTR_GUARD_END(-1)
}

int ttr_get_profile(ttr_engine* e, double ms[3], double flops[3], long long launches[3]) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.prof_collect();          // records whose events completed since the last batch was finished
  for (int i = 0; i < 3; ++i) { ms[i] = E.prof_ms[i]; flops[i] = E.prof_flops[i]; launches[i] = E.prof_launches[i]; }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_last_stage_ms(ttr_engine* e, float ms[4]) { memcpy(ms, e->e->stage_ms, sizeof(float) * 4); return 0; }

}  // extern "C"
