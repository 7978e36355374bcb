// image_to_data (tuatara.cpp:314-512) over batches of device-resident pages: detector + CCL -> boxes -> crop batch -> recogniser -> strings,
// in four phases so that several batches can be in flight; the multi-GPU exchange points; the sharded latency mode.
#include <deque>
#include <limits>

#include "engine.h"
#include "page_table.h"
#include "tables_rule.h"
#include "barcodes_rule.h"
#include "marks_rule.h"

namespace ttr {

static void push_quad(const RRect& b, std::vector<float>& quad) {   // Result::quad: the word's corners tl, tr, br, bl
  Pt2f q[4]; double cf[6];
  deskew_quad(b, q, cf);
  for (int i = 0; i < 4; ++i) { quad.push_back(q[i].x); quad.push_back(q[i].y); }
}

std::string Result::line_text(int l) const {
  std::string t;
  for (int k = line_first[(size_t)l]; k < line_first[(size_t)l + 1]; ++k) {
    if (k > line_first[(size_t)l]) t += ' ';
    t += text[(size_t)order[(size_t)k]];
  }
  return t;
}

std::string Result::page_text() const {
  std::string t;
  for (int l = 0; l < n_lines; ++l) {
    if (l) t += '\n';
    t += line_text(l);
  }
  return t;
}

std::string Result::block_text(int b) const {
  std::string t;
  for (int k = block_first[(size_t)b]; k < block_first[(size_t)b + 1]; ++k) {
    if (k > block_first[(size_t)b]) t += '\n';
    t += line_text(block_order[(size_t)k]);
  }
  return t;
}

std::string Result::page_text_blocks() const {
  std::string t;
  for (int b = 0; b < n_blocks; ++b) {
    if (b) t += "\n\n";
    t += block_text(b);
  }
  return t;
}

// o = the union of boxes[order[k]] (4 floats each: min x, min y, max x, max y) over k in [k0, k1): a line's box from its words', a block's from its lines'
static void bbox_union(const std::vector<float>& boxes, const std::vector<int32_t>& order, int k0, int k1, float* o) {
  const float inf = std::numeric_limits<float>::infinity();
  o[0] = o[1] = inf; o[2] = o[3] = -inf;
  for (int k = k0; k < k1; ++k) {
    const float* b = &boxes[4 * (size_t)order[k]];
    o[0] = std::min(o[0], b[0]); o[1] = std::min(o[1], b[1]); o[2] = std::max(o[2], b[2]); o[3] = std::max(o[3], b[3]);
  }
}

// crops are ordered by page: page pg owns crops [first[pg], first[pg + 1])
static std::vector<int> page_first(const std::vector<int>& page_of, int pages) {
  std::vector<int> first(pages + 1, 0);
  for (int pg : page_of) first[pg + 1]++;
  for (int pg = 0; pg < pages; ++pg) first[pg + 1] += first[pg];
  return first;
}

// a gathered payload without its padding: rank r's output block of `cap` rows (at r * cap * kRecWords) holds total[r] rows, which land
// rank after rank in g's ids / prob / conf
static void compact_gathered(const int32_t* payload, int cap, const std::vector<int>& total, Engine::Gathered& g) {
  size_t rows = 0;
  for (int t : total) rows += t;
  g.ids.resize(rows * 26); g.prob.resize(rows * 26); g.conf.resize(rows);
  size_t f = 0;
  for (size_t r = 0; r < total.size(); ++r) {
    if (!total[r]) continue;
    const Engine::RecRows v = Engine::rec_rows(payload + r * cap * Engine::kRecWords, cap);
    const size_t t = total[r];
    std::copy(v.ids, v.ids + t * 26, g.ids.data() + f * 26);
    std::copy(v.prob, v.prob + t * 26, g.prob.data() + f * 26);
    std::copy(v.conf, v.conf + t, g.conf.data() + f);
    f += t;
  }
}

void Engine::allgather_host(const void* mine, size_t bytes, void* all) {
  Comm& c = *comm;
  const size_t b = std::max<size_t>(bytes, 1);
  c.h_in.ensure(b); c.h_out.ensure(b * c.world); c.d_in.ensure(b); c.d_out.ensure(b * c.world);
  if (bytes) memcpy(c.h_in.p, mine, bytes);
  TTR_HIP_CHECK(hipMemcpyAsync(c.d_in.p, c.h_in.p, b, hipMemcpyHostToDevice, copy_stream));
  c.tr->all_gather(c.d_in.p, c.d_out.p, b, true, copy_stream);
  TTR_HIP_CHECK(hipMemcpyAsync(c.h_out.p, c.d_out.p, b * c.world, hipMemcpyDeviceToHost, copy_stream));
  TTR_HIP_CHECK(hipStreamSynchronize(copy_stream));
  if (bytes && all) memcpy(all, c.h_out.p, bytes * c.world);
}

void Engine::ccl_launch(const float* d_heat, int p0, int pages, int total, int g, int H2, int W2, int lane) {
  if (p0 == 0) { ccl.ensure(total, H2 * W2, cfg.max_components); h_counters.ensure((size_t)total * 8); }
  ccl.cal_cap_now = tn.gpu_calipers == 2 ? 512 : CclBatch::kCalCap;
  launch_ccl(d_heat, pages, H2, W2, cfg.text_threshold, cfg.link_threshold, cfg.low_text, cfg.min_area, ccl.view(p0, lane), stream);
  if (tn.gpu_calipers) launch_ccl_rects(ccl.view(p0, lane), pages, H2, W2, stream);   // minAreaRect of every candidate, on the stream right behind its row extremes
  TTR_HIP_CHECK(hipMemcpyAsync(h_counters.as<int>() + 2 * p0, ccl.counters.as<int>() + 2 * p0, (size_t)pages * 8, hipMemcpyDeviceToHost, stream));
  while ((int)group_ev.size() <= g) { hipEvent_t e; TTR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); group_ev.push_back(e); }
  TTR_HIP_CHECK(hipEventRecord(group_ev[g], stream));
}

void Engine::ccl_collect(int p0, int pages, int g, int H2, int W2, std::vector<std::vector<RRect>>& det) {
  const int* counters = h_counters.as<int>() + 2 * p0;
  const double tc0 = now_us();
  spin_event(group_ev[g]);
  const double tc1 = now_us();
  // two strided copies bring every page's candidates and row extremes over (width = the busiest page's share)
  int max_c = 0, max_r = 0;
  for (int pg = 0; pg < pages; ++pg) {
    if (counters[2 * pg] > cfg.max_components) throw std::runtime_error("too many text components on a page; raise ttr_config.max_components");
    max_c = std::max(max_c, counters[2 * pg]); max_r = std::max(max_r, counters[2 * pg + 1]);
  }
  const size_t pitch_c = (size_t)max_c * 32, pitch_r = (size_t)max_r * 8;
  std::vector<size_t> off_c(pages), off_r(pages);
  for (int pg = 0; pg < pages; ++pg) { off_c[pg] = pg * (pitch_c / 4); off_r[pg] = pg * (pitch_r / 4); }
  h_cand.ensure(pitch_c * pages + 4); h_rows.ensure(pitch_r * pages + 4);
  int* cand = h_cand.as<int>();
  int* rw = h_rows.as<int>();
  const CclBuffers v = ccl.view(p0);
  if (tn.gpu_calipers && max_c > 0) {
    // the calipers ran on the GPU (ccl_rects_kernel): candidates (for the label order) + 32 bytes of raw result each; sides and angle here (the host's libm)
    const size_t pitch_q = (size_t)max_c * 32;
    h_rects_f.ensure(pitch_q * pages + 4);
    float* rq = h_rects_f.as<float>();
    TTR_HIP_CHECK(hipMemcpy2DAsync(cand, pitch_c, v.cand, (size_t)ccl.max_cand * 32, pitch_c, pages, hipMemcpyDeviceToHost, copy_stream));
    TTR_HIP_CHECK(hipMemcpy2DAsync(rq, pitch_q, v.rects, (size_t)ccl.max_cand * 32, pitch_q, pages, hipMemcpyDeviceToHost, copy_stream));
    TTR_HIP_CHECK(hipEventRecord(copy_ev, copy_stream));
    spin_event(copy_ev);
    const double tc2g = now_us();
    bool pool_full = false;
    for (int pg = 0; pg < pages && !pool_full; ++pg)
      for (int i = 0; i < counters[2 * pg]; ++i)
        if (reinterpret_cast<const int*>(rq + (size_t)pg * (pitch_q / 4) + 8 * (size_t)i)[0] == 2) { pool_full = true; break; }
    if (!pool_full) {
      for (int pg = 0; pg < pages; ++pg) {
        const int n = counters[2 * pg];
        const int* cd = cand + off_c[pg];
        const float* q = rq + (size_t)pg * (pitch_q / 4);
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return cd[8 * a] < cd[8 * b]; });  // label order = ascending root
        for (int i : order) {
          const int kind = reinterpret_cast<const int*>(q + 8 * (size_t)i)[0];
          if (kind != 1 && kind != 3 && kind != 4) continue;
          det[p0 + pg].push_back(finish_min_area_rect(kind, q + 8 * (size_t)i + 1));
        }
      }
      host_us[1] += (float)(tc1 - tc0); host_us[2] += (float)(tc2g - tc1); host_us[3] += (float)(now_us() - tc2g);
      return;
    }
    // (the scratch pool was too small for this group's hulls: the host's calipers below, as without gpu_calipers)
  }
  if (max_c > 0) {
    TTR_HIP_CHECK(hipMemcpy2DAsync(cand, pitch_c, v.cand, (size_t)ccl.max_cand * 32, pitch_c, pages, hipMemcpyDeviceToHost, copy_stream));
    TTR_HIP_CHECK(hipMemcpy2DAsync(rw, pitch_r, v.rows_packed, (size_t)ccl.npx * 8, pitch_r, pages, hipMemcpyDeviceToHost, copy_stream));
    TTR_HIP_CHECK(hipEventRecord(copy_ev, copy_stream));
    spin_event(copy_ev);
  }
  const double tc2 = now_us();
  // the calipers of a page depend on nothing but that page: a few host threads share the group
  parallel_pages(pages, [&](int pg) {
    const int n = counters[2 * pg];
    const int* cd = cand + off_c[pg];
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return cd[8 * a] < cd[8 * b]; });  // label order = ascending root
    for (int i : order) {
      const int* c = &cd[8 * i];
      Component comp{c[0], c[1], c[2], c[3], c[4], c[5], rw + off_r[pg] + 2 * (size_t)c[6]};
      RRect r;
      if (component_to_rect(comp, H2, W2, &r)) det[p0 + pg].push_back(r);
    }
  });
  host_us[1] += (float)(tc1 - tc0); host_us[2] += (float)(tc2 - tc1); host_us[3] += (float)(now_us() - tc2);
}

void Engine::check_pages(std::vector<Page>& pages) const {
  for (size_t i = 0; i < pages.size(); ++i) {
    Page& P = pages[i];
    if (!P.data || P.h <= 0 || P.w <= 0 || P.stride < P.w * 3) throw std::runtime_error("Error reading image from file");  // image.empty(), tuatara.cpp:344
    P.g = page_geometry(P.h, P.w);
    if (P.g.target_h <= 0 || P.g.target_w <= 0) throw std::runtime_error("image too thin to resize");
    if (P.g.h32 != pages[0].g.h32 || P.g.w32 != pages[0].g.w32)
      throw std::runtime_error("mixed-size batch: page " + std::to_string(i) + " (" + std::to_string(P.h) + " x " + std::to_string(P.w) + ") has canvas " + std::to_string(P.g.h32) + " x " +
                               std::to_string(P.g.w32) + ", page 0 (" + std::to_string(pages[0].h) + " x " + std::to_string(pages[0].w) + ") has canvas " + std::to_string(pages[0].g.h32) +
                               " x " + std::to_string(pages[0].g.w32) + ": the pages of a batch must share one detector canvas (ttr_canvas_geometry)");
  }
}

void Engine::upload_page_table(const std::vector<Page>& pages, int sl) {
  const size_t bytes = pages.size() * sizeof(PageRow);
  h_page_table[sl].ensure(bytes); page_table[sl].ensure(bytes);
  PageRow* rows = h_page_table[sl].as<PageRow>();
  for (size_t i = 0; i < pages.size(); ++i) {
    const Page& P = pages[i];
    rows[i] = PageRow{P.data, P.h, P.w, P.stride, 0, make_resize_geom(P.h, P.w, P.g.target_h, P.g.target_w)};
  }
  if (!table_ev[sl]) TTR_HIP_CHECK(hipEventCreateWithFlags(&table_ev[sl], hipEventDisableTiming));
  TTR_HIP_CHECK(hipStreamWaitEvent(stream, table_ev[sl], 0));   // the packers of the slot's previous batch may still read its table on the recogniser's stream (no-op before the first)
  TTR_HIP_CHECK(hipMemcpyAsync(page_table[sl].p, rows, bytes, hipMemcpyHostToDevice, stream));
}

void Engine::upload_tile_table(const PageBatch& B, int sl) {
  const TilePlan& P = B.plan;
  const int T = P.tiles();
  const size_t bytes = (size_t)B.n * T * sizeof(PageRow);
  h_tile_table[sl].ensure(bytes); tile_table[sl].ensure(bytes);
  PageRow* rows = h_tile_table[sl].as<PageRow>();
  for (int i = 0; i < B.n; ++i) {
    const Page& Pg = B.pages[(size_t)i];
    for (int ty = 0; ty < P.ny; ++ty)
      for (int tx = 0; tx < P.nx; ++tx) {
        const int eh = std::min(P.Hc, Pg.h - P.oy[ty]), ew = std::min(P.Wc, Pg.w - P.ox[tx]);   // the page's own extents (pages of a batch share the canvas, not the size)
        if (eh <= 0 || ew <= 0) throw std::logic_error("tiled pages: an empty tile");
        rows[(size_t)i * T + ty * P.nx + tx] = PageRow{Pg.data + (size_t)P.oy[ty] * Pg.stride + (size_t)P.ox[tx] * 3, eh, ew, Pg.stride, 0, make_resize_geom(eh, ew, eh, ew)};
      }
  }
  TTR_HIP_CHECK(hipMemcpyAsync(tile_table[sl].p, rows, bytes, hipMemcpyHostToDevice, stream));   // (read by this batch's resize alone, on this stream)
}

const int* Engine::deskew_consts_dev() {
  if (!dsk_cs_up) {
    std::vector<int32_t>& cs = dsk_cs_host;
    cs.assign(2 * kDskSlopes, 0);
    deskew_consts(cs.data());
    dsk_cs.ensure(cs.size() * 4);
    TTR_HIP_CHECK(hipMemcpy(dsk_cs.p, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));   // (once per engine, from the setter or a stage call: not on the detector's path)
    dsk_cs_up = true;
  }
  return dsk_cs.as<int>();
}

void Engine::deskew_enqueue(PageBatch& B) {
  const int n = B.n, sl = B.slot & 1, M = B.dsk_M;
  const auto [Hcap, Wcap] = B.extent();
  // the upright copies: a uniform batch keeps its form (pages h w 3 bytes apart, rows 3 w), a mixed one gets tight pages at 256-byte offsets
  std::vector<size_t> off((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) {
    const size_t bytes = (size_t)B.pages[i].h * B.pages[i].w * 3;
    off[(size_t)i + 1] = B.mixed ? (off[(size_t)i] + bytes + 255) & ~(size_t)255 : off[(size_t)i] + bytes;
  }
  const size_t rows_b = (size_t)2 * n * sizeof(PageRow), rec_b = (size_t)n * sizeof(DeskewRec);
  dsk_pages[sl].ensure(off[(size_t)n]); dsk_table[sl].ensure(rows_b); h_dsk_table[sl].ensure(rows_b); h_dsk[sl].ensure(rec_b);
  dsk_bits.ensure(tables_bits_slot(Hcap, Wcap) * 8 * n); dsk_bitsT.ensure(tables_bitsT_slot(Hcap, Wcap) * 8 * n);
  dsk_scores.ensure((size_t)n * (2 * M + 1) * 8); dsk_rec.ensure(rec_b);
  const size_t ink_b = ink_recs_bytes(n);
  if (B.ink_radius) { dsk_ink_h.ensure(ink_ws_bytes(Hcap, Wcap, n)); dsk_ink_rec.ensure(ink_b); h_dsk_ink[sl].ensure(ink_b); }   // local ink: its workspace and records
  if (!dsk_cs_up) throw std::logic_error("deskew: the constants table was not uploaded");
  PageRow* rows = h_dsk_table[sl].as<PageRow>();
  for (int i = 0; i < n; ++i) {
    const Page& P = B.pages[i];
    rows[i] = PageRow{P.data, P.h, P.w, P.stride, 0, ResizeGeom{}};
    rows[n + i] = PageRow{dsk_pages[sl].as<uint8_t>() + off[(size_t)i], P.h, P.w, P.w * 3, 0, ResizeGeom{}};
  }
  // the slot's previous batch: its packers and page layers may still read the slot's upright pages on the recogniser's stream (a no-op before the first)
  TTR_HIP_CHECK(hipStreamWaitEvent(stream, done_ev[sl], 0));
  TTR_HIP_CHECK(hipMemcpyAsync(dsk_table[sl].p, rows, rows_b, hipMemcpyHostToDevice, stream));
  const PageRow* src = dsk_table[sl].as<PageRow>();
  // step 1: the source pages' ink - under the local rule when the engine's radius is set (DESIGN.md "Local ink"), the same bitmaps either way
  if (B.ink_radius) launch_ink_local(nullptr, 0, 0, 0, 0, src, n, Hcap, Wcap, B.ink_radius, B.ink_drop, B.ink_polarity, dsk_ink_h.as<uint32_t>(), dsk_ink_rec.as<InkRec>(),
                                     dsk_bits.as<uint64_t>(), dsk_bitsT.as<uint64_t>(), stream);
  else launch_table_ink(nullptr, 0, 0, 0, 0, src, n, Hcap, Wcap, deskew_ink, dsk_bits.as<uint64_t>(), dsk_bitsT.as<uint64_t>(), stream);
  launch_deskew_score(dsk_bits.as<uint64_t>(), src, n, Hcap, Wcap, M, dsk_scores.as<uint64_t>(), stream);
  launch_deskew_rotate(src, src + n, n, Hcap, Wcap, M, deskew_gain, dsk_scores.as<uint64_t>(), dsk_cs.as<int>(), dsk_rec.as<DeskewRec>(), stream);
  TTR_HIP_CHECK(hipMemcpyAsync(h_dsk[sl].p, dsk_rec.p, rec_b, hipMemcpyDeviceToHost, stream));   // the records: complete before the batch's components are (same stream, ahead of the detector)
  if (B.ink_radius) TTR_HIP_CHECK(hipMemcpyAsync(h_dsk_ink[sl].p, dsk_ink_rec.p, ink_b, hipMemcpyDeviceToHost, stream));   // ... and the ink records with them
  for (int i = 0; i < n; ++i) { B.pages[i].data = rows[n + i].data; B.pages[i].stride = B.pages[i].w * 3; }
}

Engine::StagedPage Engine::stage_page(const char* what_, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int side_cap, const char* bad_args,
                                      bool check) {
  const std::string what(what_);
  if (check && (!img || h <= 0 || w <= 0 || (row_stride && row_stride < w * 3))) throw std::runtime_error(what + ": bad image size");
  if (side_cap && (h >= side_cap || w >= side_cap)) throw std::runtime_error(what + ": a page side of " + std::to_string(side_cap) + " px or more");
  if (bad_args) throw std::runtime_error(what + ": " + bad_args);
  const int ds = dev_stride ? dev_stride : w * 3;
  if (dev_offset < 0 || ds < w * 3) throw std::runtime_error(what + ": bad device offset or stride");
  staging_img.ensure((size_t)dev_offset + (size_t)ds * h);
  uint8_t* d_img = staging_img.as<uint8_t>() + dev_offset;
  TTR_HIP_CHECK(hipMemcpy2DAsync(d_img, (size_t)ds, img, row_stride ? row_stride : w * 3, (size_t)w * 3, h, hipMemcpyHostToDevice, stream));
  return StagedPage{d_img, ds};
}

const PageRow* Engine::staged_page_table(const StagedPage& pg, int h, int w) {
  upload_page_table(std::vector<Page>(1, Page{pg.data, h, w, pg.stride, CanvasGeom{h, w, h, w, 1.f}}), 0);
  return page_table[0].as<PageRow>();
}

void Engine::stage_centres(const char* what, const float* quads, int nq) {
  const size_t in_ints = (size_t)nq * 2 + 2;
  rects_dev.ensure(in_ints * 4); h_rects[0].ensure(in_ints * 4);
  int32_t* in = h_rects[0].as<int32_t>();
  for (int i = 0; i < nq; ++i) {
    if (!region_quad_ok(quads + 8 * (size_t)i)) throw std::runtime_error(std::string(what) + ": quad " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
    tables_word_centre(quads + 8 * (size_t)i, in + 2 * (size_t)i);
  }
  in[2 * (size_t)nq] = 0; in[2 * (size_t)nq + 1] = nq;
  TTR_HIP_CHECK(hipMemcpyAsync(rects_dev.p, in, in_ints * 4, hipMemcpyHostToDevice, stream));
}

void Engine::deskew_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int max_slope, int gain, int ink, uint8_t* out,
                          DeskewRec* rec, uint64_t* scores) {
  const StagedPage pg = stage_page("ttr_deskew_page", img, h, w, row_stride, dev_offset, dev_stride, kDskSideCap,
                                   dsk_args_ok(max_slope, gain, ink) ? nullptr : "max_slope must lie in 1..128, gain in 256..65535 and ink in 1..255");
  const size_t out_b = (size_t)h * w * 3, nsc = (size_t)2 * max_slope + 1;
  dsk_pages[0].ensure(out_b); dsk_table[0].ensure(2 * sizeof(PageRow));
  dsk_bits.ensure(tables_bits_slot(h, w) * 8); dsk_bitsT.ensure(tables_bitsT_slot(h, w) * 8); dsk_scores.ensure(nsc * 8); dsk_rec.ensure(sizeof(DeskewRec));
  const int* cs = deskew_consts_dev();
  const PageRow rows[2] = {PageRow{pg.data, h, w, pg.stride, 0, ResizeGeom{}}, PageRow{dsk_pages[0].as<uint8_t>(), h, w, w * 3, 0, ResizeGeom{}}};
  TTR_HIP_CHECK(hipMemcpyAsync(dsk_table[0].p, rows, sizeof rows, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));                        // (rows is on the stack)
  const PageRow* src = dsk_table[0].as<PageRow>();
  launch_table_ink(nullptr, 0, 0, 0, 0, src, 1, h, w, ink, dsk_bits.as<uint64_t>(), dsk_bitsT.as<uint64_t>(), stream);
  launch_deskew_score(dsk_bits.as<uint64_t>(), src, 1, h, w, max_slope, dsk_scores.as<uint64_t>(), stream);
  launch_deskew_rotate(src, src + 1, 1, h, w, max_slope, gain, dsk_scores.as<uint64_t>(), cs, dsk_rec.as<DeskewRec>(), stream);
  DeskewRec r{};
  std::vector<uint64_t> sc(nsc);
  TTR_HIP_CHECK(hipMemcpyAsync(&r, dsk_rec.p, sizeof r, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipMemcpyAsync(sc.data(), dsk_scores.p, nsc * 8, hipMemcpyDeviceToHost, stream));
  if (out) TTR_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)w * 3, dsk_pages[0].p, (size_t)w * 3, (size_t)w * 3, h, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  std::string why;
  if (!deskew_rec_valid(r, max_slope, h, w, dsk_cs_host.data(), &why)) throw std::runtime_error("ttr_deskew_page: the record holds " + why);
  if (rec) *rec = r;
  if (scores) std::copy(sc.begin(), sc.end(), scores);
}

void Engine::detect_enqueue(PageBatch& B) {
  range_use(kRangeDet0 + (B.slot & 1));   // the detector's kernels of this batch watch its own word (engine.h)
  if (!B.mixed) {                         // a uniform batch: every page is its entry point's scalars
    if (B.h <= 0 || B.w <= 0) throw std::runtime_error("Error reading image from file");  // image.empty(), tuatara.cpp:344
    const CanvasGeom g = page_geometry(B.h, B.w);
    if (g.target_h <= 0 || g.target_w <= 0) throw std::runtime_error("image too thin to resize");
    B.pages.resize((size_t)B.n);
    for (int i = 0; i < B.n; ++i) B.pages[i] = Page{B.d_pages + (size_t)i * B.h * B.w * 3, B.h, B.w, B.w * 3, g};
  } else {
    check_pages(B.pages);                 // (before anything is enqueued)
  }
  const int side = std::max(B.extent().h, B.extent().w);   // the longest page side: the tables and marks rules' coordinates are below 32768 (likewise before anything is enqueued)
  if (tables_min_len && side >= 32768) throw std::runtime_error("tables: a page side of 32768 px or more: ttr_engine_set_tables(e, 0, 0) first");
  if (marks_min && side >= 32768) throw std::runtime_error("marks: a page side of 32768 px or more: ttr_engine_set_marks(e, 0, 0, 0, 0) first");
  if (barcodes_min && side >= 32768) throw std::runtime_error("barcodes: a page side of 32768 px or more: ttr_engine_set_barcodes(e, 0, 0, 0) first");
  // Deskew (DESIGN.md "Deskew"): every page's skew is estimated and the batch's pages become upright copies in the slot's buffer; everything below and behind
  // reads B.pages as ever.  Off: nothing here runs.
  B.ink_radius = ink_radius; B.ink_drop = ink_drop; B.ink_polarity = ink_polarity;   // local ink: fixed for the batch here (the setter refuses while batches stream)
  B.dsk_M = deskew_M;
  if (B.dsk_M) {
    if (side >= kDskSideCap) throw std::runtime_error("deskew: a page side of 8192 px or more: ttr_engine_set_deskew(e, 0, 0, 0) first");
    deskew_enqueue(B);
  }
  const Page& P0 = B.pages[0];
  B.H = P0.g.h32; B.W = P0.g.w32; B.H2 = B.H / 2; B.W2 = B.W / 2;
  const int n = B.n, H = B.H, W = B.W, H2 = B.H2, W2 = B.W2;
  // Tiled pages (DESIGN.md "Tiled pages"): the pages above keep their own scale; one larger than the detector canvas goes through the detector as T overlapping
  // tiles on a canvas of Hc x Wc (nc = n T canvases into tile_heat), and tile_stitch_kernel joins their maps into `heat` behind the last group.  A page of one
  // tile IS its canvas: it takes the path below as it stands.  Off: nc, Hc, Wc are n, H, W and nothing here differs.
  B.tiles = 0;
  if (tiled) { B.plan = tile_plan(P0.h, P0.w, cfg.canvas_size, tiled, cfg.mag_ratio); B.tiles = B.plan.tiles(); }
  const bool til = B.tiles > 1;
  const int T = til ? B.tiles : 1, nc = n * T, Hc = til ? B.plan.Hc : H, Wc = til ? B.plan.Wc : W, Hc2 = Hc / 2, Wc2 = Wc / 2;
  canvas.ensure((size_t)nc * Hc * Wc * 3);
  heat.ensure((size_t)n * H2 * W2 * 2 * 4);
  if (til) tile_heat.ensure((size_t)nc * Hc2 * Wc2 * 2 * 4);
  float* const craft_out = til ? tile_heat.as<float>() : heat.as<float>();
  if (B.mixed) upload_page_table(B.pages, B.slot & 1);   // ahead of the resize; the batch's packers read it later (engine.h)
  if (til) upload_tile_table(B, B.slot & 1);
  TTR_HIP_CHECK(hipEventRecord(ev[0], stream));
  if (til) launch_resize_pad_pages(tile_table[B.slot & 1].as<PageRow>(), canvas.as<uint8_t>(), Hc, Wc, 1, nc, stream);   // the identity path: a tile's canvas is its window's bytes
  else if (B.mixed) launch_resize_pad_pages(page_table[B.slot & 1].as<PageRow>(), canvas.as<uint8_t>(), H, W, 1, n, stream);
  else launch_resize_pad_u8(P0.data, P0.h, P0.w, P0.stride, canvas.as<uint8_t>(), P0.g.target_h, P0.g.target_w, H, W, 1, stream, n, (size_t)P0.h * P0.w * 3);
  // CRAFT in groups of <= craft_group pages: bounds the activation workspace and keeps every tensor inside the 2 GiB window the kernels' 32-bit buffer
  // offsets address.  Each group's CCL follows its CRAFT, so the host reads group g's components back (and runs its calipers) while the GPU is busy with group g + 1.
  // f16x4 (planes of f16: four or six bytes per value): the cap is what the widest tensor of the configuration in force allows - with first_fused 128 channels at half
  // resolution as pairs, 100.7 MB per 1024 x 768 page: 16-page groups, half the launches of 8-page ones (engine.h: craft_group_pages)
  int GP = tn.craft_group;
  if (prec == kSplit) GP = craft_group_pages(Hc, Wc, nc, tn.craft_group, craft_group_cfg());
  last_craft_group = GP;
  B.group = til ? n : GP;                 // (tiled: the pages' CCL is one group behind the stitch)
  const int groups = (nc + GP - 1) / GP;
  // Two detector lanes (tn.craft_lanes, engine.h): odd groups on lane_stream with their own workspaces, half a group behind the even ones, so that a lane's
  // matrix-bound full-resolution layers run beside the other lane's HBM-bound U-Net tail and head (a group alone: 9.7 ms of the one, 2.8 of the other)
  const bool two = prec == kSplit && tn.craft_lanes == 2 && groups >= 2;
  ccl.split_pool = two && !til;
  if (two) {
    TTR_HIP_CHECK(hipEventRecord(resize_done, stream));
    TTR_HIP_CHECK(hipStreamWaitEvent(lane_stream, resize_done, 0));     // (the canvas; and everything the main stream held before it: the previous batch's detector)
    lane_go_pending = true;
  }
  struct LaneGuard {   // the odd groups borrow the engine's `stream` and workspace selector; restored also when a launch throws
    Engine& E; bool on = false;
    void enter() { E.prof_break(); std::swap(E.stream, E.lane_stream); E.ws_sel = 1; on = true; }
    void leave() { if (on) { E.prof_break(); std::swap(E.stream, E.lane_stream); E.ws_sel = 0; on = false; } }
    ~LaneGuard() { if (on) { std::swap(E.stream, E.lane_stream); E.ws_sel = 0; } E.lane_go_pending = false; }
  } lane_guard{*this};
  for (int gi = 0; gi < groups; ++gi) {
    const int p0 = gi * GP, cnt = std::min(GP, nc - p0);
    const int lane = two ? (gi & 1) : 0;
    if (lane) {
      lane_guard.enter();
      if (gi == 1) TTR_HIP_CHECK(hipStreamWaitEvent(stream, lane_go, 0));   // (recorded inside group 0's forward pass, behind slice3.20)
    }
    craft_forward(canvas.as<uint8_t>() + (size_t)p0 * Hc * Wc * 3, cnt, Hc, Wc, craft_out + (size_t)p0 * Hc2 * Wc2 * 2);
    if (!til) {
      if (gi == groups - 1) TTR_HIP_CHECK(hipEventRecord(ev[1], stream));
      ccl_launch(heat.as<float>() + (size_t)p0 * H2 * W2 * 2, p0, cnt, n, gi, H2, W2, lane);
    }
    if (lane) {
      if (gi + 2 >= groups) TTR_HIP_CHECK(hipEventRecord(lane_done, stream));   // this lane's last group
      lane_guard.leave();
    }
  }
  if (two) TTR_HIP_CHECK(hipStreamWaitEvent(stream, lane_done, 0));       // the batch's detector is complete when the main stream gets here
  int ccl_groups = groups;
  if (til) {                                                              // every tile map is written (both lanes are through): the page maps, then the pages' CCL
    prof_break();
    launch_tile_stitch(tile_heat.as<float>(), heat.as<float>(), B.plan, n, stream);
    TTR_HIP_CHECK(hipEventRecord(ev[1], stream));
    ccl_launch(heat.as<float>(), 0, n, n, 0, H2, W2, 0);
    ccl_groups = 1;
  }
  if (cfg.chars) keep_batch_map(B);                                       // character boxes: the next batch's detector overwrites tnorm before this batch's recogniser runs
  range_fetch(kRangeDet0 + (B.slot & 1));
  while ((int)group_ev.size() <= ccl_groups) { hipEvent_t e; TTR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); group_ev.push_back(e); }
  TTR_HIP_CHECK(hipEventRecord(group_ev[ccl_groups], stream));                // (behind the word's copy: detect_collect_local waits for it)
  B.det_groups = ccl_groups;
  TTR_HIP_CHECK(hipEventRecord(ev[2], stream));
}

int Engine::craft_groups_plain(const uint8_t* d_canvas, int nc, int H, int W, float* d_heat) {
  int GP = tn.craft_group;
  if (prec == kSplit) GP = craft_group_pages(H, W, nc, tn.craft_group, craft_group_cfg());
  for (int p0 = 0; p0 < nc; p0 += GP)
    craft_forward(d_canvas + (size_t)p0 * H * W * 3, std::min(GP, nc - p0), H, W, d_heat + (size_t)p0 * (H / 2) * (W / 2) * 2);
  return GP;
}

void Engine::stitch_heat(const float* tiles, int pages, const TilePlan& plan, float* out) {
  if (!tiles || !out) throw std::runtime_error("ttr_stitch_heat: null argument");
  if (pages < 1 || pages > 256) throw std::runtime_error("ttr_stitch_heat: pages must lie in 1..256, got " + std::to_string(pages));
  const size_t in_bytes = (size_t)pages * plan.tiles() * (plan.Hc / 2) * (plan.Wc / 2) * 8, out_bytes = (size_t)pages * plan.H2 * plan.W2 * 8;
  tile_heat.ensure(in_bytes); heat.ensure(out_bytes);
  TTR_HIP_CHECK(hipMemcpyAsync(tile_heat.p, tiles, in_bytes, hipMemcpyHostToDevice, stream));
  launch_tile_stitch(tile_heat.as<float>(), heat.as<float>(), plan, pages, stream);
  TTR_HIP_CHECK(hipMemcpyAsync(out, heat.p, out_bytes, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
}

void Engine::craft_heatmap_tiled(const uint8_t* img, int h, int w, int row_stride, int overlap, float* out, size_t cap, int* H2, int* W2, uint8_t* canvases_out,
                                 size_t canvases_cap) {
  if (!img || h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error("Error reading image from file");
  PageBatch B;
  B.n = 1;
  B.plan = tile_plan(h, w, cfg.canvas_size, overlap, cfg.mag_ratio);   // (every refusal before anything is enqueued)
  const TilePlan& P = B.plan;
  const int T = P.tiles();
  const size_t canvas_bytes = (size_t)T * P.Hc * P.Wc * 3, map_floats = (size_t)P.H2 * P.W2 * 2;
  if (H2) *H2 = P.H2;
  if (W2) *W2 = P.W2;
  if (out && cap < map_floats) throw std::runtime_error("tiled heat map: the buffer holds " + std::to_string(cap) + " floats, the page map has " + std::to_string(map_floats));
  if (canvases_out && canvases_cap < canvas_bytes) throw std::runtime_error("tile canvases: the buffer holds " + std::to_string(canvases_cap) + " bytes, the tiles have " + std::to_string(canvas_bytes));
  const StagedPage pg = stage_page("ttr_craft_heatmap_tiled", img, h, w, row_stride, 0, 0, 0, nullptr, false);   // (checked above, under the reference's text)
  B.pages.assign(1, Page{pg.data, h, w, pg.stride, CanvasGeom{h, w, P.hp, P.wp, 1.f}});
  canvas.ensure(canvas_bytes);
  upload_tile_table(B, 0);
  launch_resize_pad_pages(tile_table[0].as<PageRow>(), canvas.as<uint8_t>(), P.Hc, P.Wc, 1, T, stream);
  if (canvases_out) TTR_HIP_CHECK(hipMemcpyAsync(canvases_out, canvas.p, canvas_bytes, hipMemcpyDeviceToHost, stream));
  if (out) {
    tile_heat.ensure((size_t)T * (P.Hc / 2) * (P.Wc / 2) * 8); heat.ensure(map_floats * 4);
    craft_groups_plain(canvas.as<uint8_t>(), T, P.Hc, P.Wc, tile_heat.as<float>());
    launch_tile_stitch(tile_heat.as<float>(), heat.as<float>(), P, 1, stream);
    TTR_HIP_CHECK(hipMemcpyAsync(out, heat.p, map_floats * 4, hipMemcpyDeviceToHost, stream));
    range_fetch(kRangeStage);
  }
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  if (out) range_verify(kRangeStage, "ttr_craft_heatmap_tiled");
}

void Engine::detect_collect(PageBatch& B, std::exception_ptr pre) {
  if (!comm) { if (pre) std::rethrow_exception(pre); detect_collect_local(B); return; }
  std::exception_ptr err = pre;
  if (!err) { try { detect_collect_local(B); } catch (...) { err = std::current_exception(); } }
  const int world = comm->world, n = B.n;
  int32_t hdr[2] = {err ? -1 : 0, n};
  std::vector<int32_t> all(2 * (size_t)world, 0);
  allgather_host(hdr, 8, all.data());
  if (err) std::rethrow_exception(err);
  for (int r = 0; r < world; ++r) {
    if (all[2 * r] < 0) throw std::runtime_error("multi-GPU batch: rank " + std::to_string(r) + " failed before the exchange; the batch is dropped on every rank");
    if (all[2 * r + 1] != n) throw std::runtime_error("multi-GPU batch: rank " + std::to_string(r) + " passed " + std::to_string(all[2 * r + 1]) + " pages, this rank " + std::to_string(n) +
                                                      ": every rank must push the same number of pages per batch");
  }
  // counts (host-side exchange on the control communicator), so that every rank knows the payload's size
  std::vector<int32_t> mine(n, 0);
  for (int pg : B.page_of) mine[pg]++;
  B.all_counts.assign((size_t)world * n, 0);
  allgather_host(mine.data(), (size_t)n * 4, B.all_counts.data());
  B.cap = GatherLayout::from_counts(B.all_counts.data(), world, n).cap;
}

void Engine::detect_collect_local(PageBatch& B) {
  const int n = B.n, GP = B.group, groups = (n + GP - 1) / GP;
  std::vector<std::vector<RRect>> dets(n);
  B.boxes.assign(n, std::vector<RRect>());
  B.rects.clear(); B.page_of.clear(); B.coef.clear(); B.twin.clear();   // x0,y0,x1,y1,page per crop; page index per crop; rectified crops' coefficients; twins'
  const int K = orient_k();
  std::vector<Pt2f> oq;                                        // orient != 0: each word's quad Q (DESIGN.md "Word orientation")
  std::vector<float> wq;                                       // wide != 0 or curved: each word's quad (DESIGN.md "Wide words", "Curved words")
  host_us[1] = host_us[2] = host_us[3] = 0.f;
  B.tab_min_len = tables_min_len; B.tab_ink = tables_ink; B.tab_centres.clear();   // tables: fixed for the batch here (the setter refuses while batches stream)
  B.mark_min = marks_min; B.mark_max = marks_max; B.mark_fill = marks_fill; B.mark_ink = marks_ink;   // selection marks: likewise
  B.bc_min = barcodes_min; B.bc_ink = barcodes_ink; B.bc_sym = barcodes_sym;                           // barcodes: likewise
  std::vector<float> tq;
  for (int gi = 0; gi < groups; ++gi) ccl_collect(gi * GP, std::min(GP, n - gi * GP), gi, B.H2, B.W2, dets);
  // deskew: the batch's records were copied ahead of its detector on the same stream, so they are here; taken now, before the slot's next batch overwrites them
  B.dsk_recs.clear();
  if (B.dsk_M) B.dsk_recs.assign(h_dsk[B.slot & 1].as<DeskewRec>(), h_dsk[B.slot & 1].as<DeskewRec>() + n);
  B.dsk_ink_recs.clear();
  if (B.dsk_M && B.ink_radius) B.dsk_ink_recs.assign(h_dsk_ink[B.slot & 1].as<InkRec>(), h_dsk_ink[B.slot & 1].as<InkRec>() + n);
  // the detector's range word of THIS batch, before any of its boxes is used: a saturated heat map fails this batch and no other
  if (range_flag_ptr() && B.det_groups == groups) { spin_event(group_ev[groups]); range_verify(kRangeDet0 + (B.slot & 1), "the detector of a batch of pages"); }
  if (tn.detector_only) for (auto& d : dets) d.clear();   // profiling (tools/prof_pages.py): the detector and CCL run, nothing goes to the recogniser
  if (tn.bench_grid_boxes) {   // benchmark workload control (tuning key "bench_grid_boxes", tuatara_hip_debug.h): the detector's work is done (and timed); 40 fixed boxes per page go on
    for (int i = 0; i < n; ++i) {
      dets[i].clear();
      for (int r = 0; r < 8; ++r)
        for (int c = 0; c < 5; ++c) {
          RRect g;
          g.cx = (c + 0.5f) * (float)B.W2 / 5.f; g.cy = (r + 0.5f) * (float)B.H2 / 8.f; g.w = 75.f * B.pages[i].g.ratio; g.h = 20.f * B.pages[i].g.ratio; g.angle = 0.f;
          dets[i].push_back(g);
        }
    }
  }
  for (int i = 0; i < n; ++i) {
    const Page& P = B.pages[i];
    const float ratio_w = 1.f / P.g.ratio, ratio_h = 1.f / P.g.ratio;   // tuatara.cpp:360-361
    for (const RRect& r : dets[i]) {
      RRect b = adjust_coordinates(r, ratio_w, ratio_h);            // :406
      int xywh[4];
      bounding_rect(b, xywh);                                       // :416
      int x0 = xywh[0], y0 = xywh[1], x1 = xywh[0] + xywh[2], y1 = xywh[1] + xywh[3];
      if (cfg.strict_crops) {
        if (x0 < 0 || y0 < 0 || x1 > P.w || y1 > P.h) throw std::runtime_error("text box leaves the image (cv::Exception in the reference, tuatara.cpp:416)");
      } else {
        x0 = std::max(x0, 0); y0 = std::max(y0, 0); x1 = std::min(x1, P.w); y1 = std::min(y1, P.h);
      }
      if (x1 <= x0 || y1 <= y0) continue;
      B.boxes[i].push_back(b);
      B.rects.insert(B.rects.end(), {x0, y0, x1, y1, i});
      B.page_of.push_back(i);
      if (B.tab_min_len || B.mark_min || B.bc_min) {   // tables, selection marks, barcodes: 64 x the centre of the quad the result will carry (DESIGN.md "Tables", step 8)
        tq.clear();
        push_quad(b, tq);
        if (!region_quad_ok(tq.data())) throw std::runtime_error(std::string(B.tab_min_len ? "tables" : B.mark_min ? "marks" : "barcodes") + ": a corner of a word of page " + std::to_string(i) + " is not finite or lies beyond 32768 px");
        int32_t c[2];
        tables_word_centre(tq.data(), c);
        B.tab_centres.insert(B.tab_centres.end(), c, c + 2);
      }
      Pt2f q[4];
      if (cfg.crop_mode == TTR_CROP_RECTIFIED) {                    // DESIGN.md "Rectified crops": same items, other pixels
        double cf[6]; int64_t fx[6];
        const int kind = deskew_quad(b, q, cf);
        deskew_fixed(cf, fx);
        B.coef.insert(B.coef.end(), {(int64_t)kind, fx[0], fx[1], fx[2], fx[3], fx[4], fx[5], 0});
        if (wide != 0.f || curved) for (int k = 0; k < 4; ++k) { wq.push_back(q[k].x); wq.push_back(q[k].y); }
      } else if (K > 1) {
        box_edge_quad(x0, y0, x1, y1, q);
      }
      if (K > 1) oq.insert(oq.end(), q, q + 4);
    }
  }
  B.N = (int)B.page_of.size();
  plan_wide(B, wq.data());
  plan_curved(B, wq.data());
  for (int j = 1; j < K; ++j) {                                 // the twins, candidate-major in ascending turn
    const int t = K == 2 ? 2 * j : j;
    for (int c = 0; c < B.N; ++c) {
      int64_t fx[6];
      turn_coef(&oq[4 * (size_t)c], t, fx);
      B.twin.insert(B.twin.end(), {(int64_t)1, fx[0], fx[1], fx[2], fx[3], fx[4], fx[5], 0});
    }
  }
}

void Engine::plan_wide(PageBatch& B, const float* quads) {
  B.wide_aspect = wide; B.X = 0; B.wide.clear(); B.wide_of.clear();
  if (wide == 0.f) return;
  const int N = B.N;
  if (B.coef.size() != (size_t)N * 8 || B.rects.size() != (size_t)N * 5) throw std::runtime_error("wide words: coefficient count does not match the crop count");
  B.wide_of.assign((size_t)N, -1);
  for (int c = 0; c < N; ++c) {
    WideWord W{};
    const int n = wide_plan(quads + 8 * (size_t)c, wide, W.f);
    if (n < 2) continue;                                       // keeps its crop of today in every bit
    W.n = n; W.page = B.page_of[(size_t)c]; W.row = c; W.extra = N + B.X;
    B.wide_of[(size_t)c] = (int32_t)B.wide.size();
    B.wide.push_back(W);
    B.X += n - 1;
    B.coef[8 * (size_t)c] = 1;                                 // its first piece: the kind-1 sampler (wide_cut_kernel writes the row)
  }
  // the extra rows: each piece under its item's rectangle (kind 1 reads the coefficients alone) and mask
  const bool masks = !B.row_masks.empty();
  for (const WideWord& W : B.wide)
    for (int j = 1; j < W.n; ++j) {
      int rc[5];
      memcpy(rc, &B.rects[5 * (size_t)W.row], sizeof rc);
      B.rects.insert(B.rects.end(), rc, rc + 5);
      B.coef.insert(B.coef.end(), {(int64_t)1, 0, 0, 0, 0, 0, 0, 0});
      if (masks) { uint32_t m[4]; memcpy(m, &B.row_masks[4 * (size_t)W.row], sizeof m); B.row_masks.insert(B.row_masks.end(), m, m + 4); }
    }
}

void Engine::plan_curved(PageBatch& B, const float* quads) {
  B.curved = curved; B.curve.clear();
  if (!curved) return;
  const int N = B.N;
  if (B.coef.size() != (size_t)N * 8 || B.rects.size() != (size_t)N * 5) throw std::runtime_error("curved words: coefficient count does not match the crop count");
  B.curve.resize((size_t)N);
  for (int c = 0; c < N; ++c) {
    if (!region_quad_ok(quads + 8 * (size_t)c)) throw std::runtime_error("curved words: a corner of word " + std::to_string(c) + " is not finite or lies beyond 32768 px");
    CurveIn W{};
    curve_frame(quads + 8 * (size_t)c, W.f);
    W.page = B.page_of[(size_t)c]; W.row = c;
    B.curve[(size_t)c] = W;
  }
}

void Engine::pack_batch_crops(const PageBatch& B, int sl) {
  const int rows = B.N + B.X;                                  // wide words: X more rows behind the batch's N
  // (tables, selection marks: every word's centre [N][2] and the pages' offsets [n + 1] travel behind the rectangles, in the same copy)
  const size_t rect_ints = B.rects.size(), tab_ints = B.tab_min_len || B.mark_min || B.bc_min ? B.tab_centres.size() + (size_t)B.n + 1 : 0;
  rects_dev.ensure((rect_ints + tab_ints) * 4);
  h_rects[sl].ensure((rect_ints + tab_ints) * 4);
  memcpy(h_rects[sl].p, B.rects.data(), rect_ints * 4);
  if (tab_ints) {
    if (B.tab_centres.size() != (size_t)B.N * 2) throw std::runtime_error(std::string(B.tab_min_len ? "tables" : B.mark_min ? "marks" : "barcodes") + ": centre count does not match the crop count");
    int32_t* t = h_rects[sl].as<int32_t>() + rect_ints;
    std::copy(B.tab_centres.begin(), B.tab_centres.end(), t);
    const std::vector<int> first = page_first(B.page_of, B.n);
    std::copy(first.begin(), first.end(), t + B.tab_centres.size());
  }
  TTR_HIP_CHECK(hipMemcpyAsync(rects_dev.p, h_rects[sl].p, (rect_ints + tab_ints) * 4, hipMemcpyHostToDevice, stream));
  // (a uniform batch: its pages are page_bytes apart behind the first; a mixed one: each crop's page from the slot's table)
  const Page& P0 = B.pages[0];
  const size_t page_bytes = (size_t)P0.h * P0.w * 3;
  const PageRow* table = B.mixed ? page_table[sl & 1].as<PageRow>() : nullptr;
  if (cfg.crop_mode != TTR_CROP_RECTIFIED && !B.regions) {   // (a region is a kind-1 crop whatever the mode)
    if (B.mixed) { launch_pack_crops_pages(table, rects_dev.as<int>(), crops.as<uint8_t>(), B.N, stream); TTR_HIP_CHECK(hipEventRecord(table_ev[sl & 1], stream)); }
    else launch_pack_crops(P0.data, page_bytes, P0.stride, rects_dev.as<int>(), crops.as<uint8_t>(), B.N, stream);
    return;
  }
  if (B.coef.size() != (size_t)rows * 8 || B.rects.size() != (size_t)rows * 5) throw std::runtime_error("rectified crops: coefficient count does not match the crop count");
  // wide words: the table of the batch's wide words travels behind the coefficients, in the same copy
  // (curved words: the batch's CurveIn entries likewise, behind those)
  const size_t coef_b = B.coef.size() * 8, words_b = B.wide.size() * sizeof(WideWord), curve_b = B.curve.size() * sizeof(CurveIn);
  coef_dev.ensure(coef_b + words_b + curve_b);
  h_coef[sl].ensure(coef_b + words_b + curve_b);
  memcpy(h_coef[sl].p, B.coef.data(), coef_b);
  if (words_b) memcpy(h_coef[sl].as<uint8_t>() + coef_b, B.wide.data(), words_b);
  if (curve_b) memcpy(h_coef[sl].as<uint8_t>() + coef_b + words_b, B.curve.data(), curve_b);
  TTR_HIP_CHECK(hipMemcpyAsync(coef_dev.p, h_coef[sl].p, coef_b + words_b + curve_b, hipMemcpyHostToDevice, stream));
  if (words_b) {   // the cuts, and every piece's packer row straight into coef_dev (wide.hip)
    const int Wn = (int)B.wide.size();
    wide_side.ensure(wide_side_bytes(Wn));
    launch_wide_cut(reinterpret_cast<const WideWord*>(coef_dev.as<uint8_t>() + coef_b), Wn, P0.data, page_bytes, P0.stride, P0.h, P0.w, table, coef_dev.as<int64_t>(), rows,
                    wide_side.as<int>(), stream);
  }
  if (B.mixed) { launch_pack_crops_rect_pages(table, rects_dev.as<int>(), coef_dev.as<int64_t>(), crops.as<uint8_t>(), rows, stream); TTR_HIP_CHECK(hipEventRecord(table_ev[sl & 1], stream)); }
  else launch_pack_crops_rect(P0.data, page_bytes, P0.stride, P0.h, P0.w, rects_dev.as<int>(), coef_dev.as<int64_t>(), crops.as<uint8_t>(), rows, stream);
  if (curve_b) {   // curved words: behind the unchanged packer, the rows of the curved ones are made again along their spines (curve.hip)
    const int Cn = (int)B.curve.size();
    curve_side.ensure(curve_side_bytes(Cn));
    launch_curve_crop(reinterpret_cast<const CurveIn*>(coef_dev.as<uint8_t>() + coef_b + words_b), Cn, P0.data, page_bytes, P0.stride, P0.h, P0.w, table, crops.as<uint8_t>(), rows,
                      curve_side.as<int>(), stream);
    if (B.mixed) TTR_HIP_CHECK(hipEventRecord(table_ev[sl & 1], stream));   // (the table's last reader of this batch is now this kernel)
  }
}

void Engine::pack_twin_crops(const PageBatch& B, int sl) {
  const int N = B.N, T = (int)(B.twin.size() / 8);
  if (T != (orient_k() - 1) * N) throw std::runtime_error("word orientation: twin count does not match the crop count");
  // orient_in: coef int64 [T][8] | rects int32 [T][5] (row (j - 1) N + c = the word's rects row) | first int32 [pages + 1]
  const size_t coef_b = (size_t)T * 64, rect_b = (size_t)T * 20, first_b = (size_t)(B.n + 1) * 4;
  h_orient_in[sl].ensure(coef_b + rect_b + first_b);
  orient_in.ensure(coef_b + rect_b + first_b);
  uint8_t* h = h_orient_in[sl].as<uint8_t>();
  memcpy(h, B.twin.data(), coef_b);
  for (int r = 0; r < T; ++r) memcpy(h + coef_b + (size_t)r * 20, &B.rects[(size_t)(r % N) * 5], 20);
  const std::vector<int> first = page_first(B.page_of, B.n);
  std::copy(first.begin(), first.end(), reinterpret_cast<int32_t*>(h + coef_b + rect_b));
  TTR_HIP_CHECK(hipMemcpyAsync(orient_in.p, h, coef_b + rect_b + first_b, hipMemcpyHostToDevice, stream));
  const Page& P0 = B.pages[0];
  if (B.mixed) {
    launch_pack_crops_rect_pages(page_table[sl & 1].as<PageRow>(), reinterpret_cast<const int*>(orient_in.as<uint8_t>() + coef_b), orient_in.as<int64_t>(),
                                 crops.as<uint8_t>() + (size_t)N * kCropBytes, T, stream);
    TTR_HIP_CHECK(hipEventRecord(table_ev[sl & 1], stream));   // (the batch's last reader of the slot's table)
  } else {
    launch_pack_crops_rect(P0.data, (size_t)P0.h * P0.w * 3, P0.stride, P0.h, P0.w, reinterpret_cast<const int*>(orient_in.as<uint8_t>() + coef_b), orient_in.as<int64_t>(),
                           crops.as<uint8_t>() + (size_t)N * kCropBytes, T, stream);
  }
}

int Engine::stage_batch_lines(const PageBatch& B, int sl) {
  const int N = B.N;
  h_lines_in[sl].ensure((size_t)N * 24 + (size_t)(B.n + 1) * 4);   // cuv int32 [N][6] | first int32 [pages + 1]
  int32_t* cuv = h_lines_in[sl].as<int32_t>();
  std::vector<float> q;
  q.reserve(8);
  int c = 0;
  for (int pg = 0; pg < B.n; ++pg)
    for (const RRect& b : B.boxes[pg]) {                       // (crop order: page after page)
      q.clear();
      push_quad(b, q);
      if (c >= N || !lines_cuv(q.data(), cuv + 6 * (size_t)c)) throw std::runtime_error("text lines: a word's corner is not finite or lies beyond 32768 px");
      ++c;
    }
  if (c != N) throw std::runtime_error("text lines: box count does not match the crop count");
  const std::vector<int> first = page_first(B.page_of, B.n);
  std::copy(first.begin(), first.end(), cuv + 6 * (size_t)N);
  int max_words = 0;
  for (int pg = 0; pg < B.n; ++pg) max_words = std::max(max_words, first[pg + 1] - first[pg]);
  if (max_words > kLinesMaxWords) throw std::runtime_error("text lines: a page has more than " + std::to_string(kLinesMaxWords) + " words");
  return max_words;
}

void Engine::group_batch_lines(const PageBatch& B, int sl, int max_words) {
  const int N = B.N;
  const size_t in_b = (size_t)N * 24 + (size_t)(B.n + 1) * 4, side_b = lines_side_bytes(N, B.n);
  lines_in.ensure(in_b);
  h_lines.arm(sl, side_b); lines_side.ensure(side_b);
  TTR_HIP_CHECK(hipMemcpyAsync(lines_in.p, h_lines_in[sl].p, in_b, hipMemcpyHostToDevice, stream));
  launch_line_group(lines_in.as<int>(), lines_in.as<int>() + 6 * (size_t)N, B.n, N, max_words, lines_side.as<int>(), stream);
  h_lines.fetch(sl, lines_side, stream);
}

void Engine::group_lines(const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines) {
  group_blocks(quads, first, pages, line, word, n_lines, nullptr, nullptr, nullptr, nullptr, false);
}

static size_t blocks_side_bytes(int N, int pages) { return ((size_t)2 * N + (size_t)2 * pages) * 4; }   // [N] block | [N] pos | [pages] n_blocks | [pages] mode

void Engine::group_batch_blocks(const PageBatch& B, int sl, int max_words) {
  const int N = B.N;
  const size_t side_b = blocks_side_bytes(N, B.n);
  blocks_side.ensure(side_b); h_blocks.arm(sl, side_b);
  launch_block_group(lines_in.as<int>(), lines_in.as<int>() + 6 * (size_t)N, lines_side.as<int>(), B.n, N, max_words, blocks_side.as<int>(), stream);
  h_blocks.fetch(sl, blocks_side, stream);
}

void Engine::group_blocks(const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block, int32_t* pos,
                          int32_t* n_blocks, int32_t* mode, bool blocks) {
  if (pages <= 0) return;
  const std::string what = blocks ? "ttr_group_blocks" : "ttr_group_lines";
  if (first[0] != 0) throw std::runtime_error(what + ": first[0] must be 0");
  int max_words = 0;
  for (int pg = 0; pg < pages; ++pg) {
    if (first[pg + 1] < first[pg]) throw std::runtime_error(what + ": first must not decrease");
    max_words = std::max(max_words, first[pg + 1] - first[pg]);
  }
  if (max_words > kLinesMaxWords) throw std::runtime_error(what + ": more than " + std::to_string(kLinesMaxWords) + " words on a page");
  const int N = first[pages];
  const size_t in_b = (size_t)N * 24 + (size_t)(pages + 1) * 4, lside_b = lines_side_bytes(N, pages), side_b = blocks_side_bytes(N, pages);
  h_lines_in[0].ensure(in_b); lines_in.ensure(in_b);
  h_lines.arm(0, lside_b); lines_side.ensure(lside_b);
  if (blocks) { h_blocks.arm(0, side_b); blocks_side.ensure(side_b); }
  int32_t* cuv = h_lines_in[0].as<int32_t>();
  for (int c = 0; c < N; ++c)
    if (!lines_cuv(quads + 8 * (size_t)c, cuv + 6 * (size_t)c)) throw std::runtime_error(what + ": a coordinate is not finite or has |x| >= 32768");
  std::copy(first, first + pages + 1, cuv + 6 * (size_t)N);
  TTR_HIP_CHECK(hipMemcpyAsync(lines_in.p, cuv, in_b, hipMemcpyHostToDevice, stream));
  launch_line_group(lines_in.as<int>(), lines_in.as<int>() + 6 * (size_t)N, pages, N, max_words, lines_side.as<int>(), stream);
  if (blocks) launch_block_group(lines_in.as<int>(), lines_in.as<int>() + 6 * (size_t)N, lines_side.as<int>(), pages, N, max_words, blocks_side.as<int>(), stream);
  h_lines.fetch(0, lines_side, stream);
  if (blocks) h_blocks.fetch(0, blocks_side, stream);
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  const int32_t *ls = h_lines.view<int32_t>(0), *bs = blocks ? h_blocks.view<int32_t>(0) : nullptr;
  if (line && N) std::copy(ls, ls + N, line);
  if (word && N) std::copy(ls + N, ls + 2 * (size_t)N, word);
  if (n_lines) std::copy(ls + 2 * (size_t)N, ls + 2 * (size_t)N + pages, n_lines);
  if (block && N) std::copy(bs, bs + N, block);
  if (pos && N) std::copy(bs + N, bs + 2 * (size_t)N, pos);
  if (n_blocks) std::copy(bs + 2 * (size_t)N, bs + 2 * (size_t)N + pages, n_blocks);
  if (mode) std::copy(bs + 2 * (size_t)N + pages, bs + 2 * (size_t)N + 2 * (size_t)pages, mode);
}

void Engine::keep_batch_map(const PageBatch& B) {
  const int sl = B.slot & 1;
  for (auto& x : chars_ev[sl]) if (!x) TTR_HIP_CHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
  const size_t bytes = (size_t)B.n * B.H2 * B.W2 * 4;
  chars_map[sl].ensure(bytes);
  TTR_HIP_CHECK(hipStreamWaitEvent(stream, chars_ev[sl][1], 0));   // the slot's previous batch may still be cut on the recogniser's stream (no-op before the first)
  TTR_HIP_CHECK(hipMemcpyAsync(chars_map[sl].p, ccl.tnorm.p, bytes, hipMemcpyDeviceToDevice, stream));
  TTR_HIP_CHECK(hipEventRecord(chars_ev[sl][0], stream));
}

static size_t chars_in_bytes(int N, int KT) { return (size_t)N * KT * 48 + (size_t)N * 4; }   // coef int64 [N][KT][6] | page_of int32 [N]

void Engine::stage_batch_chars(const PageBatch& B, int sl) {
  const int N = B.N, KT = orient_k() > 1 ? 4 : 1;
  h_chars_in[sl].ensure(chars_in_bytes(N, KT));
  int64_t* coef = h_chars_in[sl].as<int64_t>();
  int32_t* page_of = reinterpret_cast<int32_t*>(coef + (size_t)N * KT * 6);
  std::vector<float> q;
  q.reserve(8);
  int c = 0;
  for (int pg = 0; pg < B.n; ++pg) {
    const double k = chars_scale(B.pages[pg].g.ratio);         // (the ratio of the word's page)
    for (const RRect& b : B.boxes[pg]) {                       // (crop order: page after page)
      q.clear();
      push_quad(b, q);
      if (c >= N) throw std::runtime_error("character boxes: box count does not match the crop count");
      for (int t = 0; t < KT; ++t)
        if (!chars_coef(q.data(), t, k, coef + ((size_t)c * KT + t) * 6)) throw std::runtime_error("character boxes: a word's corner is not finite or lies beyond 32768 px");
      page_of[c] = pg;
      ++c;
    }
  }
  if (c != N) throw std::runtime_error("character boxes: box count does not match the crop count");
}

void Engine::cut_batch_chars(const PageBatch& B, int sl, const int* ids, const int* turns) {
  const int N = B.N, KT = orient_k() > 1 ? 4 : 1;
  if (!chars_ev[sl & 1][0] || chars_map[sl & 1].cap < (size_t)B.n * B.H2 * B.W2 * 4) throw std::runtime_error("character boxes: the batch's region planes were not kept");
  const size_t in_b = chars_in_bytes(N, KT), side_b = char_side_bytes(N);
  chars_in.ensure(in_b); chars_side.ensure(side_b); h_chars.arm(sl, side_b);
  TTR_HIP_CHECK(hipMemcpyAsync(chars_in.p, h_chars_in[sl].p, in_b, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipStreamWaitEvent(stream, chars_ev[sl & 1][0], 0));
  launch_char_cut(chars_map[sl & 1].as<float>(), B.H2, B.W2, chars_in.as<int64_t>(), KT, reinterpret_cast<const int*>(chars_in.as<int64_t>() + (size_t)N * KT * 6), turns, ids,
                  nullptr, (int)(cfg.low_text * 255.f), N, chars_side.as<int>(), stream);
  TTR_HIP_CHECK(hipEventRecord(chars_ev[sl & 1][1], stream));
  h_chars.fetch(sl, chars_side, stream);
}

void Engine::char_cuts(const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars, int n,
                       int32_t* cuts, int32_t* modes, uint8_t* profiles) {
  if (n <= 0) return;
  if (H2 <= 0 || W2 <= 0 || (size_t)H2 * W2 > ((size_t)1 << 28)) throw std::runtime_error("ttr_char_cuts: bad map size");
  const double k = chars_scale(ratio);
  // chars_in: coef int64 [n][4][6] | page_of int32 [n] (all 0) | turns int32 [n] | nchars int32 [n]
  const size_t coef_b = (size_t)n * 192, in_b = coef_b + (size_t)n * 12, side_b = char_side_bytes(n), map_b = (size_t)H2 * W2 * 4;
  h_chars_in[0].ensure(in_b); chars_in.ensure(in_b); chars_side.ensure(side_b); h_chars.arm(0, side_b); chars_map[0].ensure(map_b);
  int64_t* coef = h_chars_in[0].as<int64_t>();
  int32_t* tail = reinterpret_cast<int32_t*>(coef + (size_t)n * 24);
  for (int c = 0; c < n; ++c) {
    for (int t = 0; t < 4; ++t)
      if (!chars_coef(quads + 8 * (size_t)c, t, k, coef + ((size_t)c * 4 + t) * 6)) throw std::runtime_error("ttr_char_cuts: a coordinate is not finite or has |x| >= 32768, or the ratio is out of range");
    if (turns[c] < 0 || turns[c] > 3) throw std::runtime_error("ttr_char_cuts: a turn outside 0..3");
    if (nchars[c] < 0 || nchars[c] > kCharsMax) throw std::runtime_error("ttr_char_cuts: a character count outside 0..26");
    tail[c] = 0; tail[(size_t)n + c] = turns[c]; tail[2 * (size_t)n + c] = nchars[c];
  }
  TTR_HIP_CHECK(hipMemcpyAsync(chars_map[0].p, tnorm, map_b, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipMemcpyAsync(chars_in.p, coef, in_b, hipMemcpyHostToDevice, stream));
  const int* d_tail = reinterpret_cast<const int*>(chars_in.as<int64_t>() + (size_t)n * 24);
  launch_char_cut(chars_map[0].as<float>(), H2, W2, chars_in.as<int64_t>(), 4, d_tail, d_tail + n, nullptr, d_tail + 2 * (size_t)n, (int)(low_text * 255.f), n, chars_side.as<int>(), stream);
  h_chars.fetch(0, chars_side, stream);
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  const int32_t* side = h_chars.view<int32_t>(0);
  if (cuts) std::copy(side, side + (size_t)n * 27, cuts);
  if (modes) std::copy(side + (size_t)n * 27, side + (size_t)n * 28, modes);
  if (profiles) memcpy(profiles, side + (size_t)n * 28, (size_t)n * 128);
}

void Engine::wide_cuts(const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, float max_aspect, bool use_table, int32_t* n_out, int32_t* cuts,
                       uint16_t* profiles, int64_t* coef) {
  if (nq <= 0) return;
  if (!wide_aspect_ok(max_aspect) || max_aspect == 0.f) throw std::runtime_error("ttr_wide_cuts: max_aspect must be a finite value in [2, 64]");
  if ((size_t)h * w > ((size_t)1 << 28)) throw std::runtime_error("ttr_wide_cuts: bad image size");
  // coef_dev: coef int64 [nq][16][8] | words [nq]: word i owns rows 16 i .. 16 i + 15 (its row, then its extra rows)
  const int rows = nq * kWideMaxPieces;
  const size_t coef_b = (size_t)rows * 64, words_b = (size_t)nq * sizeof(WideWord), side_b = wide_side_bytes(nq);
  h_coef[0].ensure(coef_b + words_b); coef_dev.ensure(coef_b + words_b); wide_side.ensure(side_b);
  std::vector<uint8_t> side(side_b);
  memset(h_coef[0].p, 0, coef_b);
  WideWord* words = reinterpret_cast<WideWord*>(h_coef[0].as<uint8_t>() + coef_b);
  for (int i = 0; i < nq; ++i) {
    if (!region_quad_ok(quads + 8 * (size_t)i)) throw std::runtime_error("ttr_wide_cuts: quad " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
    WideWord W{};
    W.n = wide_plan(quads + 8 * (size_t)i, max_aspect, W.f);
    W.page = 0; W.row = i * kWideMaxPieces; W.extra = W.row + 1;
    words[i] = W;
    if (n_out) n_out[i] = W.n;
  }
  const StagedPage pg = stage_page("ttr_wide_cuts", img, h, w, row_stride);
  TTR_HIP_CHECK(hipMemcpyAsync(coef_dev.p, h_coef[0].p, coef_b + words_b, hipMemcpyHostToDevice, stream));
  const PageRow* table = use_table ? staged_page_table(pg, h, w) : nullptr;
  launch_wide_cut(reinterpret_cast<const WideWord*>(coef_dev.as<uint8_t>() + coef_b), nq, pg.data, 0, pg.stride, h, w, table, coef_dev.as<int64_t>(), rows,
                  wide_side.as<int>(), stream);
  if (use_table) TTR_HIP_CHECK(hipEventRecord(table_ev[0], stream));
  TTR_HIP_CHECK(hipMemcpyAsync(side.data(), wide_side.p, side_b, hipMemcpyDeviceToHost, stream));
  if (coef) TTR_HIP_CHECK(hipMemcpyAsync(coef, coef_dev.p, coef_b, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  if (cuts) memcpy(cuts, side.data(), wide_cuts_bytes(nq));
  if (profiles) memcpy(profiles, side.data() + wide_cuts_bytes(nq), (size_t)nq * 2048 * 2);
}

void Engine::curve_crops(const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, bool use_table, int32_t* flag, int32_t* hb, int32_t* spine,
                         int64_t* knots, uint8_t* crops_out) {
  if (nq <= 0) return;
  if ((size_t)h * w > ((size_t)1 << 28)) throw std::runtime_error("ttr_curve_crops: bad image size");
  // coef_dev: coef int64 [nq][8] | words [nq]; rects_dev: [nq][5] (kind 1 reads the coefficients alone; the rectangle only has to be non-empty)
  const size_t coef_b = (size_t)nq * 64, words_b = (size_t)nq * sizeof(CurveIn), side_b = curve_side_bytes(nq), crop_b = (size_t)nq * kCropBytes;
  h_coef[0].ensure(coef_b + words_b); coef_dev.ensure(coef_b + words_b); h_rects[0].ensure((size_t)nq * 20); rects_dev.ensure((size_t)nq * 20);
  curve_side.ensure(side_b); crops.ensure(crop_b);
  std::vector<uint8_t> side(side_b);
  int64_t* coef = h_coef[0].as<int64_t>();
  CurveIn* words = reinterpret_cast<CurveIn*>(h_coef[0].as<uint8_t>() + coef_b);
  int* rects = h_rects[0].as<int>();
  for (int i = 0; i < nq; ++i) {
    const float* q = quads + 8 * (size_t)i;
    if (!region_quad_ok(q)) throw std::runtime_error("ttr_curve_crops: quad " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
    int64_t fx[6];
    region_coef(q, fx);
    coef[8 * (size_t)i] = 1; coef[8 * (size_t)i + 7] = 0;
    for (int k = 0; k < 6; ++k) coef[8 * (size_t)i + 1 + k] = fx[k];
    CurveIn W{};
    curve_frame(q, W.f);
    W.page = 0; W.row = i;
    words[i] = W;
    const int rc[5] = {0, 0, 1, 1, 0};
    memcpy(rects + 5 * (size_t)i, rc, sizeof rc);
  }
  const StagedPage pg = stage_page("ttr_curve_crops", img, h, w, row_stride);
  TTR_HIP_CHECK(hipMemcpyAsync(coef_dev.p, h_coef[0].p, coef_b + words_b, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipMemcpyAsync(rects_dev.p, h_rects[0].p, (size_t)nq * 20, hipMemcpyHostToDevice, stream));
  const PageRow* table = use_table ? staged_page_table(pg, h, w) : nullptr;
  if (table) launch_pack_crops_rect_pages(table, rects_dev.as<int>(), coef_dev.as<int64_t>(), crops.as<uint8_t>(), nq, stream);
  else launch_pack_crops_rect(pg.data, 0, pg.stride, h, w, rects_dev.as<int>(), coef_dev.as<int64_t>(), crops.as<uint8_t>(), nq, stream);
  launch_curve_crop(reinterpret_cast<const CurveIn*>(coef_dev.as<uint8_t>() + coef_b), nq, pg.data, 0, pg.stride, h, w, table, crops.as<uint8_t>(), nq,
                    curve_side.as<int>(), stream);
  if (use_table) TTR_HIP_CHECK(hipEventRecord(table_ev[0], stream));
  TTR_HIP_CHECK(hipMemcpyAsync(side.data(), curve_side.p, side_b, hipMemcpyDeviceToHost, stream));
  if (crops_out) TTR_HIP_CHECK(hipMemcpyAsync(crops_out, crops.p, crop_b, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  if (flag) memcpy(flag, side.data(), (size_t)nq * 4);
  if (hb) memcpy(hb, side.data() + (size_t)nq * 4, (size_t)nq * 8);
  if (spine) memcpy(spine, side.data() + (size_t)nq * 12, (size_t)nq * 72);
  if (knots) memcpy(knots, side.data() + curve_side_table_offset(nq), (size_t)nq * 288);
}

Engine::LayerBatch Engine::layer_batch(const PageBatch& B, int sl) {
  const auto [Hcap, Wcap] = B.extent();
  // (detect_enqueue refused a page side of 32768 or more before anything of the batch was enqueued)
  if (B.N == 0 && !batch_offsets_up) {   // a batch without words has no packer and so no upload: the pages' offsets [n + 1], all 0, go up with the first layer that asks
    const size_t bytes = ((size_t)B.n + 1) * 4;
    rects_dev.ensure(bytes); h_rects[sl].ensure(bytes);
    std::fill(h_rects[sl].as<int32_t>(), h_rects[sl].as<int32_t>() + B.n + 1, 0);
    TTR_HIP_CHECK(hipMemcpyAsync(rects_dev.p, h_rects[sl].p, bytes, hipMemcpyHostToDevice, stream));
    batch_offsets_up = true;
  }
  const int* centres = rects_dev.as<int>() + (B.N ? B.rects.size() : 0);
  return LayerBatch{B.n, B.N, Hcap, Wcap, B.pages[0], B.mixed ? page_table[sl & 1].as<PageRow>() : nullptr, centres, centres + (size_t)B.N * 2};
}

void Engine::layer_batch_done(const LayerBatch& L, int sl) {
  if (L.table) TTR_HIP_CHECK(hipEventRecord(table_ev[sl & 1], stream));   // (the table's last reader of this batch is now the layer's last kernel)
}

void Engine::page_ink_enqueue(const PageBatch& B, int sl, int ink) {
  const int want = B.ink_radius ? kBitsLocal : ink;
  if (batch_bits == want) return;   // the bitmaps in place are this rule's already: whichever layer formed them
  batch_bits = want;
  const int n = B.n;
  ++page_ink_passes;
  const auto [Hcap, Wcap] = B.extent();
  tab_bits.ensure(tables_bits_slot(Hcap, Wcap) * 8 * n); tab_bitsT.ensure(tables_bitsT_slot(Hcap, Wcap) * 8 * n);
  const Page& P0 = B.pages[0];
  const PageRow* table = B.mixed ? page_table[sl & 1].as<PageRow>() : nullptr;
  if (B.ink_radius) {   // local ink (DESIGN.md "Local ink"): the same bitmaps under the adaptive rule, and the pages' records beside the side blocks
    tab_ink_h.ensure(ink_ws_bytes(Hcap, Wcap, n)); tab_ink_rec.ensure(ink_recs_bytes(n)); h_tab_ink.arm(sl, ink_recs_bytes(n));
    launch_ink_local(P0.data, (size_t)P0.h * P0.w * 3, P0.stride, P0.h, P0.w, table, n, Hcap, Wcap, B.ink_radius, B.ink_drop, B.ink_polarity, tab_ink_h.as<uint32_t>(),
                     tab_ink_rec.as<InkRec>(), tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), stream);
  } else
  launch_table_ink(P0.data, (size_t)P0.h * P0.w * 3, P0.stride, P0.h, P0.w, table, n, Hcap, Wcap, ink, tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), stream);
}

Engine::StagedPage Engine::stage_ink_page(const char* what, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, const char* bad_args, int ink,
                                          const float* quads, int nq, DevBuf* zero, size_t zero_b) {
  // (the image check is stage_page's: both routes here - the ttr_*_page call and the developer hook - have made it under their own names before.  The page's copy
  // is enqueued before stage_centres looks at the quads; no quad can fail there: the ttr_*_page call has checked them and the hook passes none)
  const StagedPage pg = stage_page(what, img, h, w, row_stride, dev_offset, dev_stride, 32768, bad_args);
  stage_centres(what, quads, nq);
  tab_bits.ensure(tables_bits_slot(h, w) * 8); tab_bitsT.ensure(tables_bitsT_slot(h, w) * 8);
  if (zero) { zero->ensure(zero_b); TTR_HIP_CHECK(hipMemsetAsync(zero->p, 0, zero_b, stream)); }   // (a hook that returns whole lists)
  launch_table_ink(pg.data, 0, pg.stride, h, w, nullptr, 1, h, w, ink, tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), stream);
  return pg;
}

void Engine::stage_side_home(const char* what_, const StageSide& s, int nq, std::initializer_list<StageBack> extra, const std::function<bool(const int32_t*, std::string*)>& valid,
                             int32_t* side_out, int32_t* items_out) {
  const std::string what(what_);
  std::vector<int32_t> side((size_t)s.ints + (size_t)nq * s.item_ints);
  TTR_HIP_CHECK(hipMemcpyAsync(side.data(), s.dev->p, side.size() * 4, hipMemcpyDeviceToHost, stream));
  for (const StageBack& e : extra)
    if (e.host) TTR_HIP_CHECK(hipMemcpyAsync(e.host, e.dev->p, e.bytes, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  std::string why;
  if (!valid(side.data(), &why)) throw std::runtime_error(what + ": the side block holds " + why);
  if (s.noun)
    for (size_t i = s.ints; i < side.size(); ++i)
      if (side[i] < -1 || side[i] >= side[1]) throw std::runtime_error(what + ": an item names a " + s.noun + " that does not exist");
  if (side_out) {   // (validated: the counted part is what callers read; the rest is zero as on the host)
    std::fill(side_out, side_out + s.ints, 0);
    std::copy(side.begin(), side.begin() + s.hdr + (size_t)s.rec * side[1], side_out);
  }
  if (items_out) std::copy(side.begin() + s.ints, side.end(), items_out);
}

void Engine::tables_enqueue(const PageBatch& B, int sl) {
  const LayerBatch L = layer_batch(B, sl);
  tab_runs.ensure((size_t)L.n * 2 * kTabRunCap * 3 * 4);
  const size_t side_b = tables_side_bytes(L.n, L.N);
  tab_side.ensure(side_b); h_tab.arm(sl, side_b);
  page_ink_enqueue(B, sl, B.tab_ink);
  launch_table_grid(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), L.P0.h, L.P0.w, L.table, L.n, L.Hcap, L.Wcap, B.tab_min_len, L.centres, L.first, tab_runs.as<int>(),
                    tab_side.as<int>(), tab_side.as<int>() + (size_t)L.n * kTabSideInts, stream);
  layer_batch_done(L, sl);
}

void Engine::tables_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_len, int ink, const float* quads, int nq,
                          int32_t* side_out, int32_t* items_out, uint64_t* bits_out, int32_t* runs_out) {
  const size_t runs_b = (size_t)2 * kTabRunCap * 3 * 4;
  stage_ink_page("ttr_tables_page", img, h, w, row_stride, dev_offset, dev_stride, tables_args_ok(min_len, ink) ? nullptr : "min_len must lie in 16..4096 and ink in 1..255", ink,
                 quads, nq, &tab_runs, runs_b);
  tab_side.ensure(tables_side_bytes(1, nq));
  launch_table_grid(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), h, w, nullptr, 1, h, w, min_len, rects_dev.as<int>(), rects_dev.as<int>() + (size_t)nq * 2, tab_runs.as<int>(),
                    tab_side.as<int>(), tab_side.as<int>() + kTabSideInts, stream);
  // (tables hand out the whole block, not the counted part: hdr = kTabSideInts, no records behind it)
  stage_side_home("ttr_tables_page", StageSide{&tab_side, kTabSideInts, kTabSideInts, 0, 2, nullptr}, nq, {{bits_out, &tab_bits, tables_bits_slot(h, w) * 8}, {runs_out, &tab_runs, runs_b}},
                  [&](const int32_t* side, std::string* why) { return tables_side_valid(side, why); }, side_out, items_out);
}

void Engine::marks_enqueue(const PageBatch& B, int sl) {
  const LayerBatch L = layer_batch(B, sl);
  mark_cand.ensure(marks_cand_ints(L.Hcap, L.n) * 4); mark_counts.ensure(marks_count_ints(L.Hcap, L.n) * 4);
  const size_t side_b = marks_side_bytes(L.n, L.N);
  mark_side.ensure(side_b); h_mark.arm(sl, side_b);
  page_ink_enqueue(B, sl, B.mark_ink);
  launch_mark_cand(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), L.P0.h, L.P0.w, L.table, L.n, L.Hcap, L.Wcap, B.mark_min, B.mark_max, B.mark_fill, mark_cand.as<int>(),
                   mark_counts.as<int>(), stream);
  launch_mark_page(mark_cand.as<int>(), mark_counts.as<int>(), L.n, L.Hcap, L.centres, L.first, mark_side.as<int>(), mark_side.as<int>() + (size_t)L.n * kMarkSideInts, stream);
  layer_batch_done(L, sl);
}

void Engine::marks_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_side, int max_side, int fill, int ink, const float* quads,
                         int nq, int32_t* side_out, int32_t* item_mark_out, int32_t* counts_out) {
  stage_ink_page("ttr_marks_page", img, h, w, row_stride, dev_offset, dev_stride,
                 marks_args_ok(min_side, max_side, fill, ink) ? nullptr : "min_side must lie in 8..64, max_side in min_side..128, fill and ink in 1..255", ink, quads, nq);
  const size_t cnt_b = marks_count_ints(h, 1) * 4;
  mark_cand.ensure(marks_cand_ints(h, 1) * 4); mark_counts.ensure(cnt_b); mark_side.ensure(marks_side_bytes(1, nq));
  launch_mark_cand(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), h, w, nullptr, 1, h, w, min_side, max_side, fill, mark_cand.as<int>(), mark_counts.as<int>(), stream);
  launch_mark_page(mark_cand.as<int>(), mark_counts.as<int>(), 1, h, rects_dev.as<int>(), rects_dev.as<int>() + (size_t)nq * 2, mark_side.as<int>(),
                   mark_side.as<int>() + kMarkSideInts, stream);
  stage_side_home("ttr_marks_page", StageSide{&mark_side, kMarkSideInts, kMarkHdr, kMarkRec, 1, "mark"}, nq, {{counts_out, &mark_counts, cnt_b}},
                  [&](const int32_t* side, std::string* why) { return marks_side_valid(side, h, w, fill, nq, why); }, side_out, item_mark_out);
}

void Engine::barcodes_enqueue(const PageBatch& B, int sl) {
  const LayerBatch L = layer_batch(B, sl);
  bc_hits.ensure(barcodes_hit_ints(L.Hcap, L.Wcap, L.n) * 4); bc_cnt.ensure(barcodes_count_ints(L.Hcap, L.Wcap, L.n) * 4);
  const size_t side_b = barcodes_side_bytes(L.n, L.N);
  bc_side.ensure(side_b); h_barcode.arm(sl, side_b);
  page_ink_enqueue(B, sl, B.bc_ink);
  launch_barcode_scan(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), L.P0.h, L.P0.w, L.table, L.n, L.Hcap, L.Wcap, B.bc_sym, bc_hits.as<int>(), bc_cnt.as<int>(), stream);
  launch_barcode_page(bc_hits.as<int>(), bc_cnt.as<int>(), L.P0.h, L.P0.w, L.table, L.n, L.Hcap, L.Wcap, B.bc_min, L.centres, L.first, bc_side.as<int>(),
                      bc_side.as<int>() + (size_t)L.n * kBcSideInts, stream);
  layer_batch_done(L, sl);
}

void Engine::barcodes_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_lines, int ink, int symbologies, const float* quads,
                            int nq, int32_t* side_out, int32_t* item_out, int32_t* hits_out, int32_t* cnt_out) {
  const size_t hit_b = barcodes_hit_ints(h, w, 1) * 4, cnt_b = barcodes_count_ints(h, w, 1) * 4;
  stage_ink_page("ttr_barcodes_page", img, h, w, row_stride, dev_offset, dev_stride,
                 barcodes_args_ok(min_lines, ink, symbologies) ? nullptr : "min_lines must lie in 4..256, ink in 1..255 and symbologies in 1..3", ink, quads, nq,
                 hits_out ? &bc_hits : nullptr, hit_b);
  bc_hits.ensure(hit_b); bc_cnt.ensure(cnt_b); bc_side.ensure(barcodes_side_bytes(1, nq));
  launch_barcode_scan(tab_bits.as<uint64_t>(), tab_bitsT.as<uint64_t>(), h, w, nullptr, 1, h, w, symbologies, bc_hits.as<int>(), bc_cnt.as<int>(), stream);
  launch_barcode_page(bc_hits.as<int>(), bc_cnt.as<int>(), h, w, nullptr, 1, h, w, min_lines, rects_dev.as<int>(), rects_dev.as<int>() + (size_t)nq * 2, bc_side.as<int>(),
                      bc_side.as<int>() + kBcSideInts, stream);
  stage_side_home("ttr_barcodes_page", StageSide{&bc_side, kBcSideInts, kBcHdr, kBcRec, 1, "barcode"}, nq, {{hits_out, &bc_hits, hit_b}, {cnt_out, &bc_cnt, cnt_b}},
                  [&](const int32_t* side, std::string* why) { return barcodes_side_valid(side, h, w, min_lines, symbologies, why); }, side_out, item_out);
}

void Engine::ink_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int radius, int drop, int polarity, uint64_t* bits_out,
                       uint64_t* bitsT_out, InkRec* rec) {
  const StagedPage pg = stage_page("ttr_ink_page", img, h, w, row_stride, dev_offset, dev_stride, 32768,
                                   ink_args_ok(radius, drop, polarity) ? nullptr : "radius must lie in 1..64, drop in 1..255 and polarity in 0..2");
  tab_bits.ensure(tables_bits_slot(h, w) * 8); tab_bitsT.ensure(tables_bitsT_slot(h, w) * 8);
  tab_ink_h.ensure(ink_ws_bytes(h, w, 1)); tab_ink_rec.ensure(ink_recs_bytes(1));
  launch_ink_local(pg.data, 0, pg.stride, h, w, nullptr, 1, h, w, radius, drop, polarity, tab_ink_h.as<uint32_t>(), tab_ink_rec.as<InkRec>(), tab_bits.as<uint64_t>(),
                   tab_bitsT.as<uint64_t>(), stream);
  InkRec r{};
  TTR_HIP_CHECK(hipMemcpyAsync(&r, tab_ink_rec.p, sizeof r, hipMemcpyDeviceToHost, stream));
  if (bits_out) TTR_HIP_CHECK(hipMemcpyAsync(bits_out, tab_bits.p, tables_bits_slot(h, w) * 8, hipMemcpyDeviceToHost, stream));
  if (bitsT_out) TTR_HIP_CHECK(hipMemcpyAsync(bitsT_out, tab_bitsT.p, tables_bitsT_slot(h, w) * 8, hipMemcpyDeviceToHost, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));
  std::string why;
  if (!ink_rec_valid(r, radius, drop, polarity, h, w, &why)) throw std::runtime_error("ttr_ink_page: the record holds " + why);
  if (rec) *rec = r;
}

void Engine::recog_enqueue(PageBatch& B) {
  const int N = B.N, sl = B.slot;
  batch_bits = kBitsNone; batch_offsets_up = false;   // this batch's bitmaps and zero offsets: nothing in place yet (engine.h)
  // the slot's side-block records: disarmed, then armed by each layer that runs for this batch (engine.h: SideCopy)
  for (SideCopy* c : {&h_orient, &h_lines, &h_blocks, &h_chars, &h_alts, &h_lex, &h_pat_logp, &h_wide, &h_curve, &h_tab, &h_tab_ink, &h_mark, &h_barcode}) c->disarm(sl);
  const int line_words = cfg.lines && N > 0 ? stage_batch_lines(B, sl) : 0;   // text lines: the host part, before anything of this batch is enqueued
  if (cfg.chars && N > 0) stage_batch_chars(B, sl);                          // character boxes: likewise
  B.alts = orient_k() > 1 ? 0 : alts;        // character alternatives: fixed for the batch here (the setter refuses while batches stream)
  B.lex_m = lex_v && orient_k() <= 1 ? lex_m : 0;   // lexicon matching: likewise (0 = no lexicon set)
  B.lex_band = B.lex_m ? lex_band : -1;             // ... and its fuzzy alignment: likewise (-1 = the rigid scorer); every test of the mode below is on the host
  B.pat_best = pattern_decode == TTR_PATTERN_BEST && N > 0 && (B.regions ? !B.region_pats.start_of.empty() : pattern_own.delta != nullptr);   // patterns in best mode: likewise, and only with a pattern in force
  range_use(kRangeRec0 + (sl & 1));          // the recogniser's kernels of this batch watch the slot's own word
  const int X = B.X;                         // wide words: the pieces behind the batch's N, read as a pass of their own (DESIGN.md "Wide words"); 0 with wide off
  B.rows = std::max(N + X, comm ? B.cap : 0);   // the output block's rows (RecOut): with a communicator, the gathered payload's rows per rank
  const size_t block = (size_t)B.rows * kRecWords * 4;
  h_ids[sl].ensure(block + 4);
  const RecOut out = rec_out(B.rows);
  TTR_HIP_CHECK(hipEventRecord(evr[sl][0], stream));
  if (N > 0) {
    const int K = orient_k(), T = (K - 1) * N;                 // word orientation: T twin crops behind the batch's N (DESIGN.md "Word orientation")
    crops.ensure((size_t)(N + T + X) * kCropBytes);
    logits.ensure((size_t)std::max(std::max(N, X), T) * kLogitWords * 4);
    if (X) h_wide.arm(sl, wide_cuts_bytes((int)B.wide.size()));
    if (!B.curve.empty()) h_curve.arm(sl, curve_side_bytes(N));
    const RecOut cand = T ? rec_block(orient_cand, T) : RecOut{};
    if (T) { orient_side.ensure(orient_side_bytes(N, K, B.n)); h_orient.arm(sl, orient_side_bytes(N, K, B.n)); }
    RecPass main;   // the batch's N rows: the scratch logits, the standard block, the engine's own set
    main.crops = crops.as<uint8_t>(); main.N = N; main.logits = logits.as<float>(); main.out = out; main.mask = charset;
    // character alternatives: the side block of this batch (the setter refuses an engine with orientation, so T is 0 here)
    if (B.alts) { main.alt = alts_out(N, B.alts); h_alts.arm(sl, alts_side_bytes(N, B.alts)); }
    // lexicon matching: the side block and the scorer's partials of this batch
    if (B.lex_m) { main.lex = lex_out(N, B.lex_m, B.lex_band, lex_gap); h_lex.arm(sl, lex_side_bytes(N, B.lex_m, B.lex_band)); }
    // patterns in best mode: the scratch block of the masked argmax and the side block of this batch
    if (B.pat_best) { main.best = pat_best_out(N); h_pat_logp.arm(sl, pat_logp_bytes(N)); }
    pack_batch_crops(B, sl);
    if (T) pack_twin_crops(B, sl);
    if (cfg.lines) group_batch_lines(B, sl, line_words);               // text lines: from the boxes alone, so inside the packing stage (DESIGN.md "Text lines")
    if (cfg.blocks) group_batch_blocks(B, sl, line_words);             // text blocks: directly behind, from the lines' side block on the device (DESIGN.md "Text blocks")
    if (B.tab_min_len) tables_enqueue(B, sl);                          // tables: the pages' own pixels and the boxes just made (DESIGN.md "Tables")
    if (B.mark_min) marks_enqueue(B, sl);                              // selection marks: likewise, on the bitmaps tables formed when it is on (DESIGN.md "Selection marks")
    if (B.bc_min) barcodes_enqueue(B, sl);                             // barcodes: likewise, on the bitmaps tables or marks formed under the same rule (DESIGN.md "Barcodes")
    TTR_HIP_CHECK(hipEventRecord(evr[sl][1], stream));
    if (B.regions) {   // the caller's sets: one mask by value (the engine's own path), or the rows' table through the slot's pinned staging (one copy, no launch)
      main.mask = B.region_mask;
      if (!B.region_pats.start_of.empty()) main.pat = stage_row_patterns(B.region_pats, sl, B.pat_best ? &main.best.ext : nullptr);   // ... and the regions' patterns: the call's table the same way (one more copy, no launch)
      main.row_masks = stage_row_masks(B.row_masks, sl);
    }
    parseq_forward(main);
    // the passes behind the batch's own read the crops from row N on.  The logits are scratch: every pass starts at their base, so they are named here and not
    // sliced; the side blocks and the call's pattern table belong to the batch's N rows alone
    auto behind = [&](int n) {
      RecPass r = main.rows(N, n);
      r.logits = logits.as<float>(); r.alt = AltOut{}; r.lex = LexOut{}; r.pat = PatDev{}; r.best = PatBestOut{};
      return r;
    };
    // wide words: the X other pieces as a pass of their own, into rows N.. of the same block - the batch's N rows keep their batch, and with it every bit of
    // the words that are not wide (the recogniser picks its kernels by the row count)
    if (X) parseq_forward(behind(X));
    if (T) {   // the twins as a pass of their own (turn 0 keeps its batch, and with it its bits), then the choice, in place in the standard block
      RecPass twin = behind(T);
      twin.out = cand; twin.mask = charset; twin.row_masks = nullptr;   // a block of their own, under the engine's own set
      parseq_forward(twin);
      const size_t first_off = (size_t)T * 84;
      launch_orient_select(out.ids, out.prob, out.conf, cand.ids, cand.prob, cand.conf, reinterpret_cast<const int*>(orient_in.as<uint8_t>() + first_off), B.n, N, K,
                           cfg.orient_page, orient_side.as<int>(), stream);
    }
    if (cfg.chars) cut_batch_chars(B, sl, out.ids, T ? orient_side.as<int>() : nullptr);   // character boxes: K and the turn are the chosen reading's, read on the device
    TTR_HIP_CHECK(hipEventRecord(evr[sl][2], stream));
    TTR_HIP_CHECK(hipMemcpyAsync(h_ids[sl].p, ids_dev.p, block, hipMemcpyDeviceToHost, stream));   // ids, prob and conf in one copy
  } else {
    if (B.mark_min && !B.regions) marks_enqueue(B, sl);                // selection marks: a batch of pages without words - boxes only - is a legitimate form
    if (B.bc_min && !B.regions) barcodes_enqueue(B, sl);               // barcodes: likewise - a label is a legitimate page
    TTR_HIP_CHECK(hipEventRecord(evr[sl][1], stream));
    TTR_HIP_CHECK(hipEventRecord(evr[sl][2], stream));
  }
  // the side blocks that are not copied inside their layer's own enqueue function, behind the standard block's copy: each a no-op unless its layer armed it
  // (h_wide: the cuts, the profile stays on the device; h_tab_ink: the tables / marks pass's ink records; h_mark: there for a batch without words too)
  const std::pair<SideCopy*, const DevBuf*> tail[] = {{&h_orient, &orient_side}, {&h_alts, &alts_side}, {&h_lex, &lex_side}, {&h_pat_logp, &pat_logp_dev}, {&h_wide, &wide_side},
                                                      {&h_curve, &curve_side}, {&h_tab, &tab_side}, {&h_tab_ink, &tab_ink_rec}, {&h_mark, &mark_side},
                                                      {&h_barcode, &bc_side}};
  for (const auto& t : tail) t.first->fetch(sl, *t.second, stream);
  if (comm && B.cap > 0) {   // the payload: the output block of cap rows per rank - [cap][26] ids | [cap][26] prob | [cap] conf -, straight from the recogniser's device buffer
    gath_dev[sl].ensure(block * comm->world);
    h_gath[sl].ensure(block * comm->world);
    comm->tr->all_gather(ids_dev.p, gath_dev[sl].p, block, false, stream);
    TTR_HIP_CHECK(hipMemcpyAsync(h_gath[sl].p, gath_dev[sl].p, block * comm->world, hipMemcpyDeviceToHost, stream));
  }
  range_fetch(kRangeRec0 + (sl & 1));
  TTR_HIP_CHECK(hipEventRecord(done_ev[sl], stream));
  B.enqueued = true;
}

void Engine::finish(PageBatch& B, std::vector<Result>& results) {
  const int n = B.n;
  results.assign(n, Result());
  const double th2 = now_us();
  spin_event(done_ev[B.slot]);
  range_verify(kRangeRec0 + (B.slot & 1), "the recogniser of a batch of pages");
  const double th3 = now_us();
  // stage times: detector events belong to the latest batch enqueued (complete by now: its components were collected), recogniser events to this one
  (void)hipEventElapsedTime(&stage_ms[0], ev[0], ev[1]); (void)hipEventElapsedTime(&stage_ms[1], ev[1], ev[2]);
  (void)hipEventElapsedTime(&stage_ms[2], evr[B.slot][0], evr[B.slot][1]); (void)hipEventElapsedTime(&stage_ms[3], evr[B.slot][1], evr[B.slot][2]);
  if (profiling) prof_collect();
  const double th4 = now_us();
  if (comm) {   // compact the gathered payload: (rank, page, crop) order, no padding
    const GatherLayout L = GatherLayout::from_counts(B.all_counts.data(), comm->world, n);
    last_gathered.world = L.world; last_gathered.pages = n; last_gathered.counts = B.all_counts;
    compact_gathered(h_gath[B.slot].as<int32_t>(), B.cap, L.total, last_gathered);
  }
  SideViews V;   // null where the layer did not run for this batch
  V.orient = h_orient.view<int32_t>(B.slot); V.lines = h_lines.view<int32_t>(B.slot); V.blocks = h_blocks.view<int32_t>(B.slot); V.chars = h_chars.view<int32_t>(B.slot);
  V.alts = h_alts.view<int32_t>(B.slot); V.lex = h_lex.view<int32_t>(B.slot); V.pat_logp = h_pat_logp.view<float>(B.slot); V.wide_cuts = h_wide.view<int32_t>(B.slot);
  V.curve = h_curve.view<int32_t>(B.slot); V.tab = h_tab.view<int32_t>(B.slot); V.tab_ink = h_tab_ink.view<InkRec>(B.slot); V.mark = h_mark.view<int32_t>(B.slot);
  V.barcode = h_barcode.view<int32_t>(B.slot);
  decode_pages(B, rec_rows(h_ids[B.slot].p, B.rows), V, results);
  for (Result& r : results) r.tiles = B.tiles;                                                  // tiled pages: the tiles each page's detector ran as (0: off)
  host_us[5] = (float)(th3 - th2); host_us[6] = (float)(th4 - th3); host_us[7] = (float)(now_us() - th4);
  B.live = false; B.enqueued = false;
}

void Engine::decode_words(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int N = B.N, K = orient_k();
  r.text.reserve(cnt); r.bbox.reserve((size_t)cnt * 4); r.quad.reserve((size_t)cnt * 8);
  r.ids.assign(&rows.ids[(size_t)c0 * 26], &rows.ids[(size_t)(c0 + cnt) * 26]);
  r.prob.assign(&rows.prob[(size_t)c0 * 26], &rows.prob[(size_t)(c0 + cnt) * 26]);
  r.conf.assign(&rows.conf[c0], &rows.conf[c0 + cnt]);
  r.alt_k = B.alts;
  if (V.alts && cnt > 0) {   // [N][26][K] ids | [N][26][K] prob -> the page's rows
    const size_t w = (size_t)26 * B.alts;
    const int32_t* ai = V.alts;
    const float* ap = reinterpret_cast<const float*>(ai + (size_t)N * w);
    r.alt_ids.assign(ai + (size_t)c0 * w, ai + (size_t)(c0 + cnt) * w);
    r.alt_prob.assign(ap + (size_t)c0 * w, ap + (size_t)(c0 + cnt) * w);
  }
  r.lex_m = B.lex_m; r.lex_band = B.lex_band;
  if (V.lex && cnt > 0) {   // [N][M] idx | [N][M] logp -> the page's rows
    const size_t w = (size_t)B.lex_m;
    const int32_t* li = V.lex;
    const float* ll = reinterpret_cast<const float*>(li + (size_t)N * w);
    r.lex_idx.assign(li + (size_t)c0 * w, li + (size_t)(c0 + cnt) * w);
    r.lex_logp.assign(ll + (size_t)c0 * w, ll + (size_t)(c0 + cnt) * w);
    if (B.lex_band >= 0) {     // fuzzy alignment: [N][M] edits behind the two blocks
      const int32_t* le = li + (size_t)N * w * 2;
      r.lex_edits.assign(le + (size_t)c0 * w, le + (size_t)(c0 + cnt) * w);
    }
  }
  if (V.pat_logp && cnt > 0) r.pattern_logp.assign(V.pat_logp + c0, V.pat_logp + c0 + cnt);
  if (K > 1) {
    r.orient_k = K;
    if (const int32_t* side = V.orient) {   // [N] chosen turn | [N][K] candidate conf | [pages] page turn
      const float* o_conf = reinterpret_cast<const float*>(side + N);
      const int32_t* o_page = side + (size_t)N * (K + 1);
      r.orient.assign(&side[c0], &side[c0 + cnt]);
      r.orient_conf.assign(&o_conf[(size_t)c0 * K], &o_conf[(size_t)(c0 + cnt) * K]);
      r.page_orient = o_page[pg];
    }
  }
  if (B.regions) {   // the caller's quads verbatim, their corners' extremes, their set indices
    r.quad.assign(&B.region_quad[(size_t)c0 * 8], &B.region_quad[(size_t)(c0 + cnt) * 8]);
    r.set.assign(&B.region_set[c0], &B.region_set[c0 + cnt]);
  }
  for (int k = 0; k < cnt; ++k) {
    r.text.push_back(tok.decode(&rows.ids[(size_t)(c0 + k) * 26], 26));   // :486-505
    float bb[4];
    if (B.regions) region_bbox(&r.quad[(size_t)k * 8], bb);
    else { tesseract_bbox(B.boxes[pg][k], bb); push_quad(B.boxes[pg][k], r.quad); }   // :511
    r.bbox.insert(r.bbox.end(), bb, bb + 4);
  }
}

void Engine::decode_records(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int n = B.n, N = B.N;
  if (B.dsk_M) {   // deskew: the page's record, checked before anything is built on it
    if (B.dsk_recs.size() != (size_t)n) throw std::runtime_error("deskew: the batch carries no records");
    const DeskewRec& d = B.dsk_recs[(size_t)pg];
    std::string why;
    if (!deskew_rec_valid(d, B.dsk_M, B.pages[(size_t)pg].h, B.pages[(size_t)pg].w, dsk_cs_host.data(), &why))
      throw std::runtime_error("deskew: the record of page " + std::to_string(pg) + " holds " + why);
    r.skew_on = 1; r.skew = d;
  } else if (deskew_M && B.regions) {   // a region call: the caller's quadrilaterals are in the caller's frame
    r.skew_on = 1; r.skew = DeskewRec{0, 0, 65536, 0, B.pages[(size_t)pg].w, B.pages[(size_t)pg].h, 0, 0, 0, 0};
  }
  if (B.ink_radius && !B.regions && ((B.tab_min_len && N > 0) || B.mark_min || B.bc_min || B.dsk_M)) {   // local ink: the page's record - the tables, marks or barcodes pass's when one ran, else the deskew pass's - checked before anything is built on it
    const bool from_tab = (B.tab_min_len && N > 0) || B.mark_min || B.bc_min;
    if (from_tab ? !V.tab_ink : B.dsk_ink_recs.size() != (size_t)n) throw std::runtime_error("local ink: the batch carries no records");
    const InkRec k = from_tab ? V.tab_ink[pg] : B.dsk_ink_recs[(size_t)pg];
    std::string why;
    if (!ink_rec_valid(k, B.ink_radius, B.ink_drop, B.ink_polarity, B.pages[(size_t)pg].h, B.pages[(size_t)pg].w, &why))
      throw std::runtime_error("local ink: the record of page " + std::to_string(pg) + " holds " + why);
    if (from_tab && B.dsk_M) {   // both passes ran: the deskew pass's record is checked as well (its page is the caller's, of the same size)
      if (B.dsk_ink_recs.size() != (size_t)n) throw std::runtime_error("local ink: the batch carries no records");
      if (!ink_rec_valid(B.dsk_ink_recs[(size_t)pg], B.ink_radius, B.ink_drop, B.ink_polarity, B.pages[(size_t)pg].h, B.pages[(size_t)pg].w, &why))
        throw std::runtime_error("local ink: the deskew pass's record of page " + std::to_string(pg) + " holds " + why);
    }
    r.ink_on = 1; r.ink = k;
  }
}

void Engine::decode_tables(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int n = B.n;
  if (B.tab_min_len && !B.regions && cnt > 0) {   // tables: the page's side block and its words' cells, checked before anything is built on them
    if (!V.tab) throw std::runtime_error("tables: the batch carries no side block");
    const int32_t* ts = V.tab + (size_t)pg * kTabSideInts;
    const int32_t* ti = V.tab + (size_t)n * kTabSideInts + 2 * (size_t)c0;
    std::string why;
    if (!tables_side_valid(ts, &why)) throw std::runtime_error("tables: the side block of page " + std::to_string(pg) + " holds " + why);
    int32_t counts[4];
    tables_export(ts, counts, nullptr, nullptr, nullptr, nullptr);
    r.table_mode = ts[0];
    r.rulings.assign((size_t)counts[0] * 6, 0); r.tables.assign((size_t)counts[1] * 8, 0); r.cells.assign((size_t)counts[2] * 9, 0); r.table_lines.assign((size_t)counts[3], 0);
    tables_export(ts, counts, r.rulings.data(), r.tables.data(), r.table_lines.data(), r.cells.data());
    r.item_table.assign((size_t)cnt, -1); r.item_cell.assign((size_t)cnt, -1);
    for (int k = 0; k < cnt; ++k) {
      const int t = ti[2 * k], c = ti[2 * k + 1];
      const bool none = t == -1 && c == -1;
      if (!none && (t < 0 || t >= counts[1] || c < r.tables[(size_t)t * 8 + 6] || c >= r.tables[(size_t)t * 8 + 6] + r.tables[(size_t)t * 8 + 7]))
        throw std::runtime_error("tables: word " + std::to_string(k) + " of page " + std::to_string(pg) + " names a table or cell that does not exist");
      r.item_table[(size_t)k] = t; r.item_cell[(size_t)k] = c;
    }
  }
}

void Engine::decode_marks(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int n = B.n;
  if (B.mark_min && !B.regions) {   // selection marks: the page's side block and its items' marks, checked before anything is built on them
    if (!V.mark) throw std::runtime_error("marks: the batch carries no side block");
    const int32_t* ms = V.mark + (size_t)pg * kMarkSideInts;
    const int32_t* mi = V.mark + (size_t)n * kMarkSideInts + (size_t)c0;
    std::string why;
    if (!marks_side_valid(ms, B.pages[(size_t)pg].h, B.pages[(size_t)pg].w, B.mark_fill, cnt, &why))
      throw std::runtime_error("marks: the side block of page " + std::to_string(pg) + " holds " + why);
    r.mark_mode = ms[0];
    r.marks.assign(ms + kMarkHdr, ms + kMarkHdr + (size_t)kMarkRec * ms[1]);
    r.item_mark.assign((size_t)cnt, -1);
    for (int k = 0; k < cnt; ++k) {
      if (mi[k] < -1 || mi[k] >= ms[1]) throw std::runtime_error("marks: word " + std::to_string(k) + " of page " + std::to_string(pg) + " names a mark that does not exist");
      r.item_mark[(size_t)k] = mi[k];
    }
  }
}

void Engine::decode_barcodes(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int n = B.n;
  if (B.bc_min && !B.regions) {   // barcodes: the page's side block and its items' barcodes, checked before anything is built on them
    if (!V.barcode) throw std::runtime_error("barcodes: the batch carries no side block");
    const int32_t* bs = V.barcode + (size_t)pg * kBcSideInts;
    const int32_t* bi = V.barcode + (size_t)n * kBcSideInts + (size_t)c0;
    std::string why;
    if (!barcodes_side_valid(bs, B.pages[(size_t)pg].h, B.pages[(size_t)pg].w, B.bc_min, B.bc_sym, &why))
      throw std::runtime_error("barcodes: the side block of page " + std::to_string(pg) + " holds " + why);
    r.barcode_mode = bs[0];
    r.barcodes.assign(bs + kBcHdr, bs + kBcHdr + (size_t)kBcRec * bs[1]);
    r.item_barcode.assign((size_t)cnt, -1);
    for (int k = 0; k < cnt; ++k) {
      if (bi[k] < -1 || bi[k] >= bs[1]) throw std::runtime_error("barcodes: word " + std::to_string(k) + " of page " + std::to_string(pg) + " names a barcode that does not exist");
      r.item_barcode[(size_t)k] = bi[k];
    }
  }
}

void Engine::decode_curved(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int N = B.N;
  if (B.curved && cnt > 0) {   // curved words: every item's flag, outline and knot table, checked before anything is built on them
    if (!V.curve) throw std::runtime_error("curved words: the batch carries no side block");
    const int32_t* cs = V.curve;
    const int64_t* ct = reinterpret_cast<const int64_t*>(reinterpret_cast<const uint8_t*>(V.curve) + curve_side_table_offset(N));
    r.curved.assign((size_t)cnt, 0); r.outline.assign((size_t)cnt * 36, 0.f); r.spine_knots.assign((size_t)cnt * 36, 0);
    for (int k = 0; k < cnt; ++k) {
      const size_t c = (size_t)(c0 + k);
      CurveWord w{};
      w.flag = cs[c]; w.hb[0] = cs[(size_t)N + 2 * c]; w.hb[1] = cs[(size_t)N + 2 * c + 1];
      memcpy(w.table, ct + 36 * c, sizeof w.table);
      if (!curve_word_valid(w))
        throw std::runtime_error("curved words: the side block of word " + std::to_string(k) + " of page " + std::to_string(pg) +
                                 " holds a flag that is not 0 or 1, a half band outside 0..32 or a knot outside the int32 pixel range");
      r.curved[(size_t)k] = w.flag;
      memcpy(&r.spine_knots[(size_t)k * 36], w.table, sizeof w.table);
      curve_outline(&r.quad[(size_t)k * 8], w.flag, &w.table[0][0], &r.outline[(size_t)k * 36]);
    }
  }
}

void Engine::decode_wide(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at;
  if (B.wide_aspect != 0.f && cnt > 0) {   // wide words: every item's pieces; a wide item's text and conf joined from them (its ids and prob stay its first piece's)
    r.piece_first.assign((size_t)cnt + 1, 0);
    r.piece_cuts.assign((size_t)cnt * 17, -1);
    for (int k = 0; k < cnt; ++k) {
      const int wi = B.wide_of[(size_t)(c0 + k)];
      r.piece_first[(size_t)k + 1] = r.piece_first[k] + (wi < 0 ? 1 : B.wide[(size_t)wi].n);
    }
    const size_t P = (size_t)r.piece_first[cnt];
    r.piece_ids.reserve(P * 26); r.piece_prob.reserve(P * 26); r.piece_conf.reserve(P); r.piece_quad.assign(P * 8, 0.f);
    for (int k = 0; k < cnt; ++k) {
      const int c = c0 + k, wi = B.wide_of[(size_t)c];
      int32_t* cuts = &r.piece_cuts[(size_t)k * 17];
      float* pq = &r.piece_quad[8 * (size_t)r.piece_first[k]];
      if (wi < 0) {
        cuts[0] = 0; cuts[1] = kWideCols;
        r.piece_ids.insert(r.piece_ids.end(), &rows.ids[(size_t)c * 26], &rows.ids[(size_t)(c + 1) * 26]);
        r.piece_prob.insert(r.piece_prob.end(), &rows.prob[(size_t)c * 26], &rows.prob[(size_t)(c + 1) * 26]);
        r.piece_conf.push_back(rows.conf[c]);
        std::copy(&r.quad[(size_t)k * 8], &r.quad[(size_t)k * 8 + 8], pq);
        continue;
      }
      const WideWord& W = B.wide[(size_t)wi];
      if (!V.wide_cuts || !wide_cuts_valid(V.wide_cuts + 17 * (size_t)wi, W.n))
        throw std::runtime_error("wide words: the side block of word " + std::to_string(k) + " of page " + std::to_string(pg) + " does not hold " + std::to_string(W.n) +
                                 " ascending pieces of 64 to 192 columns");
      std::copy(V.wide_cuts + 17 * (size_t)wi, V.wide_cuts + 17 * (size_t)wi + 17, cuts);
      wide_piece_quads(&r.quad[(size_t)k * 8], cuts, W.n, pq);
      std::string text;
      float conf = 1.0f;
      for (int j = 0; j < W.n; ++j) {
        const size_t row = j == 0 ? (size_t)c : (size_t)W.extra + (size_t)j - 1;
        r.piece_ids.insert(r.piece_ids.end(), &rows.ids[row * 26], &rows.ids[(row + 1) * 26]);
        r.piece_prob.insert(r.piece_prob.end(), &rows.prob[row * 26], &rows.prob[(row + 1) * 26]);
        r.piece_conf.push_back(rows.conf[row]);
        text += tok.decode(&rows.ids[row * 26], 26);
        conf = conf * rows.conf[row];
      }
      r.text[(size_t)k] = text;
      r.conf[(size_t)k] = conf;
    }
  }
}

void Engine::decode_lines(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int N = B.N;
  if (V.lines && cnt > 0) {   // [N] line | [N] word | [pages] n_lines -> the page's lines in reading order
    r.line.assign(&V.lines[c0], &V.lines[c0 + cnt]);
    r.word.assign(&V.lines[(size_t)N + c0], &V.lines[(size_t)N + c0 + cnt]);
    r.n_lines = V.lines[2 * (size_t)N + pg];
    r.order.assign(cnt, 0);
    r.line_first.assign((size_t)std::max(r.n_lines, 0) + 1, 0);
    if (!lines_reading_order(r.line.data(), r.word.data(), cnt, r.n_lines, r.order.data(), r.line_first.data()))
      throw std::runtime_error("text lines: the side block of page " + std::to_string(pg) + " is not a numbering of its lines");
    r.line_bbox.assign((size_t)r.n_lines * 4, 0.f);
    for (int l = 0; l < r.n_lines; ++l) bbox_union(r.bbox, r.order, r.line_first[l], r.line_first[l + 1], &r.line_bbox[4 * (size_t)l]);
  }
}

void Engine::decode_blocks(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int n = B.n, N = B.N;
  if (V.blocks && V.lines && cnt > 0) {   // [N] block | [N] pos | [pages] n_blocks | [pages] mode, per line -> the page's blocks in reading order
    const int nl = r.n_lines;
    r.line_block.assign(&V.blocks[c0], &V.blocks[c0 + nl]);
    r.line_pos.assign(&V.blocks[(size_t)N + c0], &V.blocks[(size_t)N + c0 + nl]);
    r.n_blocks = V.blocks[2 * (size_t)N + pg];
    r.block_mode = V.blocks[2 * (size_t)N + n + pg];
    if (r.n_blocks < 1 || r.n_blocks > nl)   // (checked before anything is sized by it)
      throw std::runtime_error("text blocks: the side block of page " + std::to_string(pg) + " is not a numbering of its blocks");
    r.block_order.assign((size_t)nl, 0);
    r.block_first.assign((size_t)r.n_blocks + 1, 0);
    if ((r.block_mode != 0 && r.block_mode != 1) ||
        !blocks_reading_order(r.line_block.data(), r.line_pos.data(), nl, r.n_blocks, r.block_order.data(), r.block_first.data()))
      throw std::runtime_error("text blocks: the side block of page " + std::to_string(pg) + " is not a numbering of its blocks");
    r.block.resize((size_t)cnt);
    for (int k = 0; k < cnt; ++k) r.block[k] = r.line_block[r.line[k]];
    r.block_bbox.assign((size_t)r.n_blocks * 4, 0.f);
    for (int b = 0; b < r.n_blocks; ++b) bbox_union(r.line_bbox, r.block_order, r.block_first[b], r.block_first[b + 1], &r.block_bbox[4 * (size_t)b]);
  }
}

void Engine::decode_chars(const PageCtx& at, Result& r) const {
  const auto& [B, rows, V, pg, c0, cnt] = at; const int N = B.N;
  if (V.chars && cnt > 0) {   // [N][27] cuts | [N] mode | [N][128] u8 profile -> the page's characters
    const int32_t* cuts = V.chars;
    const int32_t* modes = cuts + (size_t)N * 27;
    const uint8_t* prof = reinterpret_cast<const uint8_t*>(cuts + (size_t)N * 28);
    r.char_cuts.assign(&cuts[(size_t)c0 * 27], &cuts[(size_t)(c0 + cnt) * 27]);
    r.char_mode.assign(&modes[c0], &modes[c0 + cnt]);
    r.char_profile.assign(&prof[(size_t)c0 * 128], &prof[(size_t)(c0 + cnt) * 128]);
    r.char_first.assign((size_t)cnt + 1, 0);
    for (int k = 0; k < cnt; ++k) {
      const int K = text_chars(&r.ids[(size_t)k * 26]);
      if (!chars_cuts_valid(&r.char_cuts[(size_t)k * 27], K) || (r.char_mode[k] != 0 && r.char_mode[k] != 1))
        throw std::runtime_error("character boxes: the side block of word " + std::to_string(k) + " of page " + std::to_string(pg) + " does not hold " + std::to_string(K) + " ascending cells");
      r.char_first[(size_t)k + 1] = r.char_first[k] + K;
    }
    const size_t total = (size_t)r.char_first[cnt];
    r.char_quad.assign(total * 8, 0.f); r.char_bbox.assign(total * 4, 0.f);
    for (int k = 0; k < cnt; ++k) {
      const int K = r.char_first[(size_t)k + 1] - r.char_first[k];
      chars_quads_from_cuts(&r.quad[(size_t)k * 8], r.orient.empty() ? 0 : r.orient[k], &r.char_cuts[(size_t)k * 27], K, r.char_quad.data() + 8 * (size_t)r.char_first[k],
                            r.char_bbox.data() + 4 * (size_t)r.char_first[k]);
    }
  }
}

void Engine::decode_pages(const PageBatch& B, const RecRows& rows, const SideViews& views, std::vector<Result>& results) {
  const std::vector<int> first = page_first(B.page_of, B.n);
  auto decode_page = [&](int pg) {
    const PageCtx at{B, rows, views, pg, first[pg], first[pg + 1] - first[pg]};
    Result& r = results[pg];
    decode_words(at, r); decode_records(at, r); decode_tables(at, r); decode_marks(at, r); decode_barcodes(at, r); decode_curved(at, r); decode_wide(at, r);
    decode_lines(at, r); decode_blocks(at, r); decode_chars(at, r);
  };
  // pages decode independently
  if (B.N >= 256) parallel_pages(B.n, decode_page);
  else for (int pg = 0; pg < B.n; ++pg) decode_page(pg);
}

Engine::PageBatch Engine::mixed_batch(const ttr_page* pages, int n) {
  if (n > 0 && !pages) throw std::runtime_error("null argument");
  PageBatch B;
  B.n = n; B.mixed = true;
  B.pages.resize((size_t)std::max(n, 0));
  for (int i = 0; i < n; ++i) {
    // (a stride that does not fit the kernels' int stays invalid: check_pages refuses it as shorter than a row)
    const long long stride = pages[i].row_stride ? (long long)pages[i].row_stride : (long long)pages[i].w * 3;
    B.pages[i] = Page{pages[i].data, pages[i].h, pages[i].w, stride > 0x7fffffffLL ? -1 : (int)stride, CanvasGeom{}};
  }
  return B;
}

void Engine::run_pages(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& results) {
  PageBatch B;
  B.d_pages = d_pages; B.n = n; B.h = h; B.w = w;
  run_batch(B, results);
}

void Engine::run_pages_v(const ttr_page* pages, int n, std::vector<Result>& results) {
  PageBatch B = mixed_batch(pages, n);
  run_batch(B, results);
}

void Engine::run_batch(PageBatch& B, std::vector<Result>& results) {
  const int n = B.n;
  results.assign(std::max(n, 0), Result());
  if (n <= 0) return;
  if (q1.live || q2.live) throw std::runtime_error("streamed batches are in flight: call ttr_stream_flush until it returns none");
  const double th0 = now_us();
  // the reference's progress lines (tuatara.cpp:328-329, :342, :421, :434: the models are loaded once per engine here, so those
  // lines report a fact; :386, :488, :509), on request only: callers do not parse stdout
  if (verbose) std::cout << ttr_version() << " (HIP " << HIP_VERSION_MAJOR << "." << HIP_VERSION_MINOR << ")\ncraft model loaded" << std::endl;
  B.slot = 0;
  std::exception_ptr pre;
  { RangeScope r("ttr:detect_enqueue"); try { detect_enqueue(B); } catch (...) { if (!comm) throw; pre = std::current_exception(); } }
  host_us[0] = (float)(now_us() - th0);
  if (verbose) std::cout << "post processing craft predictions..." << std::endl;
  { RangeScope r("ttr:detect_collect"); detect_collect(B, pre); }
  const double th1 = now_us();
  if (verbose) std::cout << "loading parseq model...\nparseq model loaded" << std::endl;
  { RangeScope r("ttr:recog_enqueue"); recog_enqueue(B); }
  host_us[4] = (float)(now_us() - th1);
  if (verbose) std::cout << "Running tokenizer..." << std::endl;
  { RangeScope r("ttr:finish"); finish(B, results); }
  if (verbose) std::cout << "Elapsed time: " << (now_us() - th0) * 1e-6 << " seconds " << std::endl;
}

void Engine::resolve_row_masks(const char* what, const int32_t* set_of, int n, const uint32_t* sets, int n_sets, std::vector<uint32_t>& table, ClassMask& one) const {
  const std::string w(what);
  if (n_sets < 0 || (n_sets > 0 && !sets) || (n > 0 && !set_of)) throw std::runtime_error("null argument");
  std::vector<ClassMask> cms((size_t)n_sets);
  for (int s = 0; s < n_sets; ++s) {
    if (!(sets[3 * (size_t)s] & 1u)) throw std::runtime_error(w + ": set " + std::to_string(s) + ": bit 0 (the end of the text) must be set");
    cms[s] = ClassMask::from_allowed(sets + 3 * (size_t)s);
  }
  table.assign((size_t)n * 4, 0u);
  one = charset;
  bool same = true, restricts = false;
  for (int i = 0; i < n; ++i) {
    if (set_of[i] < -1 || set_of[i] >= n_sets)
      throw std::runtime_error(w + ": item " + std::to_string(i) + " names set " + std::to_string(set_of[i]) + ", the call holds " + std::to_string(n_sets) + " (-1 = the engine's own)");
    const ClassMask& m = set_of[i] < 0 ? charset : cms[(size_t)set_of[i]];
    for (int k = 0; k < 3; ++k) table[4 * (size_t)i + k] = m.blocked[k];
    if (i == 0) one = m;
    same = same && !memcmp(m.blocked, one.blocked, sizeof one.blocked);
    restricts = restricts || m.restricts();
  }
  if (restricts && prec == kBF16)
    throw std::runtime_error(w + ": a character set needs an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which take no class mask");
  if (same) table.clear();
}

const RowMask* Engine::stage_row_masks(const std::vector<uint32_t>& table, int sl) {
  if (table.empty()) return nullptr;
  const size_t bytes = table.size() * 4;
  h_row_masks[sl & 1].ensure(bytes); row_masks_dev.ensure(bytes);
  memcpy(h_row_masks[sl & 1].p, table.data(), bytes);
  TTR_HIP_CHECK(hipMemcpyAsync(row_masks_dev.p, h_row_masks[sl & 1].p, bytes, hipMemcpyHostToDevice, stream));
  return row_masks_dev.as<RowMask>();
}

void Engine::set_engine_pattern(const char* src_, const ClassMask& cm) {
  if (!src_ || !*src_) { pattern_src.clear(); pattern = Pattern(); pattern_own = PatDev{}; return; }   // (pattern.states = 0: best mode's extent of the engine's own pattern is read from `pattern`)
  const std::string src(src_);   // (a copy: the caller may pass pattern_src itself)
  uint32_t m[3];
  cm.allowed(m);
  Pattern p =pattern_compile(tok, src.c_str(), m);   // (throws before anything changes)
  const size_t db = p.delta.size() * sizeof(uint16_t), mb = p.mind.size();
  pattern_dev.ensure(db + mb);
  TTR_HIP_CHECK(hipMemcpyAsync(pattern_dev.p, p.delta.data(), db, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipMemcpyAsync(pattern_dev.as<uint8_t>() + db, p.mind.data(), mb, hipMemcpyHostToDevice, stream));
  TTR_HIP_CHECK(hipStreamSynchronize(stream));        // (the host vectors are pageable; a setter may wait)
  pattern_own = PatDev{pattern_dev.as<uint16_t>(), pattern_dev.as<uint8_t>() + db, nullptr, p.start};
  pattern = std::move(p);
  pattern_src = src;
}

bool Engine::resolve_row_patterns(const char* what, const char* const* patterns, int n_patterns, const int32_t* pattern_of, int n, const std::vector<uint32_t>& table,
                                  const ClassMask& one, PatRows& out) const {
  const std::string w(what);
  if (n_patterns < 0 || (n_patterns > 0 && !patterns)) throw std::runtime_error("null argument");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const int k = pattern_of ? pattern_of[i] : -1;
    if (k < -1 || k >= n_patterns)
      throw std::runtime_error(w + ": item " + std::to_string(i) + " names pattern " + std::to_string(k) + ", the call holds " + std::to_string(n_patterns) + " (-1 = the engine's own)");
    any = any || k >= 0 || !pattern_src.empty();
  }
  out.t = PatternTable(); out.start_of.clear(); out.extent_of.clear();
  if (!any) return false;
  if (prec == kBF16) throw std::runtime_error(w + ": a pattern needs an f16x4 or f32 engine: the bf16 engine chooses its tokens inside gemm_sk.hip and dec_fused.hip, which know no automaton");
  if (alts || lex_v) throw std::runtime_error(w + ": patterns do not combine with character alternatives or a lexicon (ttr_engine_set_alternatives(e, 0) / ttr_engine_set_lexicon(e, NULL, 0, 0) first)");
  // each distinct (pattern, mask) pair once; a row without a pattern: a DONE state alone under its mask
  struct Key { int k; uint32_t m[3]; bool operator<(const Key& o) const { return k != o.k ? k < o.k : memcmp(m, o.m, sizeof m) < 0; } };
  std::map<Key, int> index;
  std::vector<Pattern> autos;
  std::vector<int> of((size_t)n);
  int total = 0;
  for (int i = 0; i < n; ++i) {
    Key key{};
    const uint32_t* b = table.empty() ? one.blocked : &table[4 * (size_t)i];
    ClassMask{{b[0], b[1], b[2]}}.allowed(key.m);
    const int k = pattern_of ? pattern_of[i] : -1;
    const char* src = k >= 0 ? patterns[k] : (pattern_src.empty() ? nullptr : pattern_src.c_str());
    key.k = k >= 0 ? k : (src ? -1 : -2);
    auto it = index.find(key);
    if (it == index.end()) {
      try {
        autos.push_back(key.k == -2 ? pattern_none(key.m) : pattern_compile(tok, src ? src : "", key.m));
      } catch (const std::runtime_error& e) { throw std::runtime_error(w + ": item " + std::to_string(i) + ": " + e.what()); }
      total += autos.back().rows();
      it = index.emplace(key, (int)autos.size() - 1).first;
    }
    of[(size_t)i] = it->second;
  }
  if (total > kPatMaxTable) throw std::runtime_error(w + ": the call's patterns need " + std::to_string(total) + " automaton states in all: at most 1024 fit one table");
  std::vector<int> start(autos.size());
  for (size_t a = 0; a < autos.size(); ++a) start[a] = out.t.add(autos[a], what);
  out.start_of.resize((size_t)n);
  out.extent_of.resize(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    const size_t a = (size_t)of[(size_t)i];
    out.start_of[(size_t)i] = start[a];
    out.extent_of[2 * (size_t)i] = start[a] - autos[a].start; out.extent_of[2 * (size_t)i + 1] = autos[a].states;
  }
  return true;
}

PatDev Engine::stage_row_patterns(const PatRows& r, int sl, PatExtent* ext) {
  // delta | start_of | mind (| extent_of in best mode, behind the mind bytes rounded up to 4), in this order so that each part is aligned to its element
  const size_t db = r.t.delta.size() * sizeof(uint16_t), sb = r.start_of.size() * 4, mb = r.t.mind.size();
  const size_t eo = (db + sb + mb + 3) & ~(size_t)3, eb = ext ? r.extent_of.size() * 4 : 0, total = ext ? eo + eb : db + sb + mb;
  if (ext && r.extent_of.size() != 2 * r.start_of.size()) throw std::runtime_error("patterns: the rows' extents are missing");
  PinnedBuf& h = h_pat_rows[sl & 1];
  h.ensure(total); pat_rows_dev.ensure(total);
  memcpy(h.p, r.t.delta.data(), db);
  memcpy(h.as<uint8_t>() + db, r.start_of.data(), sb);
  memcpy(h.as<uint8_t>() + db + sb, r.t.mind.data(), mb);
  if (ext) memcpy(h.as<uint8_t>() + eo, r.extent_of.data(), eb);
  TTR_HIP_CHECK(hipMemcpyAsync(pat_rows_dev.p, h.p, total, hipMemcpyHostToDevice, stream));
  uint8_t* d = pat_rows_dev.as<uint8_t>();
  if (ext) *ext = PatExtent{reinterpret_cast<const int32_t*>(d + eo), 0, 0};
  return PatDev{reinterpret_cast<const uint16_t*>(d), d + db + sb, reinterpret_cast<const int32_t*>(d + db), 0};
}

void Engine::run_regions(const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets, std::vector<Result>& results,
                         const char* const* patterns, int n_patterns, const int32_t* pattern_of) {
  const char* what = "regions";
  // ---- every refusal, before anything is enqueued or changed
  if (n_pages < 0 || n < 0 || (n_pages > 0 && !pages) || (n > 0 && !regions)) throw std::runtime_error("null argument");
  refuse_while_streaming(what);
  if (comm) throw std::runtime_error("regions: a communicator is attached: regions are read by one engine alone (ttr_engine_attach_comm(e, NULL) first)");
  if (cfg.orient || cfg.lines || cfg.chars || cfg.blocks)
    throw std::runtime_error(std::string("regions: the engine has ") + (cfg.orient ? "orient" : cfg.lines ? "lines" : cfg.chars ? "chars" : "blocks") +
                             " set: that layer reads the detector's boxes (group regions with ttr_group_lines / ttr_group_blocks on their quads)");
  PageBatch B;
  B.n = n_pages; B.mixed = true; B.regions = true; B.slot = 0;
  B.pages.resize((size_t)n_pages);
  for (int i = 0; i < n_pages; ++i) {
    const long long stride = pages[i].row_stride ? (long long)pages[i].row_stride : (long long)pages[i].w * 3;
    if (!pages[i].data || pages[i].h <= 0 || pages[i].w <= 0 || stride < (long long)pages[i].w * 3 || stride > 0x7fffffffLL) throw std::runtime_error("Error reading image from file");
    // (no canvas: the table row's resize geometry is never read by the packers; the identity keeps it well defined)
    B.pages[i] = Page{pages[i].data, pages[i].h, pages[i].w, (int)stride, CanvasGeom{pages[i].h, pages[i].w, pages[i].h, pages[i].w, 1.f}};
  }
  std::vector<int32_t> set_of((size_t)n);
  for (int i = 0; i < n; ++i) {
    const ttr_region& R = regions[i];
    if (R.page < 0 || R.page >= n_pages) throw std::runtime_error("regions: region " + std::to_string(i) + " names page " + std::to_string(R.page) + ", the call holds " + std::to_string(n_pages));
    if (!region_quad_ok(R.quad)) throw std::runtime_error("regions: region " + std::to_string(i) + " has a coordinate that is not finite or has |x| >= 32768");
    if (cfg.strict_crops && !region_inside(R.quad, pages[R.page].h, pages[R.page].w))
      throw std::runtime_error("regions: region " + std::to_string(i) + " has a corner outside page " + std::to_string(R.page) + "'s pixel edges (strict_crops = 1)");
    set_of[i] = R.set;
  }
  std::vector<uint32_t> table;
  ClassMask one{};
  resolve_row_masks(what, set_of.data(), n, sets, n_sets, table, one);
  if (n_patterns > 0 && n > 0 && !pattern_of) throw std::runtime_error("null argument");
  PatRows pats;   // (in the caller's order; the batch holds them in crop order)
  const bool with_pats = resolve_row_patterns(what, patterns, n_patterns, pattern_of, n, table, one, pats);
  if (with_pats && wide != 0.f) throw std::runtime_error("regions: patterns do not combine with wide words (a pattern spans the whole text, a piece reads a part of it): ttr_engine_set_wide(e, 0) first");
  results.assign((size_t)n_pages, Result());
  if (n_pages == 0) return;
  // ---- the batch: crops by page, then in the caller's order within the page (a stable counting sort)
  std::vector<int> first((size_t)n_pages + 1, 0), at;
  for (int i = 0; i < n; ++i) first[(size_t)regions[i].page + 1]++;
  for (int p = 0; p < n_pages; ++p) first[p + 1] += first[p];
  at.assign(first.begin(), first.end() - 1);
  B.N = n;
  B.page_of.assign((size_t)n, 0); B.rects.assign((size_t)n * 5, 0); B.coef.assign((size_t)n * 8, 0);
  B.region_quad.assign((size_t)n * 8, 0.f); B.region_set.assign((size_t)n, 0);
  if (!table.empty()) B.row_masks.assign((size_t)n * 4, 0u);
  if (with_pats) { B.region_pats.t = std::move(pats.t); B.region_pats.start_of.assign((size_t)n, 0); B.region_pats.extent_of.assign(2 * (size_t)n, 0); }
  B.region_mask = one;
  for (int i = 0; i < n; ++i) {
    const ttr_region& R = regions[i];
    const size_t c = (size_t)at[R.page]++;
    B.page_of[c] = R.page;
    int* rc = &B.rects[5 * c];
    rc[0] = 0; rc[1] = 0; rc[2] = 1; rc[3] = 1; rc[4] = R.page;   // (kind 1 reads the coefficients alone; the rectangle only has to be non-empty)
    int64_t fx[6];
    region_coef(R.quad, fx);
    B.coef[8 * c] = 1;
    for (int k = 0; k < 6; ++k) B.coef[8 * c + 1 + k] = fx[k];
    memcpy(&B.region_quad[8 * c], R.quad, 8 * sizeof(float));
    B.region_set[c] = R.set;
    if (!table.empty()) memcpy(&B.row_masks[4 * c], &table[4 * (size_t)i], 16);
    if (with_pats) {
      B.region_pats.start_of[c] = pats.start_of[(size_t)i];
      B.region_pats.extent_of[2 * c] = pats.extent_of[2 * (size_t)i]; B.region_pats.extent_of[2 * c + 1] = pats.extent_of[2 * (size_t)i + 1];
    }
  }
  plan_wide(B, B.region_quad.data());   // wide words: the pieces' rows behind the call's n (DESIGN.md "Wide words")
  plan_curved(B, B.region_quad.data());   // curved words: every region is a candidate (DESIGN.md "Curved words")
  const double th0 = now_us();
  for (int k = 0; k < 3; ++k) TTR_HIP_CHECK(hipEventRecord(ev[k], stream));   // no detector: its two stage times of this call are zero
  if (n > 0) upload_page_table(B.pages, 0);
  host_us[0] = host_us[1] = host_us[2] = host_us[3] = 0.f;
  { RangeScope r("ttr:recog_enqueue"); recog_enqueue(B); }
  host_us[4] = (float)(now_us() - th0);
  { RangeScope r("ttr:finish"); finish(B, results); }
}

void Engine::run_pages_sharded(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& results) {
  if (wide != 0.f) throw std::runtime_error("latency mode does not support wide words: ttr_engine_set_wide(e, 0) first");
  if (curved) throw std::runtime_error("latency mode does not support curved words: ttr_engine_set_curved(e, 0) first");
  if (tables_min_len) throw std::runtime_error("latency mode does not support tables: ttr_engine_set_tables(e, 0, 0) first");
  if (marks_min) throw std::runtime_error("latency mode does not support selection marks: ttr_engine_set_marks(e, 0, 0, 0, 0) first");
  if (barcodes_min) throw std::runtime_error("latency mode does not support barcodes: ttr_engine_set_barcodes(e, 0, 0, 0) first");
  if (tiled) throw std::runtime_error("latency mode does not support tiled pages: ttr_engine_set_tiled(e, 0) first");
  if (deskew_M) throw std::runtime_error("latency mode does not support deskew: ttr_engine_set_deskew(e, 0, 0, 0) first");
  if (!comm) throw std::runtime_error("latency mode needs a communicator (ttr_engine_attach_comm)");
  if (cfg.orient != TTR_ORIENT_OFF) throw std::runtime_error("latency mode does not support word orientation: create the engine with orient = TTR_ORIENT_OFF");
  if (cfg.blocks) throw std::runtime_error("latency mode does not support text blocks: create the engine with blocks = 0");
  if (cfg.lines) throw std::runtime_error("latency mode does not support text lines: create the engine with lines = 0");
  if (cfg.chars) throw std::runtime_error("latency mode does not support character boxes: create the engine with chars = 0");
  if (alts) throw std::runtime_error("latency mode does not support character alternatives: ttr_engine_set_alternatives(e, 0) first");
  if (lex_v) throw std::runtime_error("latency mode does not support lexicon matching: ttr_engine_set_lexicon(e, NULL, 0, 0) first");
  if (pattern_decode == TTR_PATTERN_BEST && !pattern_src.empty())
    throw std::runtime_error("latency mode does not support the best decode of patterns: ttr_engine_set_pattern_decode(e, TTR_PATTERN_GREEDY) first");
  if (q1.live || q2.live) throw std::runtime_error("streamed batches are in flight: call ttr_stream_flush until it returns none");
  Comm* const c = comm;
  const int world = c->world, rank = c->rank;
  PageBatch B;
  int32_t hdr[2] = {0, 0};                                     // {pages, crops} of rank 0
  comm = nullptr;                                              // (the detector below is not the throughput mode's: no per-batch gather)
  try {
    if (rank == 0) {
      if (!d_pages || n <= 0) throw std::runtime_error("latency mode: rank 0 passes the pages");
      B.d_pages = d_pages; B.n = n; B.h = h; B.w = w; B.slot = 0;
      detect_enqueue(B);
      detect_collect(B);
      hdr[0] = n; hdr[1] = B.N;
    }
  } catch (...) { comm = c; hdr[0] = -1; std::vector<int32_t> all(2 * world); allgather_host(hdr, 8, all.data()); throw; }
  comm = c;
  std::vector<int32_t> all(2 * (size_t)world);
  allgather_host(hdr, 8, all.data());
  if (all[0] < 0) throw std::runtime_error("latency mode: rank 0 failed in the detector");
  const int pages = all[0], N = all[1];
  results.assign(rank == 0 ? pages : std::max(n, 0), Result());
  if (N == 0) return;
  const int per = (N + world - 1) / world;
  const int lo = std::min(N, rank * per), hi = std::min(N, lo + per);
  crops.ensure((size_t)world * per * kCropBytes);           // (the last shard may be ragged: the buffer holds world * per crops)
  if (rank == 0) {
    pack_batch_crops(B, 0);
  }
  c->tr->broadcast(crops.p, (size_t)N * kCropBytes, 0, stream);
  logits.ensure((size_t)per * kLogitWords * 4);
  const RecOut out = rec_out(per);                              // per rank: [per][26] ids | [per][26] prob | [per] conf, one collective
  const size_t block = (size_t)per * kRecWords * 4;
  range_use(kRangeRec0);
  RecPass shard;   // this rank's rows of the broadcast crops, into the base of its own logits and block
  shard.crops = crops.as<uint8_t>(); shard.mask = charset;
  shard = shard.rows(lo, hi - lo);
  shard.logits = logits.as<float>(); shard.out = out;
  parseq_forward(shard);
  gath_dev[0].ensure((size_t)world * block);
  h_gath[0].ensure((size_t)world * block);
  c->tr->all_gather(ids_dev.p, gath_dev[0].p, block, false, stream);
  TTR_HIP_CHECK(hipMemcpyAsync(h_gath[0].p, gath_dev[0].p, (size_t)world * block, hipMemcpyDeviceToHost, stream));
  range_fetch(kRangeRec0);
  TTR_HIP_CHECK(hipEventRecord(done_ev[0], stream));
  spin_event(done_ev[0]);
  range_verify(kRangeRec0, "the recogniser of a sharded page");
  if (rank != 0) return;
  // shard r (per rows, the last one ragged) holds crops [r * per, r * per + total[r])
  std::vector<int> total(world);
  for (int r = 0; r < world; ++r) total[r] = std::max(0, std::min(per, N - r * per));
  Gathered g;
  compact_gathered(h_gath[0].as<int32_t>(), per, total, g);
  decode_pages(B, RecRows{g.ids.data(), g.prob.data(), g.conf.data()}, SideViews{}, results);
}

void Engine::stream_push(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& prev_results, int& prev_n) {
  PageBatch B;
  B.d_pages = d_pages; B.n = n; B.h = h; B.w = w;
  push_batch(std::move(B), prev_results, prev_n);
}

void Engine::stream_push_v(const ttr_page* pages, int n, std::vector<Result>& prev_results, int& prev_n) {
  prev_results.clear(); prev_n = 0;
  push_batch(mixed_batch(pages, n), prev_results, prev_n);
}

void Engine::push_batch(PageBatch&& B, std::vector<Result>& prev_results, int& prev_n) {
  prev_results.clear(); prev_n = 0;
  if (B.n <= 0) throw std::runtime_error("stream_push: empty batch");
  const double th0 = now_us();
  B.slot = q1.live ? (q1.slot ^ 1) : 0;     // from the pipeline's state, not a counter: a push that throws leaves q1 / q2 and the slot parity as they were
  std::exception_ptr pre;      // (with a communicator: a failing rank still takes part in this batch's header exchange, detect_collect)
  stream_fail_age = 0;
  { RangeScope r("ttr:detect_enqueue"); try { detect_enqueue(B); } catch (...) { if (!comm) throw; pre = std::current_exception(); } }
  host_us[0] = (float)(now_us() - th0);
  const double th1 = now_us();
  if (q1.live && !q1.enqueued) {
    RangeScope r("ttr:recog_enqueue");
    struct Flag { bool& f; ~Flag() { f = false; } } flag{streaming_recog};
    streaming_recog = true;
    // (recog_overlap: everything recog_enqueue puts on "the stream" - packer, recogniser, id copy, completion event - goes to the recogniser's own stream)
    struct StreamSwap { Engine& E; bool on; StreamSwap(Engine& e, bool o) : E(e), on(o) { if (on) std::swap(E.stream, E.recog_stream); } ~StreamSwap() { if (on) std::swap(E.stream, E.recog_stream); } }
        swap_guard{*this, tn.recog_overlap != 0};
    recog_enqueue(q1);
  }
  host_us[4] = (float)(now_us() - th1);
  { RangeScope r("ttr:detect_collect"); detect_collect(B, pre); }
  // (a batch whose recogniser tripped the range guard fails HERE, once: the pipeline still advances - on every rank alike, so no rank skips a collective its
  // peers issue - and the neighbours' results survive)
  std::exception_ptr fin;
  if (q2.live) { RangeScope r("ttr:finish"); prev_n = q2.n; try { finish(q2, prev_results); } catch (...) { fin = std::current_exception(); prev_results.clear(); prev_n = 0; q2.live = false; } }
  if (q1.live) q2 = std::move(q1);
  q1 = std::move(B);
  q1.live = true; q1.enqueued = false;
  if (fin) { stream_fail_age = 2; std::rethrow_exception(fin); }
}

void Engine::stream_flush(std::vector<Result>& prev_results, int& prev_n) {
  prev_results.clear(); prev_n = 0;
  stream_fail_age = 2;
  if (q1.live && !q1.enqueued) {
    const bool sw = tn.recog_overlap != 0;
    if (sw) std::swap(stream, recog_stream);
    try { recog_enqueue(q1); } catch (...) { if (sw) std::swap(stream, recog_stream); throw; }
    if (sw) std::swap(stream, recog_stream);
  }
  // (a batch that fails in finish leaves the pipeline: the next flush returns the next batch)
  if (q2.live) { prev_n = q2.n; try { finish(q2, prev_results); } catch (...) { q2.live = false; prev_results.clear(); prev_n = 0; throw; } return; }
  if (q1.live) { prev_n = q1.n; try { finish(q1, prev_results); } catch (...) { q1.live = false; prev_results.clear(); prev_n = 0; throw; } }
}

// ---- image_to_data over a list of host images (engine.h: run_images)
void Engine::run_images(const std::vector<HostImage>& imgs, std::vector<Result>& results, std::vector<int>& failed, std::string& first_error) {
  const int n = (int)imgs.size();
  results.assign(n, Result());
  failed.clear(); first_error.clear();
  last_batches.clear();
  if (n == 0) return;
  if (q1.live || q2.live) throw std::runtime_error("streamed batches are in flight: call ttr_stream_flush until it returns none");
  if (comm) throw std::runtime_error("ttr_images_to_data runs on one engine: detach the communicator (every rank takes its own list)");
  const bool mixed = cfg.mixed_batches != 0;   // buckets are canvases, batches run through the table path (DESIGN.md "Mixed-size batches")
  std::vector<char> bad(n, 0);
  for (int i = 0; i < n; ++i) {
    const HostImage& im = imgs[i];
    if (!im.data || im.h <= 0 || im.w <= 0 || (im.row_stride >= 0 && im.row_stride < (std::ptrdiff_t)im.w * 3)) {   // tuatara.cpp:344-347: this image yields nothing, the others go on
      std::cerr << "Error reading image from file";
      bad[i] = 1; failed.push_back(i);
      if (first_error.empty()) first_error = "Error reading image from file (image " + std::to_string(i) + ")";
    } else if (tiled) {   // tiled pages: a page the tile plan refuses (a side above 8192, too many tiles) fails alone, with the plan's message
      try { (void)page_geometry(im.h, im.w); }
      catch (const std::exception& ex) {
        std::cerr << "tuatara: " << ex.what() << std::endl;
        bad[i] = 1; failed.push_back(i);
        if (first_error.empty()) first_error = std::string(ex.what()) + " (image " + std::to_string(i) + ")";
      }
    } else if (mixed) {   // a page the resize cannot take would fail its whole batch: it fails alone, here, and its canvas-mates go on
      const CanvasGeom g = canvas_geometry(im.h, im.w, cfg.canvas_size, cfg.mag_ratio);
      if (g.target_h <= 0 || g.target_w <= 0) {
        std::cerr << "tuatara: image too thin to resize" << std::endl;
        bad[i] = 1; failed.push_back(i);
        if (first_error.empty()) first_error = "image too thin to resize (image " + std::to_string(i) + ")";
      }
    }
  }
  // buckets of equal (h, w), the largest canvases first (the engine's grow-only workspaces then grow once), cut into batches
  // (mixed: buckets of equal canvas (h32, w32) instead, input order inside a bucket; the map's order breaks ties of the sort below by ascending key)
  std::map<std::pair<int, int>, std::vector<int>> by_size;
  for (int i = 0; i < n; ++i) {
    if (bad[i]) continue;
    if (mixed) { const CanvasGeom g = page_geometry(imgs[i].h, imgs[i].w); by_size[{g.h32, g.w32}].push_back(i); }
    else by_size[{imgs[i].h, imgs[i].w}].push_back(i);
  }
  std::vector<std::pair<std::pair<int, int>, std::vector<int>>> buckets(by_size.begin(), by_size.end());
  std::stable_sort(buckets.begin(), buckets.end(), [&](const auto& a, const auto& b) {
    if (mixed) return (size_t)a.first.first * a.first.second > (size_t)b.first.first * b.first.second;
    const CanvasGeom ga = page_geometry(a.first.first, a.first.second), gb = page_geometry(b.first.first, b.first.second);
    return (size_t)ga.h32 * ga.w32 > (size_t)gb.h32 * gb.w32;
  });
  struct Batch { int h, w; std::vector<int> idx; std::vector<size_t> off; };   // off (mixed): [idx.size() + 1] every image's offset in the staging slot, rounded up to 256 bytes
  std::vector<Batch> batches;
  size_t max_bytes = 0;
  const int cap = std::max(1, tn.images_batch);
  for (auto& b : buckets)
    for (size_t o = 0; o < b.second.size(); o += cap) {
      Batch t{b.first.first, b.first.second, std::vector<int>(b.second.begin() + o, b.second.begin() + std::min(b.second.size(), o + cap)), {}};
      if (mixed) {
        t.off.assign(1, 0);
        for (int i : t.idx) t.off.push_back((t.off.back() + (size_t)imgs[i].h * imgs[i].w * 3 + 255) & ~(size_t)255);
        max_bytes = std::max(max_bytes, t.off.back());
      } else {
        max_bytes = std::max(max_bytes, t.idx.size() * (size_t)t.h * t.w * 3);
      }
      batches.push_back(std::move(t));
    }
  for (const Batch& b : batches) last_batches.push_back((int32_t)b.idx.size());
  if (!up_stream) {
    TTR_HIP_CHECK(hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking));
    for (auto& x : up_ev) TTR_HIP_CHECK(hipEventCreateWithFlags(&x, hipEventDisableTiming));
  }
  for (int s = 0; s < kStageSlots && s < (int)batches.size(); ++s) { stage_host[s].ensure(max_bytes); stage_dev[s].ensure(max_bytes); }
  // stage(j): the rows of batch j's images, tightly packed, into pinned slot j % 4; one copy to the device on the upload stream; an event behind it
  std::exception_ptr stage_err;
  auto stage = [&](int j) {
    try {
      TTR_HIP_CHECK(hipSetDevice(cfg.device));
      const Batch& b = batches[j];
      const int sl = j % kStageSlots;
      uint8_t* dst = stage_host[sl].as<uint8_t>();
      if (mixed) {   // every image tightly packed at its own offset; one copy of the slot's used bytes
        for (size_t k = 0; k < b.idx.size(); ++k) {
          const HostImage& im = imgs[b.idx[k]];
          const size_t row = (size_t)im.w * 3;
          if (im.row_stride == (std::ptrdiff_t)row) memcpy(dst + b.off[k], im.data, row * im.h);
          else for (int y = 0; y < im.h; ++y) memcpy(dst + b.off[k] + (size_t)y * row, im.data + (std::ptrdiff_t)y * im.row_stride, row);
        }
        TTR_HIP_CHECK(hipMemcpyAsync(stage_dev[sl].p, dst, b.off.back(), hipMemcpyHostToDevice, up_stream));
        TTR_HIP_CHECK(hipEventRecord(up_ev[sl], up_stream));
        return;
      }
      const size_t page = (size_t)b.h * b.w * 3, row = (size_t)b.w * 3;
      for (size_t k = 0; k < b.idx.size(); ++k) {
        const HostImage& im = imgs[b.idx[k]];
        if (im.row_stride == (std::ptrdiff_t)row) memcpy(dst + k * page, im.data, page);
        else for (int y = 0; y < b.h; ++y) memcpy(dst + k * page + (size_t)y * row, im.data + (std::ptrdiff_t)y * im.row_stride, row);
      }
      TTR_HIP_CHECK(hipMemcpyAsync(stage_dev[sl].p, dst, b.idx.size() * page, hipMemcpyHostToDevice, up_stream));
      TTR_HIP_CHECK(hipEventRecord(up_ev[sl], up_stream));
    } catch (...) { stage_err = std::current_exception(); }
  };
  const int nb = (int)batches.size();
  std::thread helper;
  struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{helper};
  auto deliver = [&](int j, std::vector<Result>& res, int cnt) {       // batch j's results go to its images' places in the caller's order
    if (cnt != (int)batches[j].idx.size()) throw std::runtime_error("ttr_images_to_data: a batch came back with another page count");
    for (int k = 0; k < cnt; ++k) results[batches[j].idx[k]] = std::move(res[k]);
  };
  auto fail_batch = [&](int j, const std::string& why) {               // a batch that failed on the GPU: its images keep empty results, the list goes on
    for (int i : batches[j].idx) failed.push_back(i);
    if (first_error.empty()) first_error = why + " (images of batch " + std::to_string(j) + ")";
    std::cerr << "tuatara: " << why << std::endl;
  };
  auto drain = [&]() {                                                 // a call-level error mid-list: nothing stays in flight behind it
    std::vector<Result> r; int c = 0;
    for (int guard = 0; guard < 3 && (q1.live || q2.live); ++guard) { try { stream_flush(r, c); } catch (...) { q1 = PageBatch(); q2 = PageBatch(); } }
  };
  if (nb == 0) { std::sort(failed.begin(), failed.end()); return; }
  std::deque<int> inflight;                                            // batches inside the streamed pipeline, oldest first
  stage(0);
  if (stage_err) std::rethrow_exception(stage_err);
  try {
    for (int j = 0; j < nb; ++j) {
      if (helper.joinable()) helper.join();
      if (stage_err) std::rethrow_exception(stage_err);
      if (j + 1 < nb) helper = std::thread(stage, j + 1);               // (slot (j + 1) % 4 last held batch j - 3: returned one push ago at the latest)
      TTR_HIP_CHECK(hipStreamWaitEvent(stream, up_ev[j % kStageSlots], 0));
      std::vector<Result> prev; int np = 0;
      try {
        if (mixed) {
          const Batch& b = batches[j];
          std::vector<ttr_page> pg(b.idx.size());
          for (size_t k = 0; k < b.idx.size(); ++k) pg[k] = ttr_page{stage_dev[j % kStageSlots].as<uint8_t>() + b.off[k], imgs[b.idx[k]].h, imgs[b.idx[k]].w, 0};
          stream_push_v(pg.data(), (int)pg.size(), prev, np);
        } else {
          stream_push(stage_dev[j % kStageSlots].as<uint8_t>(), (int)batches[j].idx.size(), batches[j].h, batches[j].w, prev, np);
        }
        inflight.push_back(j);
        if (np) { deliver(inflight.front(), prev, np); inflight.pop_front(); }
      } catch (const std::exception& ex) {
        if (stream_fail_age == 2 && !inflight.empty()) { fail_batch(inflight.front(), ex.what()); inflight.pop_front(); inflight.push_back(j); }   // the batch whose results were due; j is in
        else fail_batch(j, ex.what());                                                                                                            // batch j's own detector: it never entered
      }
    }
    if (helper.joinable()) helper.join();
    while (!inflight.empty()) {
      std::vector<Result> prev; int np = 0;
      try {
        stream_flush(prev, np);
        if (np) deliver(inflight.front(), prev, np);
        else throw std::runtime_error("ttr_images_to_data: the pipeline ran dry with batches outstanding");
      } catch (const std::exception& ex) { fail_batch(inflight.front(), ex.what()); }
      inflight.pop_front();
    }
  } catch (...) {
    if (helper.joinable()) helper.join();
    drain();
    throw;
  }
  drain();   // (nothing should be left; a batch that failed inside a push may have left a neighbour parked)
  std::sort(failed.begin(), failed.end());
}

}  // namespace ttr
