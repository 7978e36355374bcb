// Developer hooks of include/tuatara_hip_debug.h: single-kernel test entry points, micro-benchmarks, the tuning registry.
#include "engine.h"
#include "tables_rule.h"
#include "barcodes_rule.h"
#include "marks_rule.h"

using namespace ttr;

extern "C" {

int ttr_dbg_conv(ttr_engine* e, const float* in0, int C0, const float* in1, int C1, int relu0, int relu1, int B, int H, int W, int ks, int dil,
                 const float* wgt, const float* bias, int Cout, int act, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  const size_t M = (size_t)B * H * W;
  const int K = ks * ks * (C0 + C1);
  DevBuf d0, d1, dout;
  Linear L;
  auto up = [&](DevBuf& d, const float* src, size_t nel) {
    d.ensure(nel * E.es);
    if (E.prec == kBF16) {
      std::vector<uint16_t> hbuf(nel);
      for (size_t i = 0; i < nel; ++i) hbuf[i] = f32_to_bf16_rne(src[i]);
      TTR_HIP_CHECK(hipMemcpy(d.p, hbuf.data(), nel * 2, hipMemcpyHostToDevice));
    } else TTR_HIP_CHECK(hipMemcpy(d.p, src, nel * 4, hipMemcpyHostToDevice));
  };
  up(d0, in0, M * C0);
  if (C1) up(d1, in1, M * C1);
  E.upload_linear(L, wgt, Cout, K, bias, Cout, K, nullptr, false);
  dout.ensure(M * Cout * 4);
  ConvParams p{};
  p.in0 = d0.p; p.C0 = C0; p.in1 = C1 ? d1.p : nullptr; p.C1 = C1; p.relu0 = relu0; p.relu1 = relu1;
  p.B = B; p.H = H; p.W = W; p.ks = ks; p.dil = dil; p.wgt = L.w.p; p.bias = bias ? L.b.as<float>() : nullptr;
  p.out = nullptr; p.out_f32 = dout.as<float>(); p.out_f32_ld = Cout; p.Cout = Cout; p.M = (int)M; p.act = act;
  const bool bf16_out = E.tn.dbg_bf16_out && E.prec == kBF16;
  if (bf16_out) { p.out = dout.p; p.out_ld = Cout; p.out_f32 = nullptr; p.out_f32_ld = 0; }
  launch_igemm(E.prec, p, E.stream);
  if (bf16_out) {
    std::vector<uint16_t> hb(M * Cout);
    TTR_HIP_CHECK(hipMemcpyAsync(hb.data(), dout.p, M * Cout * 2, hipMemcpyDeviceToHost, E.stream));
    TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
    for (size_t i = 0; i < hb.size(); ++i) { const uint32_t u = (uint32_t)hb[i] << 16; memcpy(&out[i], &u, 4); }
    return 0;
  }
  TTR_HIP_CHECK(hipMemcpyAsync(out, dout.p, M * Cout * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

// One split-operand linear layer on its own (tests): out[M][N] = act(x w^T + bias (+ resid)) through launch_gemm2's split mode (gemm_sp.hip's kernels
// where they apply), np = 3 (activation pairs) or 4 (triples); out_planes = 0 (the kernel writes fp32) or 2 / 3 (it writes f16 planes, joined here).
int ttr_dbg_split_gemm(ttr_engine* e, const float* x, int M, int K, const float* w, const float* bias, int N, int np, int act, int out_planes,
                       const float* resid, int cfg, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_split_gemm: f16x4 engines only");
  if ((np != 3 && np != 4) || (out_planes != 0 && out_planes != 2 && out_planes != 3)) throw std::runtime_error("ttr_dbg_split_gemm: np must be 3 or 4, out_planes 0, 2 or 3");
  const int ipl = np == 3 ? 2 : 3;
  DevBuf dx, dxp, dout, dres;
  Linear L;
  dx.ensure((size_t)M * K * 4); TTR_HIP_CHECK(hipMemcpy(dx.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
  dxp.ensure((size_t)M * K * 2 * ipl);
  launch_split_planes(dx.as<float>(), K, dxp.p, M, K, 0, E.stream, ipl);
  E.upload_linear(L, w, N, K, bias, cfg == 7 ? (N + 7) / 8 * 8 : N, K, nullptr, false);   // (the skinny kernel takes any channel count: zero rows pad the planes)
  if (!L.ws.p) throw std::runtime_error("ttr_dbg_split_gemm: the layer has no weight planes");
  if (resid) { dres.ensure((size_t)M * N * 4); TTR_HIP_CHECK(hipMemcpy(dres.p, resid, (size_t)M * N * 4, hipMemcpyHostToDevice)); }
  dout.ensure((size_t)M * N * (out_planes ? 2 * out_planes : 4));
  ConvParams p{};
  p.in0 = dxp.p; p.C0 = K; p.B = 1; p.H = 1; p.W = M; p.ks = 1; p.dil = 1;
  if (E.tn.sp_tiled_w) E.tile_planes(L);                       // (what the engine's own layers hand gemm_sp.hip)
  p.wgt = L.ws.p; p.bias = bias ? L.b.as<float>() : nullptr; p.split = np; p.out_scale = L.inv_scale; p.out_planes = out_planes;
  p.wgt_tiled = E.tn.sp_tiled_w ? L.wst.p : nullptr;
  if (out_planes) { p.out = dout.p; p.out_ld = N; } else { p.out_f32 = dout.as<float>(); p.out_f32_ld = N; }
  p.resid = resid ? dres.as<float>() : nullptr; p.resid_ld = N;
  p.Cout = N; p.M = M; p.act = act;
  if (cfg == 7) launch_gemm_skx(p, E.stream);       // the skinny whole-K kernel (gemm_skx.hip: triples; throws for shapes it does not take)
  else {
    if (const char* err = gemm2_check(p)) throw std::runtime_error(err);
    launch_gemm2(p, cfg, E.stream);
  }
  if (!out_planes) {
    TTR_HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, E.stream));
    TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
    return 0;
  }
  std::vector<uint16_t> h((size_t)M * N * out_planes);
  TTR_HIP_CHECK(hipMemcpyAsync(h.data(), dout.p, h.size() * 2, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  auto f16_to_f32 = [](uint16_t v) -> double {
    const int sgn = v >> 15, ex = (v >> 10) & 31, man = v & 1023;
    double r = ex == 0 ? std::ldexp((double)man, -24) : ex == 31 ? (man ? NAN : INFINITY) : std::ldexp((double)(man | 1024), ex - 25);
    return sgn ? -r : r;
  };
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) {
      const uint16_t* row = h.data() + (size_t)m * out_planes * N;
      double v = f16_to_f32(row[n]), lo = f16_to_f32(row[N + n]);
      if (out_planes == 3) lo += f16_to_f32(row[2 * N + n]);
      out[(size_t)m * N + n] = (float)(v + lo / 2048.0);
    }
  return 0;
  TTR_GUARD_END(-1)
}

// The split kernel on its own (tests): split_planes_kernel over host rows, the f16 planes back as the bits the kernel wrote.  The launch watches a word of its
// own (tag 1: a tag of 0, the scope's default, would leave a tripped word at 0), so that the engine's sticky words never see a test's out-of-range value.
int ttr_dbg_split_planes(ttr_engine* e, const float* x, int M, int C, int ld, int planes, int relu, uint16_t* raw_out, int* tripped) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_split_planes");
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_split_planes: f16x4 engines only");
  if (!x || !raw_out || M < 1 || C < 8 || C % 8 || ld < C || ld % 4 || (planes != 2 && planes != 3)) throw std::runtime_error("ttr_dbg_split_planes: M >= 1, C a multiple of 8, ld >= C a multiple of 4, planes 2 or 3");
  const size_t nin = (size_t)M * ld, nout = (size_t)M * planes * C;
  DevBuf dx, dout, dflag;
  dx.ensure(nin * 4); dout.ensure(nout * 2); dflag.ensure(4);
  TTR_HIP_CHECK(hipMemcpy(dx.p, x, nin * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemsetAsync(dflag.p, 0, 4, E.stream));
  {
    struct Restore { RangeCtx saved; ~Restore() { range_ctx() = saved; } } restore{range_ctx()};
    range_ctx().flag = dflag.as<unsigned>(); range_ctx().tag = 1;
    launch_split_planes(dx.as<float>(), ld, dout.p, M, C, relu, E.stream, planes);
  }
  unsigned word = 0;
  TTR_HIP_CHECK(hipMemcpyAsync(raw_out, dout.p, nout * 2, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipMemcpyAsync(&word, dflag.p, 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  if (tripped) *tripped = word != 0;
  return 0;
  TTR_GUARD_END(-1)
}

// layernorm_planes_kernel on its own (tests): the planes buffer back exactly as the kernel laid it out (row-major [M][planes][384], or gemm_sp.hip's loader pieces)
int ttr_dbg_layernorm_planes(ttr_engine* e, const float* x, int M, int ld, const float* gamma, const float* beta, float eps, int planes, int tiled, uint16_t* raw_out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_layernorm_planes");
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_layernorm_planes: f16x4 engines only");
  if (!x || !gamma || !beta || !raw_out || M < 1 || ld < 384 || ld % 4 || (planes != 2 && planes != 3)) throw std::runtime_error("ttr_dbg_layernorm_planes: M >= 1, ld >= 384 a multiple of 4, planes 2 or 3");
  const size_t nin = (size_t)M * ld, nout = (size_t)M * planes * 384;
  DevBuf dx, dg, db, dout;
  dx.ensure(nin * 4); dg.ensure(384 * 4); db.ensure(384 * 4); dout.ensure(nout * 2);
  TTR_HIP_CHECK(hipMemcpy(dx.p, x, nin * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(dg.p, gamma, 384 * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(db.p, beta, 384 * 4, hipMemcpyHostToDevice));
  launch_layernorm_planes(dx.as<float>(), ld, dg.as<float>(), db.as<float>(), eps, dout.p, M, E.stream, planes, nullptr, 0, tiled ? 1 : 0);
  TTR_HIP_CHECK(hipMemcpyAsync(raw_out, dout.p, nout * 2, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

// The decoder's LayerNorm + linear pair (K = 384) on its own (tests), both ways Engine::decoder_tail_split runs it: the LayerNorm kernel (triples) followed by the
// skinny linear, or the skinny linear with the LayerNorm as its prologue.
int ttr_dbg_ln_linear(ttr_engine* e, const float* x, int M, const float* gamma, const float* beta, float eps, const float* w, const float* bias, int N, int fused,
                      float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_ln_linear");
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_ln_linear: f16x4 engines only");
  if (!x || !gamma || !beta || !w || !out || M < 1 || N < 1) throw std::runtime_error("ttr_dbg_ln_linear: M, N >= 1");
  const int K = 384;
  DevBuf dx, dg, db, dxp, dout;
  Linear L;
  dx.ensure((size_t)M * K * 4); dg.ensure(K * 4); db.ensure(K * 4); dout.ensure((size_t)M * N * 4);
  TTR_HIP_CHECK(hipMemcpy(dx.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(dg.p, gamma, K * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(db.p, beta, K * 4, hipMemcpyHostToDevice));
  E.upload_linear(L, w, N, K, bias, (N + 7) / 8 * 8, K, nullptr, false);   // (the skinny kernel takes any channel count: zero rows pad the planes)
  if (!L.ws.p) throw std::runtime_error("ttr_dbg_ln_linear: the layer has no weight planes");
  ConvParams p{};
  p.C0 = K; p.B = 1; p.H = 1; p.W = M; p.ks = 1; p.dil = 1;
  p.wgt = L.ws.p; p.bias = bias ? L.b.as<float>() : nullptr; p.split = 4; p.out_scale = L.inv_scale;
  p.out_f32 = dout.as<float>(); p.out_f32_ld = N; p.Cout = N; p.M = M; p.act = kActNone;
  if (fused) {
    p.ln_in = dx.as<float>(); p.ln_ld = K; p.ln_gamma = dg.as<float>(); p.ln_beta = db.as<float>(); p.ln_eps = eps;
    if (!gemm_skx_ln_eligible(p)) throw std::runtime_error("ttr_dbg_ln_linear: the LayerNorm prologue does not take this shape");
  } else {
    dxp.ensure((size_t)M * K * 6);
    launch_layernorm_planes(dx.as<float>(), K, dg.as<float>(), db.as<float>(), eps, dxp.p, M, E.stream, 3);
    p.in0 = dxp.p;
  }
  launch_gemm_skx(p, E.stream);
  TTR_HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_mlp(ttr_engine* e, const float* x, int M, const float* ln_g, const float* ln_b, float eps, const float* w1, const float* b1, const float* w2,
                const float* b2, const float* nln_g, const float* nln_b, float* x_out, float* nln_out, const float* att, const float* wp, const float* bp) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec != kBF16) throw std::runtime_error("ttr_dbg_mlp: bf16 engines only");
  const int D = 384, H = 1536;
  DevBuf dx, dout, dg, db, dw1, db1, dw2, db2, dng, dnb, dn;
  auto upf = [&](DevBuf& d, const float* src, size_t n) { d.ensure(n * 4); TTR_HIP_CHECK(hipMemcpy(d.p, src, n * 4, hipMemcpyHostToDevice)); };
  upf(dx, x, (size_t)M * D); upf(dg, ln_g, D); upf(db, ln_b, D); upf(db1, b1, H); upf(db2, b2, D);
  if (nln_out) { upf(dng, nln_g, D); upf(dnb, nln_b, D); dn.ensure((size_t)M * D * 2); }
  std::vector<uint16_t> h((size_t)H * D);
  pack_mlp_w1(w1, h.data());
  dw1.ensure(h.size() * 2); TTR_HIP_CHECK(hipMemcpy(dw1.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  pack_mlp_w2(w2, H, h.data());
  dw2.ensure(h.size() * 2); TTR_HIP_CHECK(hipMemcpy(dw2.p, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  dout.ensure((size_t)M * D * 4);
  MlpParams q{};
  q.x = dx.as<float>(); q.x_out = dout.as<float>(); q.M = M; q.ln_g = dg.as<float>(); q.ln_b = db.as<float>(); q.ln_eps = eps;
  q.w1p = dw1.as<bf16>(); q.b1 = db1.as<float>(); q.w2p = dw2.as<bf16>(); q.b2 = db2.as<float>();
  if (nln_out) { q.nln_g = dng.as<float>(); q.nln_b = dnb.as<float>(); q.nln_eps = eps; q.nln_out = dn.as<bf16>(); }
  DevBuf datt, dwp, dbp;
  if (att) {
    std::vector<uint16_t> ha((size_t)M * D), hw((size_t)D * D);
    for (size_t i = 0; i < ha.size(); ++i) ha[i] = f32_to_bf16_rne(att[i]);
    pack_mlp_w2(wp, D, hw.data());
    datt.ensure(ha.size() * 2); TTR_HIP_CHECK(hipMemcpy(datt.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
    dwp.ensure(hw.size() * 2); TTR_HIP_CHECK(hipMemcpy(dwp.p, hw.data(), hw.size() * 2, hipMemcpyHostToDevice));
    upf(dbp, bp, D);
    q.att = datt.as<bf16>(); q.wpp = dwp.as<bf16>(); q.bp = dbp.as<float>();
  }
  launch_mlp_fused(q, E.stream);
  TTR_HIP_CHECK(hipMemcpyAsync(x_out, dout.p, (size_t)M * D * 4, hipMemcpyDeviceToHost, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  if (nln_out) {
    std::vector<uint16_t> hb((size_t)M * D);
    TTR_HIP_CHECK(hipMemcpy(hb.data(), dn.p, hb.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hb.size(); ++i) { const uint32_t u = (uint32_t)hb[i] << 16; memcpy(&nln_out[i], &u, 4); }
  }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_qkv_attn(ttr_engine* e, const float* x, int N, const float* w, const float* b, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec == kSplit) {   // the fused launch of the default precision: x -> pairs, weight rows head-major, output triples joined here
    const size_t nx = (size_t)N * 128 * 384;
    DevBuf dx, dxp, dout;
    Linear L;
    dx.ensure(nx * 4); TTR_HIP_CHECK(hipMemcpy(dx.p, x, nx * 4, hipMemcpyHostToDevice));
    dxp.ensure(nx * 4);
    launch_split_planes(dx.as<float>(), 384, dxp.p, (int64_t)N * 128, 384, 0, E.stream, 2);
    std::vector<float> wp((size_t)1152 * 384), bp(1152);
    for (int n = 0; n < 1152; ++n) { const int src = Engine::qkv_tile_row(n); memcpy(&wp[(size_t)n * 384], &w[(size_t)src * 384], 384 * 4); bp[n] = b[src]; }
    E.upload_linear(L, wp.data(), 1152, 384, bp.data(), 1152, 384, nullptr, false);
    dout.ensure(nx * 6);
    if (E.tn.sp_tiled_w) E.tile_planes(L);
    launch_qkv_attn_split(dxp.p, L.ws.p, L.b.as<float>(), L.inv_scale, dout.p, N, E.stream, E.tn.sp_tiled_w ? L.wst.p : nullptr);
    std::vector<_Float16> h(nx * 3);
    TTR_HIP_CHECK(hipMemcpyAsync(h.data(), dout.p, nx * 6, hipMemcpyDeviceToHost, E.stream));
    TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
    for (size_t m = 0; m < (size_t)N * 128; ++m)
      for (int c = 0; c < 384; ++c) {
        const _Float16* row = h.data() + m * 1152;
        out[m * 384 + c] = (float)((double)(float)row[c] + ((double)(float)row[384 + c] + (double)(float)row[768 + c]) / 2048.0);
      }
    return 0;
  }
  if (E.prec != kBF16) throw std::runtime_error("ttr_dbg_qkv_attn: bf16 and f16x4 engines only");
  const size_t nx = (size_t)N * 128 * 384, nw = (size_t)1152 * 384;
  DevBuf dx, dw, db, dout;
  std::vector<uint16_t> h(std::max(nx, nw));
  for (size_t i = 0; i < nx; ++i) h[i] = f32_to_bf16_rne(x[i]);
  dx.ensure(nx * 2); TTR_HIP_CHECK(hipMemcpy(dx.p, h.data(), nx * 2, hipMemcpyHostToDevice));
  for (size_t i = 0; i < nw; ++i) h[i] = f32_to_bf16_rne(w[i]);
  dw.ensure(nw * 2); TTR_HIP_CHECK(hipMemcpy(dw.p, h.data(), nw * 2, hipMemcpyHostToDevice));
  db.ensure(1152 * 4); TTR_HIP_CHECK(hipMemcpy(db.p, b, 1152 * 4, hipMemcpyHostToDevice));
  dout.ensure(nx * 2);
  launch_qkv_attn(dx.as<bf16>(), dw.as<bf16>(), db.as<float>(), dout.as<bf16>(), N, E.stream);
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  TTR_HIP_CHECK(hipMemcpy(h.data(), dout.p, nx * 2, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nx; ++i) { const uint32_t u = (uint32_t)h[i] << 16; memcpy(&out[i], &u, 4); }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_attn_enc(ttr_engine* e, const float* qkv, int N, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  const size_t nin = (size_t)N * 128 * 1152, nout = (size_t)N * 128 * 384;
  DevBuf din, dout;
  if (E.prec == kSplit) {   // attn_split.hip, as the encoder runs it behind a separate qkv GEMM: fp32 qkv -> exact triples -> the kernel -> triples joined here
    if (N <= 0) throw std::runtime_error("ttr_dbg_attn_enc: N >= 1");
    DevBuf dpl;
    din.ensure(nin * 4); dpl.ensure(nin * 6); dout.ensure(nout * 6);
    TTR_HIP_CHECK(hipMemcpy(din.p, qkv, nin * 4, hipMemcpyHostToDevice));
    launch_split_planes(din.as<float>(), 1152, dpl.p, (int64_t)N * 128, 1152, 0, E.stream, 3);
    launch_attn_enc_split(dpl.p, dout.p, N, E.stream);
    std::vector<_Float16> h(nout * 3);
    TTR_HIP_CHECK(hipMemcpyAsync(h.data(), dout.p, nout * 6, hipMemcpyDeviceToHost, E.stream));
    TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
    for (size_t m = 0; m < (size_t)N * 128; ++m)
      for (int c = 0; c < 384; ++c) {
        const _Float16* row = h.data() + m * 1152;
        out[m * 384 + c] = (float)((double)(float)row[c] + ((double)(float)row[384 + c] + (double)(float)row[768 + c]) / 2048.0);
      }
    return 0;
  }
  din.ensure(nin * E.es); dout.ensure(nout * E.es);
  if (E.prec == kBF16) {
    std::vector<uint16_t> h(nin);
    for (size_t i = 0; i < nin; ++i) h[i] = f32_to_bf16_rne(qkv[i]);
    TTR_HIP_CHECK(hipMemcpy(din.p, h.data(), nin * 2, hipMemcpyHostToDevice));
  } else TTR_HIP_CHECK(hipMemcpy(din.p, qkv, nin * 4, hipMemcpyHostToDevice));
  launch_attn_enc(E.prec, din.p, dout.p, N, E.stream);
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  if (E.prec == kBF16) {
    std::vector<uint16_t> h(nout);
    TTR_HIP_CHECK(hipMemcpy(h.data(), dout.p, nout * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nout; ++i) { const uint32_t u = (uint32_t)h[i] << 16; memcpy(&out[i], &u, 4); }
  } else TTR_HIP_CHECK(hipMemcpy(out, dout.p, nout * 4, hipMemcpyDeviceToHost));
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_cross_attn(ttr_engine* e, const float* q, const float* kvmem, int N, int R, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec == kBF16) throw std::runtime_error("ttr_dbg_cross_attn: split-operand / fp32 engines");
  if (N <= 0 || R <= 0) throw std::runtime_error("ttr_dbg_cross_attn: N, R >= 1");
  const size_t nq = (size_t)N * R * 384, nkv = (size_t)N * 128 * 768;
  DevBuf dq, dkv, dout;
  dq.ensure(nq * 4); dkv.ensure(nkv * 4); dout.ensure(nq * 6);
  TTR_HIP_CHECK(hipMemcpy(dq.p, q, nq * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(dkv.p, kvmem, nkv * 4, hipMemcpyHostToDevice));
  launch_dec_cross_attn(kF32, dq.p, dkv.p, dout.p, N, R, E.stream, nullptr, 0, nullptr, 0, 3);   // exact triples [N * R][3][384]
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  std::vector<_Float16> h(nq * 3);
  TTR_HIP_CHECK(hipMemcpy(h.data(), dout.p, nq * 6, hipMemcpyDeviceToHost));
  for (size_t r = 0; r < (size_t)N * R; ++r)
    for (int c = 0; c < 384; ++c)
      out[r * 384 + c] = (float)h[r * 1152 + c] + ((float)h[r * 1152 + 384 + c] + (float)h[r * 1152 + 768 + c]) * (1.f / 2048.f);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_dec_self_attn(ttr_engine* e, const float* q, const float* kvcache, const int32_t* tokens, int N, int R, int qi0, int mode, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec == kBF16) throw std::runtime_error("ttr_dbg_dec_self_attn: split-operand / fp32 engines");
  if (N <= 0 || (mode != 0 && mode != 1)) throw std::runtime_error("ttr_dbg_dec_self_attn: N >= 1, mode 0 or 1");
  if (mode == 0 ? (R != 1 || qi0 < 0 || qi0 > 25) : (R < 1 || R > 26)) throw std::runtime_error("ttr_dbg_dec_self_attn: mode 0 takes R = 1 and qi0 in 0 .. 25, mode 1 takes R in 1 .. 26");
  const int planes = E.prec == kSplit ? 3 : 0;   // what the engine's decoder hands its tail: exact triples on f16x4, fp32 rows on f32
  const size_t nq = (size_t)26 * 384, nkv = (size_t)N * 26 * 768, ntk = (size_t)N * 26, nout = (size_t)N * R * 384, out_bytes = nout * (planes ? 6 : 4);
  DevBuf dq, dkv, dtk, dout;
  dq.ensure(nq * 4); dkv.ensure(nkv * 4); dtk.ensure(ntk * 4); dout.ensure(out_bytes);
  TTR_HIP_CHECK(hipMemcpy(dq.p, q, nq * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(dkv.p, kvcache, nkv * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemcpy(dtk.p, tokens, ntk * 4, hipMemcpyHostToDevice));
  TTR_HIP_CHECK(hipMemsetAsync(dout.p, 0xFF, out_bytes, E.stream));   // a row the kernel leaves out comes back as NaN
  launch_dec_self_attn(E.prec, dq.as<float>(), dkv.p, dtk.as<int>(), dout.p, N, R, qi0, mode, E.stream, nullptr, 0, planes);   // no skip counter: every row is written
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  if (!planes) { TTR_HIP_CHECK(hipMemcpy(out, dout.p, nout * 4, hipMemcpyDeviceToHost)); return 0; }
  std::vector<_Float16> h(nout * 3);
  TTR_HIP_CHECK(hipMemcpy(h.data(), dout.p, out_bytes, hipMemcpyDeviceToHost));
  for (size_t r = 0; r < (size_t)N * R; ++r)
    for (int c = 0; c < 384; ++c)
      out[r * 384 + c] = (float)h[r * 1152 + c] + ((float)h[r * 1152 + 384 + c] + (float)h[r * 1152 + 768 + c]) * (1.f / 2048.f);   // split.h: join3
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_conv_pool(ttr_engine* e, const float* in0, int C0, int B, int H, int W, int ks, const float* wgt, const float* bias, int Cout, int act,
                      int pool_relu, float* out_full, float* out_pool) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec != kBF16) throw std::runtime_error("ttr_dbg_conv_pool: bf16 engines only (the fused pool lives in gemm2)");
  const size_t M = (size_t)B * H * W, Mp = M / 4;
  const int K = ks * ks * C0;
  DevBuf d0, dfull, dpool;
  Linear L;
  std::vector<uint16_t> hbuf(M * C0);
  for (size_t i = 0; i < hbuf.size(); ++i) hbuf[i] = f32_to_bf16_rne(in0[i]);
  d0.ensure(hbuf.size() * 2);
  TTR_HIP_CHECK(hipMemcpy(d0.p, hbuf.data(), hbuf.size() * 2, hipMemcpyHostToDevice));
  E.upload_linear(L, wgt, Cout, K, bias, Cout, K, nullptr, false);
  dfull.ensure(M * Cout * 2); dpool.ensure(Mp * Cout * 2);
  ConvParams p{};
  p.in0 = d0.p; p.C0 = C0; p.B = B; p.H = H; p.W = W; p.ks = ks; p.dil = 1; p.wgt = L.w.p; p.bias = bias ? L.b.as<float>() : nullptr;
  p.out = out_full ? dfull.p : nullptr; p.out_ld = Cout; p.out_pool = dpool.p; p.pool_relu = pool_relu;
  p.Cout = Cout; p.M = (int)M; p.act = act;
  launch_igemm(E.prec, p, E.stream);
  auto down = [&](const DevBuf& d, size_t n, float* dst) {
    std::vector<uint16_t> h(n);
    TTR_HIP_CHECK(hipMemcpyAsync(h.data(), d.p, n * 2, hipMemcpyDeviceToHost, E.stream));
    TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
    for (size_t i = 0; i < n; ++i) { uint32_t u = (uint32_t)h[i] << 16; memcpy(&dst[i], &u, 4); }
  };
  if (out_full) down(dfull, M * Cout, out_full);
  down(dpool, Mp * Cout, out_pool);
  return 0;
  TTR_GUARD_END(-1)
}

// The tap on the split detector (engine.h: Engine::CraftTap): one forward pass of B canvases with the switch on, then the records and their tensors.
int ttr_dbg_craft_taps(ttr_engine* e, const uint8_t* canvas, int B, int H, int W, float* heat_out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_craft_taps");
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_craft_taps: f16x4 engines only");
  if (B < 1 || H < 32 || W < 32) throw std::runtime_error("ttr_dbg_craft_taps: B >= 1, H, W >= 32");
  const size_t nc = (size_t)B * H * W * 3, nh = (size_t)B * H * W / 4 * 2;
  E.canvas.ensure(nc);
  E.heat.ensure(nh * 4);
  TTR_HIP_CHECK(hipMemcpyAsync(E.canvas.p, canvas, nc, hipMemcpyHostToDevice, E.stream));
  struct Off { Engine& E; ~Off() { E.craft_tap_on = false; } } off{E};
  E.craft_tap_on = true;
  E.craft_forward(E.canvas.as<uint8_t>(), B, H, W, E.heat.as<float>());
  if (heat_out) TTR_HIP_CHECK(hipMemcpyAsync(heat_out, E.heat.p, nh * 4, hipMemcpyDeviceToHost, E.stream));
  E.range_fetch(Engine::kRangeStage);
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  E.range_verify(Engine::kRangeStage, "ttr_dbg_craft_taps");
  return (int)E.craft_taps.size();
  TTR_GUARD_END(-1)
}

int ttr_dbg_craft_tap_count(ttr_engine* e) { return e ? (int)e->e->craft_taps.size() : -1; }

// (list 0: craft_taps, the pass's layers; list 1: craft_fold_taps, the folded upconv1.0 launches of a tapped pass with fc7_fold on)
static int craft_tap_info(ttr_engine* e, int list, int i, char* text, size_t cap, int dims[7]) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  const std::vector<Engine::CraftTap>& taps = list ? E.craft_fold_taps : E.craft_taps;
  if (i < 0 || i >= (int)taps.size()) throw std::runtime_error("ttr_dbg_craft_tap_info: no such record");
  const Engine::CraftTap& t = taps[i];
  const std::string s = t.layer + "\n" + t.role + "\n" + t.kind;
  if (!text || cap < s.size() + 1) throw std::runtime_error("ttr_dbg_craft_tap_info: text buffer too small");
  memcpy(text, s.c_str(), s.size() + 1);
  dims[0] = t.B; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; dims[4] = t.ld; dims[5] = t.form;
  dims[6] = t.form == Engine::kTapTriples ? 3 : t.form == Engine::kTapPairs || t.form == Engine::kTapPacked ? 2 : 0;   // f16 planes per value
  return 0;
  TTR_GUARD_END(-1)
}

static int craft_tap_read(ttr_engine* e, int list, int i, float* out) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  const std::vector<Engine::CraftTap>& taps = list ? E.craft_fold_taps : E.craft_taps;
  if (i < 0 || i >= (int)taps.size()) throw std::runtime_error("ttr_dbg_craft_tap_read: no such record");
  const Engine::CraftTap& t = taps[i];
  const size_t M = (size_t)t.B * t.H * t.W, ld = (size_t)t.ld;
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  if (t.form == Engine::kTapF32) { TTR_HIP_CHECK(hipMemcpy(out, t.p, M * ld * 4, hipMemcpyDeviceToHost)); return 0; }
  if (t.form == Engine::kTapU8) {
    std::vector<uint8_t> h(M * ld);
    TTR_HIP_CHECK(hipMemcpy(h.data(), t.p, h.size(), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < h.size(); ++j) out[j] = (float)h[j];
    return 0;
  }
  const size_t npl = t.form == Engine::kTapTriples ? 3 : 2;   // pixel row [x0 (ld) | x1 (ld) (| x2 (ld))]; packed pairs are that row with ld = 32
  std::vector<_Float16> h(M * npl * ld);
  TTR_HIP_CHECK(hipMemcpy(h.data(), t.p, h.size() * 2, hipMemcpyDeviceToHost));
  for (size_t m = 0; m < M; ++m) {
    const _Float16* row = h.data() + m * npl * ld;
    float* o = out + m * ld;
    if (npl == 3) for (size_t c = 0; c < ld; ++c) o[c] = (float)row[c] + ((float)row[ld + c] + (float)row[2 * ld + c]) * (1.f / 2048.f);   // split.h: join3, every step exact
    else for (size_t c = 0; c < ld; ++c) o[c] = (float)row[c] + (float)row[ld + c] * (1.f / 2048.f);                                       // join2
  }
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_craft_tap_info(ttr_engine* e, int i, char* text, size_t cap, int dims[7]) { return craft_tap_info(e, 0, i, text, cap, dims); }
int ttr_dbg_craft_tap_read(ttr_engine* e, int i, float* out) { return craft_tap_read(e, 0, i, out); }
int ttr_dbg_craft_fold_tap_count(ttr_engine* e) { return e ? (int)e->e->craft_fold_taps.size() : -1; }
int ttr_dbg_craft_fold_tap_info(ttr_engine* e, int i, char* text, size_t cap, int dims[7]) { return craft_tap_info(e, 1, i, text, cap, dims); }
int ttr_dbg_craft_fold_tap_read(ttr_engine* e, int i, float* out) { return craft_tap_read(e, 1, i, out); }

void ttr_set_gemm_config(int cfg) { set_gemm_config(cfg); }

void ttr_set_decoder_mode(int mode) { g_tuning_default.decoder_mode = mode; }

void ttr_last_host_us(ttr_engine* e, float out[8]) { for (int i = 0; i < 8; ++i) out[i] = e ? e->e->host_us[i] : 0.f; }

int ttr_dbg_dec_stamps_ext(unsigned long long* out, int n) { return g_dec_dbg && n >= 0 && n <= 4096 && hipMemcpy(out, g_dec_dbg, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }
int ttr_dbg_dec_stamps(unsigned long long* out) { return g_dec_dbg && hipMemcpy(out, g_dec_dbg, 26 * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }

// process-wide: the kernel files' variant switches and diagnostics; engine-level keys set the default of engines created afterwards
int ttr_set_tuning(const char* key, int value) {
  const std::string k = key ? key : "";
  if (g_tuning_default.set(k, value)) return 0;
  if (k == "gemm_config") set_gemm_config(value);
  else if (k == "self_refine") set_dec_self_refine(value);
  else if (k == "cross_mfma") set_dec_cross_mfma(value);
  else if (k == "cross_crop") set_dec_cross_crop(value);
  else if (k == "cross_split") set_dec_cross_split(value);
  else if (k == "cross_rows_hsplit") set_dec_cross_rows_hsplit(value);
  else if (k == "mlp_store_nt") set_mlp_store_nt(value);
  else if (k == "mlp_stagger") set_mlp_stagger(value);
  else if (k == "c3s_wgs") set_conv3s_wgs_per_cu(value);
  else if (k == "c3_c32") set_conv3p_c32_tile(value);
  else if (k == "c3_narrow64") set_conv3p_narrow_bn64(value);
  else if (k == "upsample_block") set_upsample_block(value);
  else if (k == "mlp_ablate") set_mlp_ablate(value);
  else if (k == "attn_impl") set_attn_impl(value);
  else if (k == "ws_dbg_flags") set_gemm_ws_dbg_flags(value);
  else if (k == "ws_lean") set_gemm_ws_lean(value);
  else if (k == "store_policy") set_store_policy(value);
  else if (k == "head_persistent") set_conv3p_head_persistent(value);
  else if (k == "up_resident") set_gemm2_up_resident(value);
  else if (k == "up_2d") set_gemm2_up_2d(value);
  else if (k == "c3h_wgs_per_cu") set_conv3h_wgs_per_cu(value);
  else if (k == "g2_x_ring3") set_gemm2_x_ring3(value);
  else if (k == "g2_split_reuse") set_gemm2_split_reuse(value);
  else if (k == "g2_split_cfg") set_gemm2_split_cfg(value);
  else if (k == "g2_split_few") set_gemm2_split_few(value);
  else if (k == "g2_split_dbg") set_gemm2_split_dbg(value);
  else if (k == "g2_split_wreg") set_gemm2_split_wreg(value);
  else if (k == "g2_split_stream") set_gemm2_split_stream(value);
  else if (k == "g2_split_stream4") set_gemm2_split_stream4(value);
  else if (k == "gsp_sched") set_gemm_sp_sched(value);
  else if (k == "gsp_few") set_gemm_sp_few(value);
  else if (k == "gsp_epi") set_gemm_sp_epi(value);
  else if (k == "gsp_ks3") set_gemm_sp_ks3(value);
  else if (k == "gsp_stagger") set_gemm_sp_stagger(value);
  else if (k == "gsp_dbg") set_gemm_sp_dbg(value);
  else if (k == "gsp_stag") set_gemm_sp_stag(value);
  else if (k == "gsp_stagger_groups") set_gemm_sp_stagger_groups(value);
  else if (k == "qkv_attn_dbg") set_qkv_attn_dbg(value);
  else if (k == "qkv_attn4") set_qkv_attn4(value);
  else if (k == "skx_ln_max_rows") set_gemm_skx_ln_max_rows(value);
  else if (k == "c3_xs1_max_cin") set_conv3p_single_stage_max_cin(value);
  else if (k == "c3_force_bn128") set_conv3p_force_bn128(value);
  else if (k == "c3_c64_waves") set_conv3p_c64_waves(value);
  else if (k == "c3_c128_waves") set_conv3p_c128_waves(value);
  else if (k == "c3_narrow_wide") set_conv3p_narrow_wide(value);
  else if (k == "c3_narrow_frac") set_conv3p_narrow_frac(value);
  else if (k == "c3_narrowest_frac") set_conv3p_narrowest_frac(value);
  else if (k == "c3_deep_w") set_conv3p_deep_w(value);
  else if (k == "c3_deep_w64") set_conv3p_deep_w64(value);
  else if (k == "c3_first_persistent") set_conv3p_first_persistent(value);
  else if (k == "sk_max_rows") set_skinny_max_rows(value);
  else if (k == "ws_min_rows") set_gemm_ws_min_rows(value);
  else if (k == "dec_stamps") {   // value != 0: allocate the stamp buffer; read it back with ttr_dev_download via ttr_dbg_dec_stamps
    if (value && !g_dec_dbg) { void* d = nullptr; if (hipMalloc(&d, 4096 * 8) != hipSuccess) return -1; (void)hipMemset(d, 0, 4096 * 8); g_dec_dbg = (unsigned long long*)d; }
    if (!value) g_dec_dbg = nullptr;
    set_gemm_ws_stamps(value == 2 ? g_dec_dbg : nullptr);
    set_conv3p_stamps(value == 4 ? g_dec_dbg : nullptr);    // 4: ... or conv3p_first2 stamps
    set_mlp_stamps(value == 3 ? g_dec_dbg : nullptr);
    set_qkv_attn_stamps(value == 5 ? g_dec_dbg : nullptr);
    set_qkv_attn4_stamps(value == 5 ? g_dec_dbg : nullptr);   // 5: ... or the fused qkv + attention launch's
    set_conv3h_stamps(value == 6 ? g_dec_dbg : nullptr);     // 6: ... or the persistent head kernel's (conv3h.hip)
    // 3: ... or mlp_fused stamps   // 2: the same buffer takes gemm_ws stamps instead
  }
  else return -1;
  return 0;
}

// per engine (under the engine's lock: a batch in flight on another thread keeps the selection it started with)
int ttr_engine_set_tuning(ttr_engine* e, const char* key, int value) {
  TTR_GUARD_BEGIN
  if (!e) return -1;
  const std::string k = key ? key : "";
  {
    std::lock_guard<std::mutex> lk(e->e->mu);
    if (e->e->tn.set(k, value)) return 0;
  }
  return ttr_set_tuning(key, value);   // not an engine key: the process-wide diagnostics setter (documented in tuatara_hip.h)
  TTR_GUARD_END(-1)
}

int ttr_bench_conv(ttr_engine* e, int B, int H, int W, int C0, int C1, int ks, int dil, int Cout, int act, int f32_resid, int iters, float* avg_us) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  const size_t M = (size_t)B * H * W;
  const int K = ks * ks * (C0 + C1);
  DevBuf d0, d1, dw, db, dout, dres;
  d0.ensure(M * C0 * E.es); launch_fill_random(E.prec, d0.p, M * C0, 1u, 1.0f, E.stream);
  if (C1) { d1.ensure(M * C1 * E.es); launch_fill_random(E.prec, d1.p, M * C1, 2u, 1.0f, E.stream); }
  dw.ensure((size_t)Cout * K * E.es); launch_fill_random(E.prec, dw.p, (size_t)Cout * K, 3u, 1.0f / std::sqrt((float)K), E.stream);
  db.ensure((size_t)Cout * 4); launch_fill_random(kF32, db.p, Cout, 4u, 1.0f, E.stream);
  ConvParams p{};
  p.in0 = d0.p; p.C0 = C0; p.in1 = C1 ? d1.p : nullptr; p.C1 = C1;
  p.B = B; p.H = H; p.W = W; p.ks = ks; p.dil = dil; p.wgt = dw.p; p.bias = db.as<float>();
  p.Cout = Cout; p.M = (int)M; p.act = act;
  if (f32_resid) {   // the PARSeq residual-stream form: f32 in, f32 out
    dres.ensure(M * Cout * 4); launch_fill_random(kF32, dres.p, M * Cout, 5u, 1.0f, E.stream);
    p.out_f32 = dres.as<float>(); p.out_f32_ld = Cout; p.resid = dres.as<float>(); p.resid_ld = Cout;
  } else {
    dout.ensure(M * Cout * E.es); p.out = dout.p; p.out_ld = Cout;
  }
  for (int i = 0; i < 2; ++i) launch_igemm(E.prec, p, E.stream);
  hipEvent_t a, b;
  TTR_HIP_CHECK(hipEventCreate(&a)); TTR_HIP_CHECK(hipEventCreate(&b));
  TTR_HIP_CHECK(hipEventRecord(a, E.stream));
  for (int i = 0; i < iters; ++i) launch_igemm(E.prec, p, E.stream);
  TTR_HIP_CHECK(hipEventRecord(b, E.stream));
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  float ms = 0.f;
  TTR_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  *avg_us = ms * 1e3f / iters;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_min_area_rect(const float* xy, int n, float* r5) {
  TTR_GUARD_BEGIN
  std::vector<Pt2f> p(n);
  for (int i = 0; i < n; ++i) p[i] = Pt2f{xy[2 * i], xy[2 * i + 1]};
  RRect r = min_area_rect(p.data(), n);
  r5[0] = r.cx; r5[1] = r.cy; r5[2] = r.w; r5[3] = r.h; r5[4] = r.angle;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_component_rect(int area, int x0, int y0, int x1, int y1, const int32_t* rows, int H, int W, float* r5) {
  TTR_GUARD_BEGIN
  Component c{0, area, x0, y0, x1, y1, rows};
  RRect r;
  if (!component_to_rect(c, H, W, &r)) return 0;
  r5[0] = r.cx; r5[1] = r.cy; r5[2] = r.w; r5[3] = r.h; r5[4] = r.angle;
  return 1;
  TTR_GUARD_END(-1)
}

int ttr_dbg_box_geometry(const float* r5, float ratio, float* adj5, int32_t* xywh, float* bbox4) {
  TTR_GUARD_BEGIN
  RRect r{r5[0], r5[1], r5[2], r5[3], r5[4]};
  RRect b = adjust_coordinates(r, 1.f / ratio, 1.f / ratio);
  adj5[0] = b.cx; adj5[1] = b.cy; adj5[2] = b.w; adj5[3] = b.h; adj5[4] = b.angle;
  int q[4];
  bounding_rect(b, q);
  for (int i = 0; i < 4; ++i) xywh[i] = q[i];
  tesseract_bbox(b, bbox4);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_deskew(const float* r5, float* quad8, double* coef6, int64_t* fixed6) {
  TTR_GUARD_BEGIN
  const RRect r{r5[0], r5[1], r5[2], r5[3], r5[4]};
  Pt2f q[4];
  const int kind = deskew_quad(r, q, coef6);
  deskew_fixed(coef6, fixed6);
  for (int k = 0; k < 4; ++k) { quad8[2 * k] = q[k].x; quad8[2 * k + 1] = q[k].y; }
  return kind;
  TTR_GUARD_END(-1)
}

int ttr_dbg_canvas_geometry(int h, int w, int canvas_size, float mag_ratio, int* H, int* W, float* ratio, int* target_h, int* target_w) {
  if (h <= 0 || w <= 0) return -1;
  const CanvasGeom g = canvas_geometry(h, w, canvas_size, mag_ratio);
  if (H) *H = g.h32;
  if (W) *W = g.w32;
  if (ratio) *ratio = g.ratio;
  if (target_h) *target_h = g.target_h;
  if (target_w) *target_w = g.target_w;
  return 0;
}

int ttr_dbg_launch_groups(int H, int W, int n_pages, int n_crops, int craft_group, int first_fused, int craft_products, int up_commute, int enc_chunk,
                          int enc_fc2_pairs, int qkv_attn_split, int enc_ln_pairs, int sp_hidden16, int* craft_pages, int* enc_crops, int64_t* page_bytes,
                          int64_t* crop_bytes) {
  if (H <= 0 || W <= 0 || H % 32 || W % 32 || n_pages < 1 || n_crops < 1 || craft_group < 1) return -1;
  const int products = craft_products == 4 ? 4 : 3;
  const CraftGroupCfg cc{first_fused && products != 4 ? 1 : 0, products, up_commute};
  const EncGroupCfg ec{enc_fc2_pairs, qkv_attn_split, enc_ln_pairs, sp_hidden16};
  if (craft_pages) *craft_pages = craft_group_pages(H, W, n_pages, std::min(craft_group, 32), cc);
  if (enc_crops) *enc_crops = encoder_group_crops(n_crops, enc_chunk, ec);
  if (page_bytes) *page_bytes = (int64_t)craft_widest_per_page(H, W, cc).bytes;
  if (crop_bytes) *crop_bytes = (int64_t)encoder_bytes_per_crop(ec).widest().bytes;
  return 0;
}

int ttr_dbg_split_layer_check(int kernel, int B, int H, int W, int C0, int Cout, int ks, int products, int out_planes, int pooled, char* text, size_t cap) {
  if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > 0x7fffffff || (products != 3 && products != 4)) return -1;
  ConvParams p{};
  void* const any = reinterpret_cast<void*>((uintptr_t)4096);   // (aligned and never dereferenced: the checks read shapes and alignments only)
  p.in0 = any; p.C0 = C0; p.B = B; p.H = H; p.W = W; p.ks = ks; p.dil = 1;
  p.wgt = any; p.bias = reinterpret_cast<const float*>(any); p.split = products; p.out_scale = 1.f; p.out_planes = out_planes;
  p.out = any; p.out_ld = Cout; p.out_pool = pooled ? any : nullptr; p.Cout = Cout; p.M = B * H * W; p.act = kActRelu;
  if (kernel == 2) { p.pre_wgt = any; p.pre_bias = reinterpret_cast<const float*>(any); p.pre_scale = 1.f; p.out = nullptr; p.out_pool = any; }   // conv1_1 fused in front: in0 is the u8 canvas
  const char* e = kernel == 1 ? gemm2_check(p) : conv3p_check(p);
  if (text && cap) { const std::string s = e ? e : ""; memcpy(text, s.c_str(), std::min(cap - 1, s.size())); text[std::min(cap - 1, s.size())] = 0; }
  return e ? 1 : 0;
}

int ttr_dbg_last_groups(ttr_engine* e, int* craft_pages, int* enc_crops) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  if (craft_pages) *craft_pages = E.last_craft_group;
  if (enc_crops) *enc_crops = E.last_enc_group;
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_last_heat(ttr_engine* e, float* heat, size_t floats) {
  TTR_GUARD_BEGIN
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_last_heat");
  if (!heat || floats == 0 || floats * 4 > E.heat.cap) throw std::runtime_error("ttr_dbg_last_heat: more floats than the last batch's heat maps hold");
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  TTR_HIP_CHECK(hipMemcpy(heat, E.heat.p, floats * 4, hipMemcpyDeviceToHost));
  return 0;
  TTR_GUARD_END(-1)
}

// ---- the device buffers' table (engine.h: kDevBufTable) as text, and the poison over its scratch rows
static const char* buf_kind_name(BufKind k) { return k == kElF32 ? "f32" : k == kElF16 ? "f16" : k == kElU8 ? "u8" : k == kElI32 ? "i32" : "addr"; }

int ttr_dbg_scratch_table(char* text, size_t cap) {
  TTR_GUARD_BEGIN
  std::string s;
  for (const BufRow& r : kDevBufTable) {
    s += std::string(r.name) + " " + (r.kept ? "kept" : "scratch") + " " + buf_kind_name(r.kind);
    if (r.note[0]) s += std::string(" ") + r.note;
    s += "\n";
  }
  if (text && cap) { const size_t n = std::min(cap - 1, s.size()); memcpy(text, s.data(), n); text[n] = 0; }
  return (int)s.size();
  TTR_GUARD_END(-1)
}

int64_t ttr_dbg_poison_scratch(ttr_engine* e, int pattern, int also_kept_once) {
  TTR_GUARD_BEGIN
  if (!e) throw std::runtime_error("null argument");
  if (pattern < 0 || pattern > 2) throw std::runtime_error("ttr_dbg_poison_scratch: pattern must be 0 (zeros), 1 (quiet NaN) or 2 (large finite)");
  Engine& E = *e->e;
  EngineScope lk(E);
  if (E.prec != kSplit) throw std::runtime_error("ttr_dbg_poison_scratch: an f16x4 engine only (the table's kinds are that engine's)");
  E.refuse_while_streaming("ttr_dbg_poison_scratch");
  for (hipStream_t st : {E.stream, E.recog_stream, E.lane_stream, E.copy_stream, E.up_stream}) if (st) TTR_HIP_CHECK(hipStreamSynchronize(st));
  static const uint32_t v32[3] = {0u, 0x7FC00000u, 0x461C4000u};   // 0, quiet NaN, 1e4
  static const uint16_t v16[3] = {0, 0x7E00, 0x7000};              // 0, quiet NaN, 8192
  static const uint8_t v8[3] = {0, 0xA5, 0x5A};
  size_t filled = 0;
  auto fill = [&](DevBuf& d, BufKind kind) {
    if (!d.p || !d.cap || kind == kElAddr) return;   // (capacities are whole MiB: every element width divides them)
    if (kind == kElF32) TTR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d.p, (int)v32[pattern], d.cap / 4, E.stream));
    else if (kind == kElF16) TTR_HIP_CHECK(hipMemsetD16Async((hipDeviceptr_t)d.p, v16[pattern], d.cap / 2, E.stream));
    else if (kind == kElU8) TTR_HIP_CHECK(hipMemsetD8Async((hipDeviceptr_t)d.p, v8[pattern], d.cap, E.stream));
    else TTR_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)d.p, 0, d.cap / 4, E.stream));
    filled += d.cap;
  };
  std::vector<std::string> seen;
  size_t craft_slot = 0; int craft_set = 0, pq_slot = 0;
  E.for_scratch([&](const char* name, DevBuf& d, BufKind kind) {
    if (seen.empty() || seen.back() != name) seen.push_back(name);
    if (!strcmp(name, "craft_ws_set")) {   // the slot's own kind, and the write-once slots only on request
      while (craft_set < 2 && craft_slot >= E.craft_ws_set[craft_set].size()) { ++craft_set; craft_slot = 0; }
      const auto& meta = E.craft_ws_meta[craft_set];
      const uint8_t m = craft_slot < meta.size() ? meta[craft_slot] : (uint8_t)kElF16;
      ++craft_slot;
      if ((m & Engine::kWsZeroedOnce) && !also_kept_once) return;
      kind = (BufKind)(m & Engine::kWsKindMask);
    } else if (!strcmp(name, "pq_ws")) {
      const int i = pq_slot++;
      if (i == Engine::kWsKvcache && !also_kept_once) return;
      kind = i >= Engine::kWsLnPlanes ? kElF16 : kElF32;
    }
    fill(d, kind);
  });
  // the visit and the table must name the same scratch rows, in the same order
  std::vector<std::string> want;
  const bool no_craft = E.craft_ws_set[0].empty() && E.craft_ws_set[1].empty();   // (before the first detector pass the sets hold no slot to visit)
  for (const BufRow& r : kDevBufTable)
    if (!r.kept && (E.comm || strncmp(r.name, "comm.", 5) != 0) && !(no_craft && !strcmp(r.name, "craft_ws_set"))) want.push_back(r.name);
  if (seen != want) throw std::logic_error("ttr_dbg_poison_scratch: Engine::for_scratch and kDevBufTable name different scratch buffers");
  TTR_HIP_CHECK(hipStreamSynchronize(E.stream));
  return (int64_t)filled;
  TTR_GUARD_END(-1)
}

// tables (DESIGN.md "Tables"): the ink bitmap and the run lists as the device formed them
int ttr_dbg_tables(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_len, int ink, uint64_t* bits, int32_t* runs,
                   int32_t* n_runs, int32_t* mode) {
  TTR_GUARD_BEGIN
  if (!e || !img) throw std::runtime_error("null argument");
  if (h <= 0 || w <= 0 || (row_stride && row_stride < w * 3)) throw std::runtime_error("ttr_dbg_tables: bad image size");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_tables");
  std::vector<int32_t> side(kTabSideInts);
  E.tables_stage(img, h, w, row_stride, dev_offset, dev_stride, min_len, ink, nullptr, 0, side.data(), nullptr, bits, runs);
  if (n_runs) { n_runs[0] = side[5]; n_runs[1] = side[6]; }
  if (mode) *mode = side[0];
  return 0;
  TTR_GUARD_END(-1)
}

// deskew (DESIGN.md "Deskew"): the stage call with the image placed anywhere in a device buffer
int ttr_dbg_deskew_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int max_slope, int gain, int ink, uint8_t* out_img,
                   ttr_skew* rec, uint64_t* scores) {
  TTR_GUARD_BEGIN
  if (!e || !img) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_deskew_page");
  DeskewRec r;
  E.deskew_stage(img, h, w, row_stride, dev_offset, dev_stride, max_slope, gain, ink, out_img, &r, scores);
  if (rec) memcpy(rec, &r, sizeof r);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_ink_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int radius, int drop, int polarity, uint64_t* bits,
                     uint64_t* bitsT, ttr_ink* rec) {
  TTR_GUARD_BEGIN
  if (!e || !img) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_ink_page");
  InkRec r;
  E.ink_stage(img, h, w, row_stride, dev_offset, dev_stride, radius, drop, polarity, bits, bitsT, &r);
  if (rec) memcpy(rec, &r, sizeof r);
  return 0;
  TTR_GUARD_END(-1)
}

int64_t ttr_dbg_page_ink_passes(const ttr_engine* e) { return e ? e->e->page_ink_passes : -1; }

// barcodes (DESIGN.md "Barcodes"): the lines' raw hits and counters as the device formed them
int ttr_dbg_barcodes(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_lines, int ink, int symbologies, int32_t* hits,
                     int32_t* line_counts, int32_t* side_out) {
  TTR_GUARD_BEGIN
  if (!e || !img) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_barcodes");
  E.barcodes_stage(img, h, w, row_stride, dev_offset, dev_stride, min_lines, ink, symbologies, nullptr, 0, side_out, nullptr, hits, line_counts);
  return 0;
  TTR_GUARD_END(-1)
}

// selection marks (DESIGN.md "Selection marks"): the corner count and the band counts as the device formed them
int ttr_dbg_marks(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_side, int max_side, int fill, int ink,
                  int32_t* corners, int32_t* band_counts, int32_t* mode, int32_t* marks) {
  TTR_GUARD_BEGIN
  if (!e || !img) throw std::runtime_error("null argument");
  Engine& E = *e->e;
  EngineScope lk(E);
  E.refuse_while_streaming("ttr_dbg_marks");
  std::vector<int32_t> side(kMarkSideInts);
  E.marks_stage(img, h, w, row_stride, dev_offset, dev_stride, min_side, max_side, fill, ink, nullptr, 0, side.data(), nullptr, band_counts);
  if (corners) *corners = side[2];
  if (mode) *mode = side[0];
  if (marks) std::copy(side.begin() + kMarkHdr, side.end(), marks);
  return 0;
  TTR_GUARD_END(-1)
}

int ttr_dbg_orient_quad(const float* r5, int h, int w, int crop_mode, int turn, float* quad8, int64_t* fixed6) {
  TTR_GUARD_BEGIN
  if (turn < 0 || turn > 3 || (crop_mode != TTR_CROP_BOUNDING && crop_mode != TTR_CROP_RECTIFIED)) throw std::runtime_error("bad turn or crop_mode");
  const RRect r{r5[0], r5[1], r5[2], r5[3], r5[4]};
  Pt2f q[4]; double cf[6];
  deskew_quad(r, q, cf);
  if (crop_mode == TTR_CROP_BOUNDING) {
    int xywh[4];
    bounding_rect(r, xywh);
    box_edge_quad(std::max(xywh[0], 0), std::max(xywh[1], 0), std::min(xywh[0] + xywh[2], w), std::min(xywh[1] + xywh[3], h), q);
  }
  turn_coef(q, turn, fixed6);
  for (int k = 0; k < 4; ++k) { quad8[2 * k] = q[(k + turn) & 3].x; quad8[2 * k + 1] = q[(k + turn) & 3].y; }
  return 0;
  TTR_GUARD_END(-1)
}

}  // extern "C"
