// The engine of the MI355X-native tuatara hot path: declarations shared by its translation units.
//   engine.cpp          construction, weights -> device, workspaces, per-launch profile
//   engine_craft.cpp    the detector's forward pass (tuatara.cpp:363-394)
//   engine_parseq.cpp   the recogniser's forward pass (tuatara.cpp:307, :450-485)
//   engine_pages.cpp    image_to_data over batches of pages: detect / collect / recognise / finish, streamed batches, the sharded latency mode
//   comm.cpp            transports (RCCL, framed TCP), rendezvous, the ttr_comm_* entry points
//   capi.cpp            the C ABI of include/tuatara_hip.h;  capi_debug.cpp: the developer hooks of include/tuatara_hip_debug.h
//
// Re-implements the reference's pipeline function image_to_data (tuatara.cpp:314-512):
//   resize/pad/swap (:349-358) -> CRAFT (:363-394) -> get_detected_boxes (:400) ->
//   adjust_result_coordinates (:406) -> crop (:408-418) -> resize 128x32 (:436-448) ->
//   PARSeq (:450-485) -> argmax + Tokenizer (:486-505) -> format_output (:511)
// with every tensor op on the GPU (igemm.hip, craft_ops.hip, parseq_ops.hip, post_ops.hip)
// and only the per-component calipers + string decoding on the host (geometry.cpp).
// Differences by design: models are loaded once per engine (the reference reloads both
// per call, :336, :428), crops of all pages of a batch run as one PARSeq batch (the
// reference chunks by 4 over 6 threads, :452-475; logits are batch-invariant), the AR
// decoder keeps a K/V cache and leaves its loop once every crop has emitted EOS, like upstream PARSeq.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <chrono>
#include <dlfcn.h>
#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <atomic>
#include <functional>
#include <condition_variable>
#include <thread>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/tuatara_hip_debug.h"
#include "common.h"
#include "deskew_rule.h"
#include "ink_rule.h"
#include "geometry.h"
#include "host_util.h"
#include "kernels.h"
#include "pattern.h"

namespace ttr {


extern thread_local std::string g_last_error;   // capi.cpp
extern unsigned long long* g_dec_dbg;   // device buffer for dec_ar phase stamps (diagnostics; engine_parseq.cpp)
// Kernel-selection knobs, per engine (ttr_engine_set_tuning); g_tuning_default seeds engines created afterwards (ttr_set_tuning)
struct Tuning {
  int dbg_bf16_out = 0;       // ttr_dbg_conv on a bf16 engine: take the kernel's bf16 output (the path the engine uses) instead of the f32 one
  int qkv_attn = 1;           // bf16 encoder: qkv projection + self-attention as one kernel (qkv_attn.hip) from qkv_attn_min crops on
  int qkv_attn_min = 160;
  int mlp_proj = 1;           // ... with the attention output projection in front of it in the same launch
  int mlp_min_rows = 49152;   // = 384 crops
  int dec_mlp_fused = 1;      // bf16 refinement pass: cross_out + norm2 + linear1 + GELU + linear2 + final norm through mlp_fused.hip
  int dec_mlp_min_rows = 16384;
  int mlp_fused = 1;          // bf16 encoder: norm2 + fc1 + GELU + fc2 + residual (+ the next LayerNorm) as one kernel (mlp_fused.hip)
  int tok_fuse = 1;           // bf16 AR steps: argmax of the previous step + token embedding + norm_c inside the self_kv skinny GEMM
  int ln_fuse = 1;            // bf16 decoder steps: LayerNorm computed inside the skinny GEMM's loader (gemm_sk ln_in)
  int fuse_first = 1;         // bf16: CRAFT conv1_1 fused into conv1_2's loader (conv3p FIRST)
  int qkv_attn_split = 1;     // split-operand engines, PARSeq encoder: qkv projection + self-attention as ONE launch (gemm_sp.hip, attention epilogue); needs enc_ln_pairs
  int skinny_split = 1;       // split-operand engines: linears of <= skinny_max_rows rows (the AR steps: one row per crop) on gemm_skx.hip
  int skinny_max_rows = 2048;
  int skx_ln_fuse = 1;        // split engines, <= 256 rows: the decoder's LayerNorm + linear pairs as one skinny launch (gemm_skx.hip, LayerNorm prologue)
  int embed_fold = 1;         // split engines, <= 256 crops: an AR step's embedding + norm_c inside its self_kv linear (gemm_skx.hip, token prologue)
  int argmax_fold = 1;        // split engines: an AR step's argmax inside the next step's embedding kernel (one dependent launch less per step)
  int sp_tiled_x = 1;         // ... and the encoder's activation planes (LayerNorm outputs, attention output, MLP hidden) are written and read as such pieces
  int sp_tiled_w = 1;         // split engines: gemm_sp.hip reads the recogniser's weight planes as contiguous 1-KiB pieces (Linear::wst)
  int ar_host_check = 10;     // split / fp32 engines, batches of <= 256 crops (the latency regime): from this AR step on the host looks at the done counter every fourth
                              // step and stops enqueuing steps once every crop has emitted EOS (upstream's loop does that check every step); 0 = never
  int enc_chunk = 0;          // crops per encoder group, at most.  f16x4: capped by what the widest tensor of the configuration allows inside the 2 GiB window
                              // (encoder_group_crops below: 2730 on the default path), 0 = 1820 (kEncGroupDefault: 2560 crops = 1280 + 1280; enc_chunk = 4096 runs them
                              // as one group).  bf16 / f32: 0 = all crops at once
  int enc_ln_pairs = 1;       // split-operand engines, PARSeq encoder: LayerNorm outputs as pairs (qkv and fc1 on three MFMAs per product: their inputs tolerate ~23.5 bits - 3 x 1280 crops: max |dlogit| 7.6e-4 vs 6.9e-4 with triples; proj and fc2 keep exact triples); 0 = triples
  int dec_planes = 1;         // split-operand engines: the decoder's layers hand each other planes (13 launches per AR step instead of 20); 0 = fp32 tensors + split passes
  int qkv_kv_pairs = 1;       // the qkv GEMM leaves the third plane of its K and V columns unwritten (the attention kernel reads them as pairs)
  int enc_fc2_pairs = 1;      // ... and the MLP hidden activation as pairs (fc2 on three MFMAs per product; 3 x 640 crops: max |dlogit| 5.1 - 6.7e-4 vs 5.6 - 7.6e-4 with triples); the attention output - the projection input - stays an exact triple: the one encoder linear whose result moves with the 24th bit (oracle/splitsim.py)
  int craft_products = 3;     // split-operand engines, CRAFT: 3 = activation pairs (~23.5 bits; the heat map stays at fp32 noise level), 4 = exact triples
  int gpu_calipers = 1;       // get_detected_boxes' per-component tail (dilated extremes -> hull -> minAreaRect, tuatara.cpp:162-179) on the GPU (post_ops.hip: ccl_rects_kernel);
                              // the host then reads 24 bytes per candidate instead of its row extremes and runs no calipers; 0 = geometry.cpp on the host
  int up_commute = 1;         // split engines, CRAFT's upconv2.0 / 3.0 / 4.0 (1x1 over cat(upsample(y), skip)): W_up . y at the low resolution, its bilinear upsample added in the
                              // epilogue of the skip half's 1x1 (gemm2.hip, ConvParams::up_z) - the upsampled tensors are never written; 0 = upsample kernel + two-source 1x1
  int fc7_fold = 1;           // split engines, CRAFT: slice5.1 (3x3, dilation 6) -> slice5.2 (1x1) -> upconv1.0's fc7 half (1x1), three linear maps with no activation between
                              // them, as ONE 3x3 of 512 -> 512 folded at load time (Engine::load_craft), upconv1.0's skip half as a 1x1 into an fp32 addend of that launch's
                              // epilogue (Engine::fc7_folded): the two 1024-channel tensors are neither computed nor stored; 0 = the three layers as the reference runs them
  int head_tail = 1;          // ... and the two 1x1 layers behind conv_cls.4 inside its epilogue (no 16-channel tensors, two launches less); 0 = fp32 MFMA launches
  int first_fused = 1;        // pairs, pages that tile into 8 x 32 patches: conv1_1 evaluated inside conv1_2's kernel on the halo patch (conv3p.hip, FIRST on pairs) - the
                              // 64-channel full-resolution tensor is neither written nor read; bit-identical to the two launches (0: conv1_split_kernel + the plain tile)
  int head_packed = 1;        // ... with pairs: the 32-channel head tensors as 128-byte pixel rows [x0 | x1] and conv_cls.0 / .2 / .4 on packed pairs (two virtual
                              // chunks instead of three over zero-padded 64-channel rows: two thirds of the MFMAs, half the bytes); 0 = zero-padded rows
  int detector_only = 0;      // profiling: drop every detected box, so that a batch runs the detector + CCL only
  int bench_grid_boxes = 0;   // benchmark workload control (bench.py --boxes=grid40): the detector runs in full, then every page's boxes are replaced by a fixed 5 x 8 grid
  int split_planes = 1;       // split-operand engines: activations stay in planes between the layers (0: fp32 tensors + a split pass in front of every GEMM)
  int split_conv3p = 1;       // split-operand engines: 3x3 layers on the patch-stationary kernel (0: gemm2)
  int split_gemm = 1;         // split-operand engines: 0 = every layer on the fp32 MFMA kernel (A/B and tests)
  int craft_group = 16;       // pages per CRAFT launch group, at most (1 .. 32).  f16x4: capped by what the widest tensor of the configuration allows inside the 2 GiB
                              // window of 32-bit buffer offsets (craft_group_pages below: 21 pages of 1024 x 768 with first_fused, 10 without, 7 as triples), then evened
                              // to 16 or 8; activation workspace ~0.35 GB/page.  craft_group = 8 is the schedule of before the cap followed the configuration
  int ar_tail_step = 12;      // with ar_early_exit: AR steps from this one on run as ONE launch of the fused kernel (which returns at once when the batch is done)
  int ar_crop_exit = 1;       // ... and, per crop, the two attention kernels of a step return for crops that have emitted EOS
  int ar_early_exit = 1;      // bf16 kernel-per-op AR loop: the steps' kernels return at once when every crop of the batch has emitted EOS (upstream's break)
  int decoder_mode = 1;       // 0 = kernel-per-op AR loop, 4/8/16 = fused kernel with that many crops per workgroup, else automatic
  int sp_hidden16 = 0;        // split engines, encoder MLP: the hidden activation (fc1 -> fc2, 1 GB per layer at 1280 crops) as 16-row pieces in the producing epilogue's lane
                              // order - a store instruction writes one contiguous KiB (gemm_sp.hip, x_tiled / out_tiled = 2); 2 = and those stores stream (nt) past the
                              // weights and activation rows the tiles re-read from L2; 0 = the loader's 8-row pieces
  int craft_lanes = 1;        // split engines, batches of >= 2 CRAFT launch groups: 2 = the groups on two staggered streams (Engine::lane_stream) - measured: no gain
                              // (403.0 / 403.3 against 403.7 / 404.3 pages/s: both lanes want the matrix pipe and the power budget); 1 = one after the other
  int recog_overlap = 1;      // streamed batches: the recogniser of batch j - 1 on a stream of its own, beside the detector of batch j (they share no buffer): the
                              // HBM-bound kernels and tile tails of one run under the other's matrix work.  Per-kernel times then include the neighbour's share of the chip
  int images_batch = 32;      // ttr_images_to_data: pages per streamed batch (same-sized images travel together)
  int range_guard = 1;        // split engines: every kernel that writes planes watches |x| < 65504 (split.h: RangeWatch); a tripped batch 1 = fails the call naming the
                              // layer, 2 = warns on stderr and returns the (saturated) result, 0 = not watched
  bool set(const std::string& k, int value) {
    if (k == "decoder_mode") decoder_mode = value;
    else if (k == "enc_chunk") enc_chunk = value;
    else if (k == "range_guard") range_guard = value;
    else if (k == "recog_overlap") recog_overlap = value;
    else if (k == "craft_lanes") craft_lanes = value == 2 ? 2 : 1;
    else if (k == "sp_hidden16") sp_hidden16 = value;
    else if (k == "images_batch") images_batch = value < 1 ? 1 : (value > 256 ? 256 : value);
    else if (k == "up_commute") up_commute = value;
    else if (k == "fc7_fold") fc7_fold = value;
    else if (k == "gpu_calipers") gpu_calipers = value;
    else if (k == "skinny_split") skinny_split = value;
    else if (k == "skinny_max_rows") skinny_max_rows = value;
    else if (k == "ar_host_check") ar_host_check = value;
    else if (k == "sp_tiled_w") sp_tiled_w = value;
    else if (k == "sp_tiled_x") sp_tiled_x = value;
    else if (k == "argmax_fold") argmax_fold = value;
    else if (k == "embed_fold") embed_fold = value;
    else if (k == "skx_ln_fuse") skx_ln_fuse = value;
    else if (k == "qkv_attn_split") qkv_attn_split = value;
    else if (k == "fuse_first") fuse_first = value;
    else if (k == "ln_fuse") ln_fuse = value;
    else if (k == "tok_fuse") tok_fuse = value;
    else if (k == "ar_early_exit") ar_early_exit = value;
    else if (k == "ar_crop_exit") ar_crop_exit = value;
    else if (k == "ar_tail_step") ar_tail_step = value;
    else if (k == "split_gemm") split_gemm = value;
    else if (k == "bench_grid_boxes") bench_grid_boxes = value;
    else if (k == "detector_only") detector_only = value;
    else if (k == "craft_products") craft_products = value == 4 ? 4 : 3;
    else if (k == "head_packed") head_packed = value;
    else if (k == "first_fused") first_fused = value;
    else if (k == "head_tail") head_tail = value;
    else if (k == "enc_ln_pairs") enc_ln_pairs = value;
    else if (k == "enc_fc2_pairs") enc_fc2_pairs = value;
    else if (k == "qkv_kv_pairs") qkv_kv_pairs = value;
    else if (k == "dec_planes") dec_planes = value;
    else if (k == "split_conv3p") split_conv3p = value;
    else if (k == "split_planes") split_planes = value;
    else if (k == "craft_group") craft_group = value < 1 ? 1 : (value > 32 ? 32 : value);
    else if (k == "mlp_fused") mlp_fused = value;     // 0 off, 1 from mlp_min_rows rows on, 2 always
    else if (k == "mlp_min_rows") mlp_min_rows = value;
    else if (k == "dec_mlp_fused") dec_mlp_fused = value;
    else if (k == "dec_mlp_min_rows") dec_mlp_min_rows = value;
    else if (k == "mlp_proj") mlp_proj = value;
    else if (k == "qkv_attn") qkv_attn = value;        // 0 off, 1 from qkv_attn_min crops on, 2 always
    else if (k == "qkv_attn_min") qkv_attn_min = value;
    else if (k == "dbg_bf16_out") dbg_bf16_out = value;
    else return false;
    return true;
  }
};
extern Tuning g_tuning_default;   // engine.cpp

// ------------------------------------------------------------------ launch groups (DESIGN.md section d / e: "Launch groups")
// The f16x4 kernels address their plane tensors with 32-bit buffer offsets: a tensor of a launch must end below 2^31 bytes (0x80000000 is the loaders'
// out-of-range marker).  The detector therefore walks a batch in groups of pages and the encoder one in groups of crops, as large as the WIDEST tensor of the
// configuration in force allows.  These functions are that figure, pure host arithmetic (ttr_dbg_launch_groups): the caps, the workspaces and the forward
// passes' own refusals all come from them, so that none can drift from the others.
constexpr size_t kOffsetWindow = ((size_t)1 << 31) - 1;   // most bytes a tensor addressed with 32-bit offsets may hold
struct Widest { size_t bytes; const char* layer; };       // bytes per page / per crop of the widest tensor, and the layer that writes it
// CRAFT on a canvas of H x W (a multiple of 32 each), f16x4: every tensor craft_forward_split hands a kernel.  first_fused is the EFFECTIVE switch (the tuning key,
// pairs and the split 3x3 tiles on); craft_products 3 = pairs (4 bytes per value), 4 = triples (6)
// fc7_fold = 1: the pass allocates no slice5.1 / slice5.2 tensors (tn.fc7_fold outside a tapped pass) and upconv1.0 has an fp32 addend of 512 channels
struct CraftGroupCfg { int first_fused = 1, craft_products = 3, up_commute = 1, fc7_fold = 0; };
Widest craft_widest_per_page(int H, int W, const CraftGroupCfg& c);
// pages per CRAFT launch group for a batch of n: min(craft_group, window / per page), then evened - 16 when n % 16 == 0, else 8 when n % 8 == 0 (64 pages = 4 x 16
// rather than 21 + 21 + 21 + 1)
int craft_group_pages(int H, int W, int n, int craft_group, const CraftGroupCfg& c);
// the split encoder's tensors per crop (128 rows): LayerNorm planes, the qkv planes of the unfused path (0 when qkv + attention are one launch), the MLP hidden,
// the attention output; sp_hidden16 moves the hidden's layout, not its size
struct EncGroupCfg { int enc_fc2_pairs = 1, qkv_attn_split = 1, enc_ln_pairs = 1, sp_hidden16 = 0; };
struct EncTensors {
  size_t ln, qkv, hidden, att;
  size_t big() const { return std::max(qkv, hidden); }   // kWsBigPlanes holds either
  Widest widest() const;
};
EncTensors encoder_bytes_per_crop(const EncGroupCfg& c);
// crops per encoder group for N crops: min(window / per crop, enc_chunk), then even groups (2731 crops = 1366 + 1365 under enc_chunk = 4096).  enc_chunk = 0 stands
// for kEncGroupDefault: one group of the benchmark's 2560 crops fits the window of the default path, but measured against 1280 + 1280 on the same box it was never
// ahead (-1.3 % pages/s beside 8-page CRAFT groups, +-0.3 % beside 16-page ones: profiles/groups.md), so the groups of before stay the default and the key lifts them
constexpr int kEncGroupDefault = 1820;
int encoder_group_crops(int N, int enc_chunk, const EncGroupCfg& c);

// ------------------------------------------------------------------ small utilities
// roctx ranges around the host phases of a batch (rocprofv3 --marker-trace shows them next to the kernels).
// The marker library is looked up at run time: without it the ranges are no-ops.
struct Roctx {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
  Roctx() {
    for (const char* n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      if (void* h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) {
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA"); pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr; pop = nullptr;
      }
    }
  }
};
inline Roctx& roctx() { static Roctx r; return r; }
struct RangeScope {
  bool on;
  explicit RangeScope(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~RangeScope() { if (on) roctx().pop(); }
};

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  size_t cap_seen = 0;   // the last capacity this buffer had (survives the window in which cap is 0 during a re-allocation)
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    void* old = p;
    p = nullptr; cap = 0;                       // a throwing hipFree must not leave a dangling pointer for the destructor
    if (old) TTR_HIP_CHECK(hipFree(old));
    // a buffer that grows again grows by a quarter at least: batches of slightly different crop counts must not re-allocate (hipFree waits for the whole
    // device) pass after pass - 288 GB of HBM make the slack free
    const size_t old_cap = cap_seen;
    size_t want = std::max(bytes, old_cap ? old_cap + old_cap / 4 : (size_t)0);
    want = (want + (1u << 20) - 1) & ~(size_t)((1u << 20) - 1);
    TTR_HIP_CHECK(hipMalloc(&p, want));
    cap = want; cap_seen = want;
  }
  template <typename U> U* as() const { return reinterpret_cast<U*>(p); }
  ~DevBuf() { if (p) (void)hipFree(p); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

static inline uint16_t f32_to_bf16_rne(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// grow-only pinned host buffer: async copies to / from it need no staging and do not serialise the stream
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  void ensure(size_t bytes) {
    if (bytes <= cap) return;
    void* old = p;
    p = nullptr; cap = 0;
    if (old) TTR_HIP_CHECK(hipHostFree(old));
    size_t want = (bytes + 65535) & ~(size_t)65535;
    TTR_HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
    cap = want;
  }
  template <typename U> U* as() const { return reinterpret_cast<U*>(p); }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
};

// The host half of an opt-in page layer's side block, per pipeline slot: the pinned copy and the bytes the slot's batch fetches into it, 0 = the layer did not
// run for that batch.  recog_enqueue disarms the slot's records; each layer arms its own where it sizes its device block; fetch copies exactly the armed bytes;
// finish reads through view(), so that a layer that did not run has no block to misread.  The device half stays a DevBuf member of the engine (kDevBufTable).
struct SideCopy {
  PinnedBuf host[2];
  size_t bytes[2] = {0, 0};
  void arm(int sl, size_t b) { host[sl].ensure(b); bytes[sl] = b; }
  void disarm(int sl) { bytes[sl] = 0; }
  void fetch(int sl, const DevBuf& dev, hipStream_t s) const { if (bytes[sl]) TTR_HIP_CHECK(hipMemcpyAsync(host[sl].p, dev.p, bytes[sl], hipMemcpyDeviceToHost, s)); }
  template <typename U> const U* view(int sl) const { return bytes[sl] ? host[sl].as<U>() : nullptr; }
};

// A GEMM-shaped weight on the device: T [Cout_pad][K_pad] + f32 bias
struct Linear {
  DevBuf w, b;
  int cout = 0, k = 0;  // padded sizes as the kernel sees them
  int cout_valid = 0;   // != 0: the layer's own output count, below `cout` (PARSeq's head: 95 classes in 96 weight rows, so that it has f16 planes); the kernels get this as Cout
  DevBuf ws;            // split-operand engines (split.h): f16 [cout][3][k] = w0 | w0/2^11 | w1 of w S
  DevBuf wst;           // ... the same planes as the loader pieces of gemm_sp.hip (Engine::tile_planes): f16 [ceil(cout / 32) * 4][3][k / 64][8 rows][64]
  DevBuf wsp;           // ... CRAFT's 3x3 layers of 32 input channels, PACKED pairs form (conv3p.hip, NP = 2): f16 [cout][3][taps * 64], per tap
                        // plane 0 = [w0 (32) | w0 / 2^11 (32)], plane 1 unused, plane 2 = [w1 (32) | 0]; multiplies pixel rows [x0 (32) | x1 (32)]
  float inv_scale = 0;  // 1 / S
  int dil = 1;          // CRAFT's 3x3 layers: the dilation (CraftConv::dil; 6 for slice5.1 and the layer folded from it)
};

// ------------------------------------------------------------------ the engine
struct CraftConv { const char* name; int cin, cout, ks, dil; };

struct Result {
  std::vector<std::string> text;
  std::vector<float> bbox;   // 4 per item
  std::vector<int32_t> ids;  // 26 per item
  std::vector<float> quad;   // 8 per item: the word's corners tl, tr, br, bl in image pixels (geometry.h: deskew_quad), every crop mode
  std::vector<float> prob;   // 26 per item: softmax probability of each argmax id (decode_conf.hip)
  std::vector<float> conf;   // 1 per item: the word's confidence (DESIGN.md "Recognition confidence")
  std::vector<int32_t> set;  // 1 per item: the caller's set index (results of the region entry points only; DESIGN.md "Regions and per-row character sets")
  // character alternatives (ttr_engine_set_alternatives; DESIGN.md "Character alternatives"): 0 / empty when off
  int alt_k = 0;                   // K: alternatives per position, the winner included
  std::vector<int32_t> alt_ids;    // 26 K per item: the K best allowed classes of every position, -1 in the empty slots (decode_alts.hip)
  std::vector<float> alt_prob;     // 26 K per item: their softmax probabilities; slot 0 is `prob`
  // lexicon matches (ttr_engine_set_lexicon; DESIGN.md "Lexicon matching"): 0 / empty when no lexicon is set
  int lex_m = 0;                   // M: matches kept per item
  std::vector<int32_t> lex_idx;    // M per item: the M best entries of the engine's word list by (logp descending, index ascending), -1 in the empty slots (lexicon.hip)
  std::vector<float> lex_logp;     // M per item: their log-probabilities, -INFINITY in the empty slots
  int lex_band = -1;               // fuzzy alignment (ttr_engine_set_lexicon_fuzzy): the band the matches were scored under, -1 = off (the rigid scorer)
  std::vector<int32_t> lex_edits;  // ... M per item: the edits of each match's alignment, -1 in the empty slots; empty when the mode is off (lexicon_fuzzy.hip)
  std::vector<float> pattern_logp; // patterns in best mode: one per item, the log-probability of its reading (-INFINITY for an item without a pattern); empty otherwise
  // word orientation (cfg.orient != TTR_ORIENT_OFF; DESIGN.md "Word orientation"): empty when off
  std::vector<int32_t> orient;      // 1 per item: the chosen turn 0..3
  std::vector<float> orient_conf;   // orient_k per item: every candidate's conf, ascending turn
  int orient_k = 1, page_orient = 0;
  // text lines (cfg.lines = 1; DESIGN.md "Text lines"): empty / 0 when off
  std::vector<int32_t> line, word;          // 1 per item: its line in line order, its position inside that line
  std::vector<int32_t> order, line_first;   // the items in reading order; [n_lines + 1] the lines' offsets into `order`
  std::vector<float> line_bbox;             // 4 per line: min / max of the members' bbox
  int n_lines = 0;
  std::string line_text(int l) const;       // the members' text in word order, joined by ' '
  std::string page_text() const;            // the lines joined by '\n'
  // character boxes (cfg.chars = 1; DESIGN.md "Character boxes"): empty when off
  std::vector<int32_t> char_first;          // [items + 1]: item i owns characters [char_first[i], char_first[i + 1])
  std::vector<float> char_quad, char_bbox;  // 8 / 4 per character: tl, tr, br, bl; min x, min y, max x, max y
  std::vector<int32_t> char_cuts, char_mode;   // 27 / 1 per item: the cuts b[0..K] in 1/256 column (-1 beyond K); 0 uniform, 1 valley cuts
  std::vector<uint8_t> char_profile;        // 128 per item: the word's profile q
  // wide words (ttr_engine_set_wide; DESIGN.md "Wide words"): empty when off
  std::vector<int32_t> piece_first;         // [items + 1]: item i owns pieces [piece_first[i], piece_first[i + 1]); an item that is not wide owns one, itself
  std::vector<int32_t> piece_ids;           // 26 per piece
  std::vector<float> piece_prob, piece_conf, piece_quad;   // 26 / 1 / 8 per piece
  std::vector<int32_t> piece_cuts;          // 17 per item: c_0 = 0 < ... < c_n = 128 n in frame columns, -1 beyond n
  // curved words (ttr_engine_set_curved; DESIGN.md "Curved words"): empty when off
  std::vector<int32_t> curved;              // 1 per item: 1 = its crop was straightened along its spine
  std::vector<float> outline;               // 36 per item: 18 points, the top edge left to right, then the bottom edge right to left
  std::vector<int64_t> spine_knots;         // 36 per item: the knot table {Cx, Cy, Hx, Hy} x 9 in 2^-16 px (zeros for an item whose second pass did not run)
  // tables (ttr_engine_set_tables; DESIGN.md "Tables"): 0 / empty when off and for a page without items
  int table_mode = 0;                       // 1, or -(step) of the cap the page overflowed
  std::vector<int32_t> rulings;             // 6 per ruling: dir, x0, y0, x1, y1, table
  std::vector<int32_t> tables;              // 8 per table: x0, y0, x1, y1, rows, cols, first cell, cell count
  std::vector<int32_t> table_lines;         // per table its rows + 1 row lines, then its cols + 1 column lines, in doubled px
  std::vector<int32_t> cells;               // 9 per cell: table, row, col, rowspan, colspan, x0, y0, x1, y1
  std::vector<int32_t> item_table, item_cell;   // 1 per item: -1 = in no cell
  // selection marks (ttr_engine_set_marks; DESIGN.md "Selection marks"): 0 / empty when off and for region calls
  int mark_mode = 0;                        // 1, or -6 for a page of more than 512 marks
  std::vector<int32_t> marks;               // 12 per mark: x0, y0, x1, y1, ix0, iy0, ix1, iy1, inked, area, state, label
  std::vector<int32_t> item_mark;           // 1 per item: the mark its centre lies in, -1 = none
  // barcodes (ttr_engine_set_barcodes; DESIGN.md "Barcodes"): 0 / empty when off and for region calls
  int barcode_mode = 0;                     // 1, or -7 for a page of more than 64 barcodes
  std::vector<int32_t> barcodes;            // 24 per barcode: x0, y0, x1, y1, symbology, dir, lines, module64, flags, len, 0, 0, text [12]
  std::vector<int32_t> item_barcode;        // 1 per item: the barcode its centre lies in, -1 = none
  // text blocks (cfg.blocks = 1; DESIGN.md "Text blocks"): empty / 0 when off
  std::vector<int32_t> line_block, line_pos;     // 1 per line: its block in reading order, its position inside that block
  std::vector<int32_t> block;                    // 1 per item: its line's block
  std::vector<int32_t> block_order, block_first; // the lines in block reading order; [n_blocks + 1] the blocks' offsets into `block_order`
  std::vector<float> block_bbox;                 // 4 per block: min / max of the member lines' bbox
  int n_blocks = 0, block_mode = 0;              // block_mode 1: ordered by the precedence relation; 0: more than 512 blocks, by key alone
  int tiles = 0;                                 // tiled pages (ttr_engine_set_tiled; DESIGN.md "Tiled pages"): the tiles the page's detector ran as, 0 when off
  // deskew (ttr_engine_set_deskew; DESIGN.md "Deskew"): skew_on 0 when the layer was off; else the page's record - every coordinate of this result is in the
  // upright page's frame, and deskew_to_page maps it to the caller's (a region call: slope 0, the identity)
  int skew_on = 0;
  DeskewRec skew{};
  // local ink (ttr_engine_set_ink; DESIGN.md "Local ink"): ink_on 0 when no pass of this page ran under it; else the record of the tables pass when tables ran,
  // else that of the deskew pass
  int ink_on = 0;
  InkRec ink{};
  std::string block_text(int b) const;           // the block's lines joined by '\n'
  std::string page_text_blocks() const;          // the blocks in reading order, joined by "\n\n"
};

struct CclBatch {   // device workspaces of the CCL stage for a batch of equally sized pages
  DevBuf tnorm, flags, parent, mm, area, bbox, maxt, cand_slot, cand, counters, rows;
  DevBuf rects, cal_pool, cal_ctr;   // GPU-side minAreaRect: per-candidate results, the hulls' scratch pool and its bump counter
  static constexpr int kCalCap = 4 << 20;   // floats (16 MB: ~230 k hull points per CRAFT group - half of that per lane when two detector lanes are active; a group that needs more falls back to the host's calipers)
  int pages = 0, npx = 0, max_cand = 0;
  int cal_cap_now = kCalCap;          // (tuning key gpu_calipers = 2 shrinks it to 512 floats: the host-fallback path under test)
  bool split_pool = false;            // two detector lanes are active for this batch: each takes half of the hulls' pool (set by detect_enqueue)
  CclBuffers view(int p0 = 0, int lane = 0) {   // the slices of pages p0.. (every array is strided by the page); lane: which half of the hulls' pool (two detector lanes)
    CclBuffers b;
    const size_t o = (size_t)p0 * npx;
    b.tnorm = tnorm.as<float>() + o; b.flags = flags.as<uint8_t>() + o; b.parent = parent.as<int>() + o; b.mm = mm.as<unsigned>() + (size_t)p0 * 4;
    b.area = area.as<int>() + o; b.bbox = bbox.as<int>() + o * 4; b.maxt = maxt.as<unsigned>() + o; b.cand_slot = cand_slot.as<int>() + o;
    b.cand = cand.as<int>() + (size_t)p0 * max_cand * 8; b.counters = counters.as<int>() + (size_t)p0 * 2; b.rows_packed = rows.as<int>() + o * 2;
    b.max_cand = max_cand;
    b.rects = rects.as<float>() + (size_t)p0 * max_cand * 8;
    b.cal_pool = cal_pool.as<float>() + (split_pool ? (size_t)lane * (kCalCap / 2) : 0); b.cal_ctr = cal_ctr.as<int>() + lane; b.cal_cap = std::min(cal_cap_now, split_pool ? kCalCap / 2 : kCalCap);
    return b;
  }
  void ensure(int pages_, int npx_, int max_cand_) {
    pages = pages_; npx = npx_; max_cand = max_cand_;
    const size_t n = (size_t)pages * npx;
    tnorm.ensure(n * 4); flags.ensure(n); parent.ensure(n * 4); mm.ensure((size_t)pages * 16);
    area.ensure(n * 4); bbox.ensure(n * 16); maxt.ensure(n * 4); cand_slot.ensure(n * 4);
    cand.ensure((size_t)pages * max_cand * 32); counters.ensure((size_t)pages * 8); rows.ensure(n * 8);
    rects.ensure((size_t)pages * max_cand * 32); cal_pool.ensure((size_t)kCalCap * 4); cal_ctr.ensure(64);
  }
};




#define TTR_NCCL_CHECK(expr)                                                                                          \
  do {                                                                                                                \
    ncclResult_t _r = (expr);                                                                                         \
    if (_r != ncclSuccess) throw std::runtime_error(std::string("RCCL: ") + ncclGetErrorString(_r) + " at " #expr);   \
  } while (0)

// Multi-GPU exchange in the C++ host (RCCL = the NCCL API of /opt/rocm/include/rccl/rccl.h): one process per GPU.
// The engine speaks to a Transport: two kinds of collective on device buffers, enqueued on a stream -
//   all_gather (data: the per-batch token ids on the engine's main stream; control: the small host-side exchanges - crop counts, status
//   headers, barriers - on the copy stream) and broadcast (latency mode's crop batch).
// RcclTransport is the product: two communicators per process (collectives of one communicator must be issued in one order on every rank,
// and the two kinds interleave differently from batch to batch).  SocketTransport carries the SAME calls over TCP through rank 0, staged
// through host memory, every call framed with a sequence number and its size so that a mismatched call sequence is an error, not a hang: it
// is what lets two ranks share ONE GPU (RCCL refuses two ranks on a device), i.e. what runs the engine's multi-rank code paths at world
// size 2 on a single-GPU box (tests/test_gpu_dist.py), and a fallback where RCCL cannot initialise.
struct Transport {
  virtual ~Transport() {}
  virtual const char* name() const = 0;
  virtual void all_gather(const void* d_send, void* d_recv, size_t bytes, bool control, hipStream_t stream) = 0;   // d_recv: world * bytes, by rank
  virtual void broadcast(void* d_buf, size_t bytes, int root, hipStream_t stream) = 0;
};

struct Comm {
  std::unique_ptr<Transport> tr;
  int rank = 0, world = 1;
  struct Engine* E = nullptr;
  DevBuf d_in, d_out;
  PinnedBuf h_in, h_out;
};

// The layout of a gathered batch (pure host logic, tests/test_comm_cpu.py drives it through ttr_gather_layout): every rank
// contributes its crops-per-page counts first; the payload then travels as `cap` = the largest rank total rows of 26 ids per rank.
// Nothing is truncated: a page may hold any number of crops.
struct GatherLayout {
  int world = 0, pages = 0, cap = 0;
  std::vector<int> total;      // crops of rank r
  std::vector<int64_t> first;  // row of (rank r, page p)'s first crop in the compacted [sum(total)][26] array
  static GatherLayout from_counts(const int32_t* counts, int world, int pages) {
    GatherLayout L;
    L.world = world; L.pages = pages; L.total.assign(world, 0); L.first.assign((size_t)world * pages + 1, 0);
    int64_t run = 0;
    for (int r = 0; r < world; ++r)
      for (int p = 0; p < pages; ++p) {
        const int c = counts[(size_t)r * pages + p];
        if (c < 0) throw std::runtime_error("gather: negative crop count");
        L.first[(size_t)r * pages + p] = run;
        run += c; L.total[r] += c;
      }
    L.first[(size_t)world * pages] = run;
    for (int r = 0; r < world; ++r) L.cap = std::max(L.cap, L.total[r]);
    return L;
  }
};

// ------------------------------------------------------------------ the engine's device buffers, classified (ttr_dbg_scratch_table, ttr_dbg_poison_scratch)
// Every DevBuf declared in this header has one row here (tests/test_scratch_table_cpu.py holds the two lists together; members of the helper structs carry their
// owner's name: ccl. / linear. / head_tail. / comm.).
//   scratch  wholly rewritten by each call that reads it, before it is read: what it holds between calls is nobody's business, and the poison hook may fill it
//   kept     its contents must survive from call to call; the row says why
// kind: what the poison hook writes - f32 / f16 (16-bit planes) / u8 patterns, and ALWAYS zeros into i32 (indices, counters, integer records and blocks that mix
// integers with floats: a stale index that gets read must come out as a wrong value, never as a wild address) and nothing at all into addr (rows that hold device
// addresses: a zero address is no safer than a stale one)
enum BufKind : uint8_t { kElF32 = 0, kElF16 = 1, kElU8 = 2, kElI32 = 3, kElAddr = 4 };
struct BufRow { const char* name; bool kept; BufKind kind; const char* note; };
constexpr BufRow kDevBufTable[] = {
    // ---- weights and other uploads
    {"linear.w", true, kElF32, "a layer's weight in the engine's type, uploaded once by the constructor"},
    {"linear.b", true, kElF32, "a layer's fp32 bias, uploaded once by the constructor"},
    {"linear.ws", true, kElF16, "a layer's f16 weight planes, written once by upload_linear"},
    {"linear.wst", true, kElF16, "the same planes as gemm_sp's loader pieces, written once by tile_planes"},
    {"linear.wsp", true, kElF16, "the packed-pairs form of a 32-channel 3x3 layer's planes, written once by load_craft"},
    {"head_tail.w6", true, kElF32, "conv_cls.6's weight for the fused head tail, uploaded once by load_head_tail"},
    {"head_tail.w8", true, kElF32, "conv_cls.8's weight for the fused head tail, uploaded once by load_head_tail"},
    {"head_tail.b6", true, kElF32, "conv_cls.6's bias, uploaded once by load_head_tail"},
    {"head_tail.b8", true, kElF32, "conv_cls.8's bias, uploaded once by load_head_tail"},
    {"pqf", true, kElF32, "the recogniser's fp32 vectors (LayerNorm parameters, embeddings, position queries), uploaded once by load_parseq"},
    {"fc1_packed", true, kElF16, "bf16 engines: encoder fc1 weights as mlp_fused's LDS images, uploaded once"},
    {"proj_packed", true, kElF16, "bf16 engines: encoder attn.proj weights k-step-major, uploaded once"},
    {"fc2_packed", true, kElF16, "bf16 engines: encoder fc2 weights chunk-major, uploaded once"},
    {"dec_ffn1_packed", true, kElF16, "bf16 engines: the decoder's linear1 as an mlp_fused image, uploaded once"},
    {"dec_ffn2_packed", true, kElF16, "bf16 engines: the decoder's linear2 as an mlp_fused image, uploaded once"},
    {"dec_co_packed", true, kElF16, "bf16 engines: the decoder's cross_attn.out_proj as an mlp_fused image, uploaded once"},
    {"qself", true, kElF32, "the projected position queries, computed on the host and uploaded once by load_parseq"},
    {"lex_records", true, kElU8, "the caller's word list as 32-byte records, uploaded by ttr_engine_set_lexicon and read by every pass until the next one"},
    {"pattern_dev", true, kElI32, "the engine's pattern table, uploaded by set_engine_pattern: nothing travels per call"},
    {"dsk_cs", true, kElI32, "deskew's (C, S) table, uploaded by the first call that needs it (dsk_cs_up)"},
    {"range_word", true, kElI32, "the range guard's sticky words: zeroed by the constructor, and each is cleared again by the stream that fetched it"},
    {"ar_done", true, kElI32, "the AR loop's done counter: its first word is cleared on the stream in front of every loop, the host reads it between steps"},
    // ---- the detector
    {"craft_ws_set", false, kElF16, "per slot as ws() noted it: planes or fp32; the slots ws() zeroed once (zero_new: the unpacked head tensors' padding channels) are kept and left alone"},
    {"canvas", false, kElU8, ""},
    {"heat", false, kElF32, ""},
    {"tile_heat", false, kElF32, ""},
    {"tile_table", false, kElAddr, ""},
    {"page_table", false, kElAddr, ""},
    {"staging_img", false, kElU8, ""},
    {"stage_dev", false, kElU8, ""},
    {"split_in", false, kElF16, ""},
    {"dsk_bits", false, kElU8, ""},
    {"dsk_bitsT", false, kElU8, ""},
    {"dsk_scores", false, kElI32, ""},
    {"dsk_rec", false, kElI32, ""},
    {"dsk_ink_h", false, kElU8, ""},
    {"dsk_ink_rec", false, kElI32, ""},
    {"dsk_table", false, kElAddr, ""},
    {"dsk_pages", false, kElU8, ""},
    // ---- post-processing
    {"ccl.tnorm", false, kElF32, ""},
    {"ccl.flags", false, kElU8, ""},
    {"ccl.parent", false, kElI32, ""},
    {"ccl.mm", false, kElI32, ""},
    {"ccl.area", false, kElI32, ""},
    {"ccl.bbox", false, kElI32, ""},
    {"ccl.maxt", false, kElI32, ""},
    {"ccl.cand_slot", false, kElI32, ""},
    {"ccl.cand", false, kElI32, ""},
    {"ccl.counters", false, kElI32, ""},
    {"ccl.rows", false, kElI32, ""},
    {"ccl.rects", false, kElI32, "a kind word in front of seven floats per candidate"},
    {"ccl.cal_pool", false, kElF32, ""},
    {"ccl.cal_ctr", false, kElI32, ""},
    {"crops", false, kElU8, ""},
    {"rects_dev", false, kElI32, ""},
    {"coef_dev", false, kElI32, ""},
    // ---- the recogniser
    {"pq_ws", false, kElF32, "per slot: fp32 tensors up to kWsStepLogits, f16 planes from kWsLnPlanes on; kWsKvcache is kept: zeroed once per capacity by parseq_ar (kvcache_zeroed), "
                             "slots behind an early exit keep older finite rows, which the attention kernels mask"},
    {"logits", false, kElF32, ""},
    {"ar_logits", false, kElF32, ""},
    {"ids_dev", false, kElI32, "ids | prob | conf"},
    {"tokens", false, kElI32, ""},
    {"row_masks_dev", false, kElI32, ""},
    {"pat_rows_dev", false, kElI32, ""},
    {"pat_state", false, kElI32, ""},
    {"pat_best_scratch", false, kElI32, "ids | prob | conf"},
    {"pat_logp_dev", false, kElF32, ""},
    {"gath_dev", false, kElI32, "the ranks' ids | prob | conf blocks"},
    {"comm.d_in", false, kElU8, ""},
    {"comm.d_out", false, kElU8, ""},
    // ---- the opt-in layers' inputs and side blocks
    {"orient_in", false, kElI32, ""},
    {"orient_cand", false, kElI32, "ids | prob | conf"},
    {"orient_side", false, kElI32, ""},
    {"lines_in", false, kElI32, ""},
    {"lines_side", false, kElI32, ""},
    {"alts_side", false, kElI32, "ids | prob"},
    {"lex_side", false, kElI32, "idx | logp | edits"},
    {"lex_part", false, kElI32, "idx | logp"},
    {"wide_side", false, kElI32, "cuts | u16 profiles"},
    {"curve_side", false, kElI32, ""},
    {"tab_bits", false, kElU8, ""},
    {"tab_bitsT", false, kElU8, ""},
    {"tab_runs", false, kElI32, ""},
    {"tab_side", false, kElI32, ""},
    {"tab_ink_h", false, kElU8, ""},
    {"tab_ink_rec", false, kElI32, ""},
    {"mark_cand", false, kElI32, ""},
    {"mark_counts", false, kElI32, ""},
    {"mark_side", false, kElI32, ""},
    {"bc_hits", false, kElI32, ""},
    {"bc_cnt", false, kElI32, ""},
    {"bc_side", false, kElI32, ""},
    {"blocks_side", false, kElI32, ""},
    {"chars_map", false, kElF32, ""},
    {"chars_in", false, kElI32, ""},
    {"chars_side", false, kElI32, "cuts | modes | u8 profiles"},
};

struct Engine {
  ttr_config cfg;
  Tuning tn = g_tuning_default;
  Precision prec;
  size_t es;  // element size of T
  hipStream_t stream = nullptr;
  std::unique_ptr<HostPool> host_pool;
  hipStream_t recog_stream = nullptr;             // tn.recog_overlap: the recogniser of a streamed batch runs here
  hipStream_t copy_stream = nullptr;              // device -> host copies of one page group's components while the next group's CRAFT runs
  hipEvent_t copy_ev = nullptr, done_ev[2] = {nullptr, nullptr};   // done_ev[slot]: a batch's token ids have landed
  hipEvent_t evr[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // per slot: before the packer, after it, after PARSeq
  // hand-over points of a batch are polled, not slept on: a blocking wait costs tens of microseconds of wake-up per sync
  static void spin_event(hipEvent_t e) {
    for (;;) {
      const hipError_t r = hipEventQuery(e);
      if (r == hipSuccess) return;
      if (r != hipErrorNotReady) hip_fail("hipEventQuery", r, __FILE__, __LINE__);
    }
  }
  std::vector<hipEvent_t> group_ev;               // per page group: component counters are on the host
  std::mutex mu;
  Tokenizer tok;
  int alts = 0;                                   // alternatives per position, 0 = off or 2..8 (ttr_engine_set_alternatives; DESIGN.md "Character alternatives")
  // lexicon matching (ttr_engine_set_lexicon; DESIGN.md "Lexicon matching"): the caller's word list, off while lex_v == 0
  int lex_v = 0, lex_m = 0;                       // V words, M matches kept per item (1..8)
  DevBuf lex_records;                             // [V] 32-byte records: length | 25 class bytes | zero padding (geometry.h: lexicon_encode)
  std::vector<std::string> lex_words;             // the host copy of the words (ttr_engine_lexicon_word)
  int lex_band = -1; float lex_gap = 0.f;         // fuzzy alignment (ttr_engine_set_lexicon_fuzzy): the band 0..3 (-1 = off: the rigid scorer) and the gap's log-probability
  float wide = 0.f;                               // wide words: the largest aspect a piece may have, 0 = off or 2..64 (ttr_engine_set_wide; DESIGN.md "Wide words")
  bool curved = false;                            // curved words: straighten the crops of words set on an arc (ttr_engine_set_curved; DESIGN.md "Curved words")
  // selection marks: the smallest side in px, 0 = off or 8..64; the largest side, min..128; the fill threshold in 256ths, 1..255; the ink threshold 1..255
  // (ttr_engine_set_marks; DESIGN.md "Selection marks")
  int marks_min = 0, marks_max = 64, marks_fill = 24, marks_ink = 128;
  // barcodes: the scan lines that must agree, 0 = off or 4..256; the ink threshold 1..255; the symbologies, bit 0 Code 128, bit 1 Code 39
  // (ttr_engine_set_barcodes; DESIGN.md "Barcodes")
  int barcodes_min = 0, barcodes_ink = 128, barcodes_sym = 3;
  int tables_min_len = 0, tables_ink = 128;       // tables: the shortest ruling in px, 0 = off or 16..4096, and the ink threshold 1..255 (ttr_engine_set_tables; DESIGN.md "Tables")
  // tiled pages (ttr_engine_set_tiled; DESIGN.md "Tiled pages"): the tiles' overlap in pixels, 0 = off.  On, a page keeps its own scale (ratio 1, page canvas
  // c32(h) x c32(w)); one larger than the detector canvas goes through CRAFT as overlapping tiles whose maps tile_stitch_kernel joins into `heat`
  int tiled = 0;
  // deskew (ttr_engine_set_deskew; DESIGN.md "Deskew"): max_slope 1..128, 0 = off; the gate in 1/256ths; the ink threshold.  On, detect_enqueue estimates every
  // page's skew and redirects the batch's pages to upright copies in dsk_pages[slot]; everything behind reads those
  int deskew_M = 0, deskew_gain = 288, deskew_ink = 128;
  DevBuf dsk_bits, dsk_bitsT, dsk_scores, dsk_rec; // ... workspaces: the ink bitmaps (tables.hip's pixel pass), scores [pages][2 M + 1], the records [pages]
  DevBuf dsk_cs;                                  // ... the (C, S) table [257][2], uploaded once
  bool dsk_cs_up = false;
  std::vector<int32_t> dsk_cs_host;               // ... and on the host: what decode_pages checks a record's constants against
  DevBuf dsk_table[2], dsk_pages[2];              // ... per slot: the source and upright pages' rows [2][pages] (page_table.h), and the upright pages themselves
  PinnedBuf h_dsk_table[2], h_dsk[2];             // ... per slot: the rows' staging, and the records' host copy
  // local ink (ttr_engine_set_ink; DESIGN.md "Local ink"): radius 1..64, 0 = off; the drop in 1/256ths; the polarity 0 dark, 1 light, 2 auto.  On, the engine's
  // tables and deskew passes take their bitmaps from ink.hip's two kernels instead of table_ink_kernel (their own `ink` is then not consulted); the stage calls
  // and ttr_dbg_tables keep the fixed rule.  Tables and deskew run on different streams: each has its own workspace and records
  int ink_radius = 0, ink_drop = 38, ink_polarity = kInkAuto;
  DevBuf dsk_ink_h, dsk_ink_rec;                  // ... deskew's: the horizontal sums [pages][Hcap][Wcap] uint32, the records [pages]
  static size_t ink_recs_bytes(int pages) { return (size_t)pages * sizeof(InkRec); }   // a pass's records: [pages] InkRec
  PinnedBuf h_dsk_ink[2]; SideCopy h_tab_ink;     // ... the records' host copies: the deskew pass's (the detector's stream; detect_collect takes them), the tables / marks pass's
  DevBuf tile_heat;                               // ... the tile canvases' maps [n T][Hc / 2][Wc / 2][2] (allocated by the first tiled batch)
  DevBuf tile_table[2];                           // ... the tiles as rows of a second page table, per slot (the packers go on reading page_table: the real pages)
  PinnedBuf h_tile_table[2];
  // the canvas and ratio this engine gives an h x w page: canvas_geometry, or - tiled - the page's own size rounded up to 32 (throws tile_plan's refusals)
  CanvasGeom page_geometry(int h, int w) const {
    if (!tiled) return canvas_geometry(h, w, cfg.canvas_size, cfg.mag_ratio);
    const TilePlan p = tile_plan(h, w, cfg.canvas_size, tiled, cfg.mag_ratio);
    return CanvasGeom{h, w, p.hp, p.wp, 1.f};
  }
  ClassMask charset{};                            // classes the recogniser may not choose (ttr_engine_set_charset; DESIGN.md "Character sets"); zero = no set
  // the engine's pattern (ttr_engine_set_pattern; DESIGN.md "Patterns"): empty = none.  `pattern` is pattern_src compiled under `charset`; its table lives in
  // pattern_dev (delta | mind, uploaded once by set_engine_pattern: nothing travels per call)
  std::string pattern_src;
  Pattern pattern;
  DevBuf pattern_dev;
  // a call's table, each row's start state and the extent of its automaton in the table - {first state, states}, DONE not counted (resolve_row_patterns)
  struct PatRows { PatternTable t; std::vector<int32_t> start_of, extent_of; };
  PatDev pattern_own{};                           // the device form of `pattern`; delta == null while there is none
  // the decode mode of patterns (ttr_engine_set_pattern_decode): TTR_PATTERN_GREEDY, or TTR_PATTERN_BEST - every row that has a pattern is read as the
  // likeliest member of its language (pattern.hip: pattern_best_kernel).  Without a pattern in force the mode has no effect
  int pattern_decode = 0;
  // best mode's buffers: the masked argmax's standard block of the pass (launch_decode_conf into scratch: [N][26] id0 | [N][26] prob0 | [N] conf0), and the
  // side block [N] f32 with its pinned twin per slot
  DevBuf pat_best_scratch, pat_logp_dev;
  SideCopy h_pat_logp;
  static size_t pat_logp_bytes(int N) { return (size_t)N * 4; }   // the side block: [N] f32
  struct PatBestOut { int* id0; float* prob0; float* conf0; float* logp; PatExtent ext; };   // logp null = greedy mode
  PatBestOut pat_best_out(int N) {
    const RecOut o = rec_block(pat_best_scratch, N);
    pat_logp_dev.ensure(pat_logp_bytes(std::max(N, 1)));
    return PatBestOut{o.ids, o.prob, o.conf, pat_logp_dev.as<float>(), PatExtent{nullptr, 0, 0}};
  }

  // CRAFT
  std::map<std::string, Linear> craft;
  // split-operand engines: conv_cls.6 / conv_cls.8 as the epilogue of conv_cls.4's packed-pairs tile (ConvParams::tail_*, conv3p.hip)
  struct HeadTail { DevBuf w6, w8, b6, b8; float s6 = 0, s8 = 0; } head_tail;
  // PARSeq
  std::map<std::string, Linear> pq;               // linears by upstream name
  std::map<std::string, DevBuf> pqf;              // f32 vectors (LayerNorm params, pos embed, ...)
  DevBuf fc1_packed[12];                          // bf16 engines: encoder fc1 / fc2 / attn.proj weights as mlp_fused.hip's LDS images
  DevBuf proj_packed[12];                         // bf16 engines: encoder attn.proj weights k-step-major [12][384][32] (mlp_fused.hip, PROJ)
  DevBuf dec_ffn1_packed, dec_ffn2_packed, dec_co_packed;   // bf16 engines: decoder linear1 / linear2 / cross_attn.out_proj as mlp_fused images (refinement pass)
  DevBuf fc2_packed[12];                          // bf16 engines: encoder fc2 weights chunk-major [48][384][32] for mlp_fused.hip
  DevBuf qself;                                   // f32 [26][384]

  // workspaces
  std::vector<std::unique_ptr<DevBuf>> craft_ws_set[2];   // per-layer activations; [1]: the second detector lane's (tn.craft_lanes)
  enum { kWsKindMask = 7, kWsZeroedOnce = 8 };
  std::vector<uint8_t> craft_ws_meta[2];          // per slot of the set, as ws() last handed it out: its BufKind, | kWsZeroedOnce for a zero_new slot (host bookkeeping of the poison hook)
  int ws_sel = 0;                                 // which set ws() hands out
  std::vector<std::unique_ptr<DevBuf>>& craft_ws_cur() { return craft_ws_set[ws_sel]; }
  // tn.craft_lanes = 2: a batch's CRAFT launch groups alternate between the main stream and lane_stream, the second lane half a group behind the first
  // (lane_go: recorded by the first group once its full-resolution layers are through), so that one lane's matrix-bound first half runs beside the other's
  // HBM-bound U-Net tail; lane_done: the second lane's last CCL is enqueued (the main stream waits for it before the batch's closing events)
  hipStream_t lane_stream = nullptr;
  hipEvent_t lane_go = nullptr, lane_done = nullptr, resize_done = nullptr;
  bool lane_go_pending = false;                   // craft_forward_split records lane_go behind slice3.20 when set
  int craft_ws_npl = 0;                           // planes per value the split CRAFT workspaces were laid out for
  // launch groups (above): the configuration in force, and what the last batch / recogniser pass ran with (ttr_dbg_last_groups)
  CraftGroupCfg craft_group_cfg() const { return CraftGroupCfg{tn.first_fused && tn.craft_products != 4 && tn.split_conv3p ? 1 : 0, tn.craft_products, tn.up_commute, tn.fc7_fold && !craft_tap_on ? 1 : 0}; }
  EncGroupCfg enc_group_cfg() const { return EncGroupCfg{tn.enc_fc2_pairs, tn.qkv_attn_split, tn.enc_ln_pairs, tn.sp_hidden16}; }
  int last_craft_group = 0, last_enc_group = 0;
  // the recogniser's workspaces, by what they hold (a group's pointers into them: PqWork, engine_parseq.cpp)
  enum PqWs { kWsPatches, kWsX, kWsT384, kWsTbig, kWsAtt, kWsKvmem, kWsKvcache, kWsTgt, kWsD384b, kWsD1536, kWsStepLogits,
              kWsLnPlanes, kWsBigPlanes, kWsAttPlanes, kWsDecPlanesA, kWsDecPlanesB, kWsDecPlanes1536, kWsDecPlanesSa, kWsCount };
  DevBuf pq_ws[kWsCount];
  template <typename U = void> U* pq_buf(PqWs i, size_t bytes) { pq_ws[i].ensure(bytes); return pq_ws[i].as<U>(); }
  DevBuf canvas, heat, staging_img, crops, rects_dev, coef_dev, logits, ar_logits, ids_dev, tokens;
  DevBuf orient_in, orient_cand, orient_side;     // word orientation: the twins' coef | rects | page firsts; their recogniser block; the side block (orient.hip)
  PinnedBuf h_orient_in[2]; SideCopy h_orient;    // ... per slot: staging of orient_in; the side block's host copy, [N] turn | [N][K] candidate conf | [pages] page turn
  static size_t orient_side_bytes(int N, int K, int pages) { return ((size_t)N * (K + 1) + pages) * 4; }
  DevBuf lines_in, lines_side;                    // text lines: the words' cuv | page firsts; the side block (lines.hip)
  PinnedBuf h_lines_in[2]; SideCopy h_lines;      // ... per slot: staging of lines_in; the side block's host copy, [N] line | [N] word | [pages] n_lines
  static size_t lines_side_bytes(int N, int pages) { return ((size_t)2 * N + pages) * 4; }
  DevBuf alts_side;                               // character alternatives: the side block (decode_alts.hip), [N][26][K] int32 ids | [N][26][K] f32 prob
  SideCopy h_alts;                                // ... its host copy
  struct AltOut { int* ids; float* prob; int k; };   // k: the block's alternatives per position, 0 = none
  static size_t alts_side_bytes(int N, int K) { return (size_t)N * 26 * K * 8; }
  AltOut alts_out(int N, int K) { alts_side.ensure(alts_side_bytes(std::max(N, 1), K)); return AltOut{alts_side.as<int>(), alts_side.as<float>() + (size_t)N * 26 * K, K}; }
  DevBuf lex_side, lex_part;                      // lexicon matching: the side block (lexicon.hip), [N][M] int32 idx | [N][M] f32 logp; the scorer's partials [N][chunks][M] idx | logp
  SideCopy h_lex;                                 // ... the side block's host copy
  // m: the block's matches per item, 0 = none; band >= 0: the fuzzy scorer under (band, gap) in the rigid one's place, edits [N][m] behind the two blocks
  struct LexOut { int* idx; float* logp; int* part_idx; float* part_logp; int m; int band = -1; float gap = 0.f; int* edits = nullptr; };
  static size_t lex_side_bytes(int N, int M, int band = -1) { return (size_t)N * M * (band >= 0 ? 12 : 8); }
  LexOut lex_out(int N, int M, int band = -1, float gap = 0.f) {
    N = std::max(N, 1);
    lex_side.ensure(lex_side_bytes(N, M, band));
    const size_t pe = lexicon_partial_entries(N, lex_v, M);
    lex_part.ensure(pe * 8);
    LexOut l{lex_side.as<int>(), lex_side.as<float>() + (size_t)N * M, lex_part.as<int>(), lex_part.as<float>() + pe, M};
    if (band >= 0) { l.band = band; l.gap = gap; l.edits = lex_side.as<int>() + (size_t)N * M * 2; }
    return l;
  }
  DevBuf wide_side;                               // wide words: the side block (wide.hip), [Wn][17] int32 cuts | [Wn][2048] u16 profile
  SideCopy h_wide;                                // ... the cuts' host copy (wide_cuts_bytes: the profile stays on the device)
  DevBuf curve_side;                              // curved words: the side block (curve.hip), [N] flag | [N][2] hb | [N][2][9] spine | [N][9][4] int64 knots
  SideCopy h_curve;                               // ... its host copy
  DevBuf tab_bits, tab_bitsT, tab_runs, tab_side; // tables: the two bitmaps and the run lists (workspaces), and the side blocks [pages][kTabSideInts] | [N][2] table, cell (tables.hip)
  SideCopy h_tab;                                 // ... the side blocks' host copy
  // selection marks (marks.hip): the bands' record slots and counters (workspaces), and the side blocks [pages][kMarkSideInts] | [N] item_mark.  The bitmaps are
  // the tables pass's (tab_bits / tab_bitsT), formed once per batch whichever of the two layers is on
  DevBuf mark_cand, mark_counts, mark_side;
  SideCopy h_mark;                                // ... the side blocks' host copy
  // barcodes (barcodes.hip): the lines' hit slots and counters (workspaces), and the side blocks [pages][kBcSideInts] | [N] item_barcode.  The bitmaps are the
  // tables pass's again, formed once per batch whichever of the three layers is on under one ink rule
  DevBuf bc_hits, bc_cnt, bc_side;
  SideCopy h_barcode;                             // ... the side blocks' host copy
  int64_t page_ink_passes = 0;                    // the ink passes page_ink_enqueue has enqueued for batches (ttr_dbg_page_ink_passes: one per batch, whichever layers are on)
  DevBuf tab_ink_h, tab_ink_rec;                  // local ink under tables (and ttr_ink_page): the horizontal sums [pages][Hcap][Wcap] uint32, the records [pages]
  DevBuf blocks_side;                             // text blocks: the side block (blocks.hip)
  SideCopy h_blocks;                              // ... its host copy
  DevBuf chars_map[2], chars_in, chars_side;      // character boxes: per slot the batch's region planes (a copy of ccl.tnorm); coef | page_of | turns | nchars; the side block (chars.hip)
  PinnedBuf h_chars_in[2]; SideCopy h_chars;      // ... per slot: staging of chars_in; the side block's host copy
  hipEvent_t chars_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // ... per slot: the planes are copied; char_cut_kernel has read them (created with the first chars batch)
  CclBatch ccl;
  PinnedBuf h_counters, h_cand, h_rows, h_rects_f, h_rects[2], h_coef[2], h_ids[2];   // (h_coef: crop_mode = TTR_CROP_RECTIFIED only)   // pinned staging of the small host <-> device transfers
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float stage_ms[4] = {0, 0, 0, 0};
  float host_us[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // host wall-clock splits of the last run_pages (ttr_last_host_us)
  static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  // optional per-launch timing of the igemm kernel (bench.py's roofline): events bracket every launch
  int profiling = 0;                                   // 0 off, 1 = CRAFT conv launches only, 2 = every conv / GEMM launch
  int prof_stage = 0;                                  // 0 = CRAFT convs, 1 = PARSeq encoder (ViT) + batched decoder GEMMs, 2 = per-step AR decoder GEMMs
  std::vector<hipEvent_t> prof_pool;
  // Every timed launch carries its KIND (which kernel family / which layer role), its ALGORITHMIC flops (2 x MACs of the layer: the figure
  // SURVEY.md section 8(d) prices the roofline with) and the flops the matrix cores EXECUTE for it (x 3 or x 4 in the split-operand mode).
  struct ProfRec { int stage; int kind; double alg, exec; int launches; double bytes = 0; };
  struct ProfKind { std::string name; int stage = 0; double ms = 0, alg = 0, exec = 0; long launches = 0; double bytes = 0; };   // bytes: ALGORITHMIC HBM bytes (every operand read once, every result written once), 0 = not tallied
  std::vector<ProfKind> prof_kinds;
  std::map<std::string, int> prof_kind_ids;
  int kind_id(const char* name) {   // (a kind is a name in a stage: the decoder's linears run in the batched stage and in the AR steps)
    const std::string key = std::string(name) + "#" + std::to_string(prof_stage);
    auto it = prof_kind_ids.find(key);
    if (it != prof_kind_ids.end()) return it->second;
    const int id = (int)prof_kinds.size();
    prof_kinds.push_back(ProfKind{name, prof_stage});
    prof_kind_ids[key] = id;
    return id;
  }
  bool seg_open = false;                               // profiling == 1: an event pair brackets a RUN of consecutive CRAFT conv launches of one kind
  int seg_kind = -1;                                   // (an event record between two kernels costs ~8 us of idle GPU)
  double seg_alg = 0, seg_exec = 0, seg_bytes = 0; int seg_launches = 0;
  std::vector<ProfRec> prof_recs;
  double prof_ms[3] = {0, 0, 0}, prof_flops[3] = {0, 0, 0};
  long prof_launches[3] = {0, 0, 0};

  template <class F> void timed(const char* kind, double alg_flops, double exec_flops, F&& launch, double alg_bytes = 0) {
    if (!profiling || (profiling == 1 && prof_stage != 0)) { launch(); return; }
    const int k = kind_id(kind);
    if (profiling == 1) {   // the timed region of bench.py: one event pair per run of same-kind convolutions, closed by the next kind or by prof_break()
      if (seg_open && seg_kind != k) prof_break();
      const size_t i = prof_recs.size();
      while (prof_pool.size() < 2 * (i + 1)) { hipEvent_t e; TTR_HIP_CHECK(hipEventCreate(&e)); prof_pool.push_back(e); }
      if (!seg_open) { TTR_HIP_CHECK(hipEventRecord(prof_pool[2 * i], stream)); seg_open = true; seg_kind = k; seg_alg = seg_exec = seg_bytes = 0; seg_launches = 0; }
      launch();
      seg_alg += alg_flops; seg_exec += exec_flops; seg_bytes += alg_bytes; ++seg_launches;
      return;
    }
    const size_t i = prof_recs.size();
    while (prof_pool.size() < 2 * (i + 1)) { hipEvent_t e; TTR_HIP_CHECK(hipEventCreate(&e)); prof_pool.push_back(e); }
    TTR_HIP_CHECK(hipEventRecord(prof_pool[2 * i], stream));
    launch();
    TTR_HIP_CHECK(hipEventRecord(prof_pool[2 * i + 1], stream));
    prof_recs.push_back(ProfRec{prof_stage, k, alg_flops, exec_flops, 1, alg_bytes});
  }
  void prof_break() {       // call before any kernel that is not a CRAFT convolution, and at the end of CRAFT
    if (!seg_open) return;
    TTR_HIP_CHECK(hipEventRecord(prof_pool[2 * prof_recs.size() + 1], stream));
    prof_recs.push_back(ProfRec{0, seg_kind, seg_alg, seg_exec, seg_launches, seg_bytes});
    seg_open = false;
  }
  void igemm(const ConvParams& p, double true_flops, const char* kind = "igemm");
  // split-operand engines: the layer as four f16 MFMAs per product (gemm2.hip, SP) when its shape allows; the fp32 inputs
  // are written as planes first (split_ops.hip)
  std::map<const void*, const Linear*> split_by_w;   // fp32 weight pointer -> its Linear (the one with the planes)
  DevBuf split_in[2];
  bool split_gemm(const ConvParams& p, double true_flops, const char* kind);
  void prof_break_if_craft() { if (prof_stage == 0) prof_break(); }
  // Folds the records whose events have completed (one stream: they complete in order).  With streamed batches the newest records
  // belong to a pass that is still running: they stay, with their events, for the next call.
  void prof_collect();

  // ---- construction
  void upload_linear(Linear& L, const float* w, int cout, int k, const float* bias, int cout_pad, int k_pad,
                     const std::vector<int>* kmap = nullptr, bool own = true);
  void tile_planes(Linear& L);   // L.ws -> L.wst (gemm_sp.hip's contiguous loader pieces)
  bool drop_w1 = false;          // (experiment, load_craft: the weight planes' low parts as zeros)
  void upload_f32(DevBuf& d, const float* p, size_t n);

  static const std::vector<CraftConv>& craft_convs() {
    static const std::vector<CraftConv> v = {
        {"slice1.0", 3, 64, 3, 1},     {"slice1.3", 64, 64, 3, 1},    {"slice1.7", 64, 128, 3, 1},   {"slice1.10", 128, 128, 3, 1},
        {"slice2.14", 128, 256, 3, 1}, {"slice2.17", 256, 256, 3, 1}, {"slice3.20", 256, 256, 3, 1}, {"slice3.24", 256, 512, 3, 1},
        {"slice3.27", 512, 512, 3, 1}, {"slice4.30", 512, 512, 3, 1}, {"slice4.34", 512, 512, 3, 1}, {"slice4.37", 512, 512, 3, 1},
        {"slice5.1", 512, 1024, 3, 6}, {"slice5.2", 1024, 1024, 1, 1},
        {"upconv1.0", 1536, 512, 1, 1}, {"upconv1.3", 512, 256, 3, 1}, {"upconv2.0", 768, 256, 1, 1}, {"upconv2.3", 256, 128, 3, 1},
        {"upconv3.0", 384, 128, 1, 1},  {"upconv3.3", 128, 64, 3, 1},  {"upconv4.0", 192, 64, 1, 1},  {"upconv4.3", 64, 32, 3, 1},
        {"conv_cls.0", 32, 32, 3, 1},   {"conv_cls.2", 32, 32, 3, 1},  {"conv_cls.4", 32, 16, 3, 1},  {"conv_cls.6", 16, 16, 1, 1},
        {"conv_cls.8", 16, 2, 1, 1}};
    return v;
  }

  void load_craft(const std::string& dir);

  // Row order of the qkv weight for the fused qkv + attention launch: row n = 192 h + c of the head-major matrix is tile channel c of head h,
  // c = 96 wn + 32 t + dd -> Q (t = 0), K (t = 1), V (t = 2), d = 32 wn + dd; upstream (timm) row = 384 t + 64 h + d
  static int qkv_tile_row(int n) {
    const int h = n / 192, c = n % 192, wn = c / 96, t = (c % 96) / 32, dd = c % 32;
    return 384 * t + 64 * h + 32 * wn + dd;
  }

  void load_head_tail(WeightFile& wf);
  void load_fc7_fold(WeightFile& wf);   // the derived layers "upconv1.0.fold" / "upconv1.0.skip" (tn.fc7_fold)
  void load_parseq(const std::string& dir);

  bool verbose = false;
  // ---- range guard of the split-operand mode (split.h: RangeWatch; kernels.h: range_ctx)
  // One sticky word PER STAGE AND SLOT (a word = 0, or the tag of the first layer whose planes left the f16 range): with streamed batches the detector of batch j
  // (main stream) and the recogniser of batch j - 1 (recog_stream) are on the GPU together, and a word shared by both blamed the wrong batch.  A word is copied to
  // its host slot and cleared by the stream that wrote it, right behind the kernels that could set it; the detector's is verified in detect_collect, before the
  // batch's boxes are used, the recogniser's in finish.
  enum { kRangeDet0 = 0, kRangeDet1 = 1, kRangeRec0 = 2, kRangeRec1 = 3, kRangeStage = 4, kRangeWords = 8 };
  DevBuf range_word;                               // [kRangeWords] device words
  PinnedBuf h_range;                               // [kRangeWords] host copies
  std::vector<std::string> range_names;            // tag - 1 -> layer name
  std::map<std::string, unsigned> range_ids;
  std::string range_scope;                         // prefix of the tags sgemm() forms from its profile kinds ("encoder.blocks.3.", "decoder.")
  unsigned* range_flag_ptr(int w = kRangeStage) { return prec == kSplit && tn.range_guard ? range_word.as<unsigned>() + w : nullptr; }
  void range_use(int w) { range_ctx().flag = range_flag_ptr(w); }   // this thread's launches from here on watch word w
  void range_tag(const std::string& layer);        // names the layer whose launches follow (this thread's range_ctx().tag)
  void range_fetch(int w);                         // on `stream`, behind the kernels that watch word w: its copy to the host, then its clear
  void range_verify(int w, const char* where);     // after the sync that covers the copy: a tripped word fails the call (or warns)
  // ---- multi-GPU (ttr_engine_attach_comm): every batch's token ids are all-gathered on the stream, device buffer to device buffer
  Comm* comm = nullptr;
  DevBuf gath_dev[2];
  PinnedBuf h_gath[2];
  struct Gathered { int world = 0, pages = 0; std::vector<int32_t> counts, ids; std::vector<float> prob, conf; } last_gathered;
  // small host buffers of every rank, concatenated by rank (also the barrier): staged through device memory on the copy stream
  void allgather_host(const void* mine, size_t bytes, void* all);
  Engine(const std::string& dir, const ttr_config& c);
  ~Engine();

  // ---- CRAFT
  DevBuf& ws(size_t idx, size_t bytes, bool zero_new = false, BufKind kind = kElF16);

  void conv(const char* name, const void* in0, int C0, const void* in1, int C1, int relu0, int B, int H, int W, void* out, int act,
            float* out_f32 = nullptr, void* out_relu = nullptr, void* out_pool = nullptr, int pool_relu = 0);

  // canvas u8 [B][H][W][3] (device) -> heat f32 [B][H/2][W/2][2] (device)
  void craft_forward(const uint8_t* d_canvas, int B, int H, int W, float* d_heat);


  // ---- CRAFT, split-operand engines: every tensor between the convolutions lives as f16 planes ([pixel][x0 | x1 | x2], 6 bytes per
  // value); the convolutions' epilogues write them (bias, ReLU, ReLU copy, 2x2 max-pool fused), so no fp32 tensor and no separate
  // split pass exists up to the 32-channel head, which stays on the fp32 MFMA kernel (thin layers: 3 % of the FLOPs).
  void upconv_commuted(const char* name, const void* y_lo, int C0, const void* skip, int C1, int B, int H, int W, float* z, void* out);
  // upconv1.0 with slice5.1 and slice5.2 folded into it (tn.fc7_fold): z = W_skip . relu5_3 (fp32, no bias), out = ReLU(conv3x3_dil6(mp; Wf) + bf + z)
  void fc7_folded(const void* mp, const void* skip, int B, int H, int W, float* z, void* out);
  const uint8_t* sconv_canvas = nullptr;   // set around the sconv of slice1.3: its input tensor does not exist, conv1_1 is evaluated from this canvas inside the kernel (tn.first_fused)
  void sconv(const char* name, const void* in0, int C0, const void* in1, int C1, int B, int H, int W, void* out, int act,
             void* out_relu = nullptr, void* out_pool = nullptr, int pool_relu = 0, int out_planes = -1, int out_ld = 0, bool packed = false, float* tail_heat = nullptr);
  void craft_forward_split(const uint8_t* d_canvas, int B, int H, int W, float* d_heat);
  // Developer tap on the split detector (ttr_dbg_craft_taps): with craft_tap_on, every launch of craft_forward_split notes where its tensors live - each one
  // already has a workspace slot of its own, so nothing is copied and no kernel is added; the records are read after a stream synchronise and hold until the
  // engine's next forward pass.  Off (the default), tap() returns at once: same launches, same bits.
  enum { kTapF32 = 0, kTapPacked = 1, kTapPairs = 2, kTapTriples = 3, kTapU8 = 4 };   // CraftTap::form (packed pairs: pixel rows [x0 (32) | x1 (32)])
  struct CraftTap {
    std::string layer, role, kind;   // role: "in0", "in1", "out", "out_relu", "out_pool", "z", "heat"; kind: the kernel that ran (outputs only)
    const void* p; int B, H, W, C, ld, form;   // C real channels of a pixel row of ld channels
  };
  bool craft_tap_on = false;
  std::vector<CraftTap> craft_taps;
  std::vector<CraftTap> craft_fold_taps;   // the folded upconv1.0 launches of a tapped pass (roles in0 = mp, in1 = relu5_3, z, out): a list of their own, craft_taps keeps the three original layers' records
  void tap(const char* layer, const char* role, const void* p, int B, int H, int W, int C, int ld, int form, const char* kind = "") {
    if (craft_tap_on && p) craft_taps.push_back(CraftTap{layer, role, kind, p, B, H, W, C, ld, form});
  }

  // ---- PARSeq
  // split-operand linear on planes: in [M][3 K] -> out (planes [M][3 out_ld] or fp32 [M][out_ld]) and / or out_f32 (+ fp32 residual)
  void sgemm(const Linear& L, const void* in_planes, int M, void* out, int out_ld, int act, int out_planes,
             float* out_f32 = nullptr, int out_f32_ld = 0, const float* resid = nullptr, int resid_ld = 0, int np = 4, int resid_mod = 0, int out_full_cols = 0,
             const char* kind = nullptr, int x_tiled = 0, int out_tiled = 0);
  // out = L(LayerNorm(x)) for the decoder's per-step rows: the skinny GEMM normalises its own activation rows (bf16, few rows);
  // otherwise the LayerNorm kernel writes `scratch` and the plain GEMM follows
  void ln_gemm(const float* x, const std::string& ln_name, float eps, void* scratch, const Linear& L, int M, void* out, int out_ld, int act,
               float* out_f32 = nullptr, int out_f32_ld = 0);
  void gemm(const Linear& L, const void* in, int M, void* out, int out_ld, int act, float* out_f32 = nullptr, int out_f32_ld = 0,
            const float* resid = nullptr, int resid_ld = 0, int resid_mod = 0);
  // AR early exit: while set, the decoder's per-step launches carry the batch's done counter (ConvParams::skip); only the skinny
  // GEMM and the per-row attention kernels honour it, which are the ones the bf16 AR steps use
  const int* cur_skip = nullptr; int cur_skip_n = 0;
  DevBuf ar_done;
  PinnedBuf h_ar_done;
  bool streaming_recog = false;   // set around the recogniser of a STREAMED batch: no host-side wait there (the stream holds the next batch's detector)
  size_t kvcache_zeroed = 0;
  void ln(const float* x, const std::string& name, float eps, void* out, int M);

  // The decoder tail of the split-operand engines: the same layers as decoder_tail() below, handing each other f16 planes (split.h) instead of
  // fp32 tensors + split passes - 13 launches per AR step instead of 20.  sa: planes [rows][3 * 384] (self-attention output).
  void decoder_tail_split(const void* sa, int N, int R, const float* resid_pos, int resid_mod, float* tgt, void* pa, void* pb, void* p1536, float* q384,
                          void* t384, const void* kvmem, float* logits_out, int logits_ld, const int* done_tok = nullptr, int done_col = 0);

  // decoder tail shared by the AR steps (R = 1) and the refinement pass (R = 26):
  // sa T [rows][384] -> logits f32 (row stride logits_ld)
  void decoder_tail(const void* sa, int N, int R, const float* resid_pos, int resid_mod, float* tgt, void* t384, void* t384b, void* t1536,
                    const void* kvmem, float* logits_out, int logits_ld, const int* done_tok = nullptr, int done_col = 0);

  // The recogniser's outputs of `rows` crops share one device buffer (ids_dev), laid out [rows][26] ids | [rows][26] prob | [rows] conf, so that
  // one device-to-host copy and one collective carry all three.  Ensures the buffer (never inside a launch function).
  struct RecOut {
    int* ids; float* prob; float* conf;
    RecOut at(size_t row) const { return RecOut{ids + row * 26, prob + row * 26, conf + row}; }   // the block's rows from `row` on
  };
  static constexpr int kRecWords = 26 + 26 + 1;   // 4-byte words per crop
  static constexpr int kLogitWords = 26 * 95;     // 4-byte words of a crop's logits
  static constexpr int kCropBytes = 32 * 128 * 3; // bytes of a crop: 32 x 128 RGB
  RecOut rec_out(int rows) { return rec_block(ids_dev, rows); }
  static RecOut rec_block(DevBuf& d, int rows) {
    d.ensure((size_t)std::max(rows, 1) * kRecWords * 4);
    int* b = d.as<int>();
    return RecOut{b, reinterpret_cast<float*>(b + (size_t)rows * 26), reinterpret_cast<float*>(b + (size_t)rows * 52)};
  }
  // One recogniser pass, everything on the device.  Reads `crops` u8 [N][32][128][3]; writes `logits` f32 [N][26][95], the AR steps' logits `ar` (same
  // shape; null = not kept) and `out`: ids i32 [N][26], prob f32 [N][26], conf f32 [N].  What constrains it travels with it, by value:
  //   mask / row_masks  the character set (DESIGN.md "Character sets"): every crop chooses its tokens under `mask`, or - row_masks not null ([N] RowMask;
  //                     DESIGN.md "Regions and per-row character sets") - crop n under row_masks[n]
  //   alt               (DESIGN.md "Character alternatives") with alt.k set and both blocks given ([N][26][k]), decode_alts_kernel runs behind the final decode
  //   lex               (DESIGN.md "Lexicon matching") with lex.m set and the blocks given (idx / logp [N][m], the partials as lex_out sizes them for these N
  //                     crops), the scorer and its merge run behind the final decode, on the engine's word list
  //   pat               (DESIGN.md "Patterns") the call's table; an empty one (delta null) = the engine's own pattern, or none
  //   best              (DESIGN.md "Patterns", best mode) with best.logp given and a pattern in force, the final decode is launch_decode_conf into best.id0 /
  //                     prob0 / conf0 and launch_pattern_best; best.ext: the rows' extents in the call's table (the engine's own pattern: parseq_forward's to fill in)
  struct RecPass {
    const uint8_t* crops = nullptr; int N = 0;
    float *logits = nullptr, *ar = nullptr;
    RecOut out{};
    ClassMask mask{}; const RowMask* row_masks = nullptr;
    AltOut alt{}; LexOut lex{}; PatDev pat{}; PatBestOut best{};
    bool with_alts() const { return alt.k && alt.ids && alt.prob; }
    bool with_lex() const { return lex.m && lex.idx && lex.logp; }
    // the same pass over rows [r0, r0 + n): every per-row pointer moves by its own width (rows are never permuted: a row's crop, mask, start state and
    // outputs share its index), null stays null; the mask, the pattern's tables and the lexicon's partials (passes run one after another on the stream) are shared
    RecPass rows(int r0, int n) const {
      auto at = [r0](auto* p, size_t width) { return p ? p + (size_t)r0 * width : nullptr; };
      RecPass g = *this;
      g.N = n;
      g.crops = at(crops, kCropBytes); g.logits = at(logits, kLogitWords); g.ar = at(ar, kLogitWords);
      g.out = out.at(r0);
      g.row_masks = at(row_masks, 1);
      g.alt.ids = at(alt.ids, 26 * (size_t)alt.k); g.alt.prob = at(alt.prob, 26 * (size_t)alt.k);
      g.lex.idx = at(lex.idx, lex.m); g.lex.logp = at(lex.logp, lex.m); g.lex.edits = at(lex.edits, lex.m);
      g.pat.start_of = at(pat.start_of, 1);
      g.best.id0 = at(best.id0, 26); g.best.prob0 = at(best.prob0, 26); g.best.conf0 = at(best.conf0, 1); g.best.logp = at(best.logp, 1);
      g.best.ext.extent_of = at(best.ext.extent_of, 2);
      return g;
    }
  };
  // A batch of more than 4096 crops goes through in even groups (rows()); each group is parseq_group: the four steps below, which hand each other the
  // group's workspaces (PqWork, engine_parseq.cpp).  parseq_decode is also the whole of the decode stage calls (a pass over logits alone): the pattern or
  // confidence decode, then the alternatives, then the lexicon - under pass.pat as it stands (the engine's own pattern is parseq_forward's to fill in)
  struct PqWork;
  void parseq_forward(const RecPass& pass);
  void parseq_group(const RecPass& p);
  void parseq_encode(const RecPass& p, PqWork& w);
  void encoder_split(int N, PqWork& w);   // the 12 blocks and the final norm on planes (split-operand engines) ...
  void encoder_plain(int N, PqWork& w);   // ... and on T tensors (bf16, fp32)
  bool enc_split() const { return prec == kSplit && tn.split_gemm && tn.split_planes; }
  bool dec_split() const { return enc_split() && tn.dec_planes; }   // the decoder's layers hand each other planes (decoder_tail_split)
  DecArParams dec_ar_params(const RecPass& p, const PqWork& w);
  void parseq_ar(const RecPass& p, PqWork& w);
  void parseq_refine(const RecPass& p, PqWork& w);
  void parseq_decode(const RecPass& p);
  // the host's view of such a block of `rows` rows, as it lands in h_ids[slot] or as rank r's share of h_gath[slot]
  struct RecRows { const int32_t* ids; const float* prob; const float* conf; };
  static RecRows rec_rows(const void* block, int rows) {
    const int32_t* b = static_cast<const int32_t*>(block);
    return RecRows{b, reinterpret_cast<const float*>(b + (size_t)rows * 26), reinterpret_cast<const float*>(b + (size_t)rows * 52)};
  }
  // word orientation: candidate turns per word (1 = off, 2 = {0, 2}, 4 = {0, 1, 2, 3})
  int orient_k() const { return cfg.orient == TTR_ORIENT_QUARTER ? 4 : cfg.orient == TTR_ORIENT_FLIP ? 2 : 1; }

  // ---- post-processing of one page's heat map: GPU CCL + host calipers
  struct PageBoxes { std::vector<RRect> det; };

  // CCL kernels of pages [p0, p0 + pages) of a batch of `total` pages, then their component counters -> host; group `g`'s event
  // fires when the counters have landed
  void ccl_launch(const float* d_heat, int p0, int pages, int total, int g, int H2, int W2, int lane = 0);
  // boxes of pages [p0, p0 + pages): waits for the group's counters, pulls candidates + row extremes over on the copy stream
  // (the main stream may already be running the next group's CRAFT), then the host calipers
  void ccl_collect(int p0, int pages, int g, int H2, int W2, std::vector<std::vector<RRect>>& det);
  // run f(page) for every page on the engine's host threads
  void parallel_pages(int pages, const std::function<void(int)>& f) { host_pool->run(pages, f); }

  // ---- the hot path over a batch of same-sized device pages, in four phases so that several batches can be in flight:
  //   detect_enqueue   resize + CRAFT + CCL kernels of a batch on the stream
  //   detect_collect   host: wait for each CRAFT group's components, calipers -> boxes -> crop rectangles
  //   recog_enqueue    crop rectangles -> packer -> PARSeq -> token ids back (stream)
  //   finish           wait, decode the ids per page
  // run_pages runs them in that order for one batch.  stream_push(j) runs detect_enqueue(j), recog_enqueue(j-1), detect_collect(j),
  // finish(j-2): the stream holds C(j) P(j-1) behind whatever is running, so the GPU works through the previous batch's recogniser
  // while the host turns batch j's components into boxes, and still has a whole recogniser queued while the host decodes batch j-2,
  // returns to the caller and comes back with batch j+1 — no GPU idle at any hand-over; one stream, every kernel still runs alone.
  // Host staging (crop rectangles, token ids) and the completion events exist twice (slot = batch parity).
  // A page of a batch by itself: where it lives on the device, its size and row stride, and its geometry on the batch's canvas.
  struct Page { const uint8_t* data = nullptr; int h = 0, w = 0, stride = 0; CanvasGeom g{}; };
  struct PageBatch {
    const uint8_t* d_pages = nullptr; int n = 0, h = 0, w = 0;   // a uniform batch as its entry point passed it: n pages of h x w, contiguous
    bool mixed = false;                // the pages came one by one (ttr_page) and may differ in size and stride: the table kernels run (DESIGN.md "Mixed-size batches")
    std::vector<Page> pages;           // [n] every page by itself; filled by detect_enqueue from the scalars above for a uniform batch
    int H = 0, W = 0, H2 = 0, W2 = 0;  // the canvas all pages share
    struct Extent { int h = 0, w = 0; };   // the tallest and the widest page: what the page layers' per-page workspaces are sized and strided by
    Extent extent() const { Extent e; for (const Page& P : pages) { e.h = std::max(e.h, P.h); e.w = std::max(e.w, P.w); } return e; }
    std::vector<std::vector<RRect>> boxes;
    std::vector<int> rects, page_of;
    std::vector<int64_t> coef;         // crop_mode = TTR_CROP_RECTIFIED: {kind, X0, Ax, Bx, Y0, Ay, By, 0} per crop, beside rects
    std::vector<int64_t> twin;         // orient != 0: {1, X0, Ax, Bx, Y0, Ay, By, 0} of the (K - 1) N twin crops, candidate-major (row (j - 1) N + c)
    int N = 0, slot = 0, group = 16;
    // wide words (plan_wide; DESIGN.md "Wide words"): with wide_aspect != 0, rects / coef (and row_masks, when not empty) hold N + X rows - the pieces 1..n - 1 of
    // all wide items behind the batch's N, in (item, piece) order; wide_of[c] = the item's entry of `wide`, or -1
    float wide_aspect = 0.f;
    int X = 0;
    std::vector<WideWord> wide;
    std::vector<int32_t> wide_of;
    // curved words (plan_curved; DESIGN.md "Curved words"): with `curved`, one entry per crop - its frame, page and row
    bool curved = false;
    std::vector<CurveIn> curve;
    // tables (DESIGN.md "Tables"): the engine's setting when the boxes were made (0 = off, and for region calls), and 64 x every word's centre [N][2]
    int tab_min_len = 0, tab_ink = 0;
    std::vector<int32_t> tab_centres;
    // selection marks (DESIGN.md "Selection marks"): the engine's setting when the boxes were made (mark_min 0 = off, and for region calls); they share the centres
    int mark_min = 0, mark_max = 0, mark_fill = 0, mark_ink = 0;
    // barcodes (DESIGN.md "Barcodes"): likewise (bc_min 0 = off, and for region calls)
    int bc_min = 0, bc_ink = 0, bc_sym = 0;
    std::vector<DeskewRec> dsk_recs;   // deskew: the pages' records as the device wrote them (detect_collect_local takes them from the slot's pinned copy)
    // local ink (DESIGN.md "Local ink"): the engine's setting when the detector was enqueued (radius 0 = off), and the records of the deskew pass, taken with dsk_recs
    int ink_radius = 0, ink_drop = 0, ink_polarity = 0;
    std::vector<InkRec> dsk_ink_recs;
    int dsk_M = 0;                     // deskew: max_slope when the detector was enqueued (0 = off, and for region calls); the pages of the batch are then upright copies
    int tiles = 0;                     // tiled pages: tiles per page (0 = the engine's tiling was off when the detector was enqueued), and their plan
    TilePlan plan{};
    int det_groups = -1;               // CCL groups enqueued for it (group_ev[det_groups]: behind the copy of its detector range word)
    bool live = false, enqueued = false;
    std::vector<int32_t> all_counts;   // with a communicator: crops per page of every rank [world][n]
    int cap = 0;                       // ... and the largest rank total (rows of the gathered payload per rank)
    int rows = 0;                      // rows of the recogniser's output block (RecOut) staged in h_ids[slot]: max(N, cap)
    int alts = 0;                      // the engine's `alts` when the recogniser was enqueued: h_alts's copy of the slot holds [N][26][alts] ids | prob
    bool pat_best = false;             // patterns in best mode, fixed when the recogniser was enqueued with a pattern in force: h_pat_logp's copy of the slot holds [N] f32
    int lex_m = 0;                     // the engine's `lex_m` when the recogniser was enqueued with a lexicon set (0 = none): h_lex's copy of the slot holds [N][lex_m] idx | logp
    int lex_band = -1;                 // ... and the engine's `lex_band` then (-1 = the rigid scorer): >= 0, [N][lex_m] int32 edits follow the two blocks
    // regions (run_regions; DESIGN.md "Regions and per-row character sets"): the boxes are the caller's quads - no detector ran, `boxes` stays empty, every crop is
    // a kind-1 crop of the table packer.  Crop c (page order, then the caller's order): its quad verbatim, its set index, and - when the sets differ - its row
    // of the class-mask table ({blocked[3], 0}); row_masks empty = every crop reads under region_mask, by value
    bool regions = false;
    std::vector<float> region_quad;    // [N][8]
    std::vector<int32_t> region_set;   // [N]
    std::vector<uint32_t> row_masks;   // [N][4], or empty
    ClassMask region_mask{};
    PatRows region_pats;               // the regions' patterns in crop order (DESIGN.md "Patterns"); start_of empty = none
  };
  PageBatch q1, q2;        // streamed batches: q1 = boxes known (recogniser enqueued or not), q2 = older, recogniser enqueued, results not yet returned

  void detect_enqueue(PageBatch& B);
  // tiled pages: the tiles of every page of B (B.plan's windows, each page's own extents) as rows of the slot's tile table, one copy on `stream`
  void upload_tile_table(const PageBatch& B, int sl);
  // the stage forms: ttr_stitch_heat - host tile maps -> tile_heat, tile_stitch_kernel once, the page maps back; ttr_craft_heatmap_tiled - a host image under
  // overlap O (whatever the engine's setting): its tiles' canvases, CRAFT in launch groups, the stitch -> the page map [H2][W2][2] (cap: floats `out` holds)
  void stitch_heat(const float* tiles, int pages, const TilePlan& plan, float* out);
  void craft_heatmap_tiled(const uint8_t* img, int h, int w, int row_stride, int overlap, float* out, size_t cap, int* H2, int* W2, uint8_t* canvases_out, size_t canvases_cap);
  // CRAFT over nc canvases of H x W in launch groups (no CCL), on `stream`: the tiled path's detector; returns the group size
  int craft_groups_plain(const uint8_t* d_canvas, int nc, int H, int W, float* d_heat);
  // Mixed-size batches: the device page table of a batch (page_table.h), one per pipeline slot - the resize of batch j reads its table on the main stream while
  // the packers of batch j - 1 read theirs on the recogniser's.  upload_page_table writes the rows into the slot's pinned buffer and copies them once, on
  // `stream`, behind table_ev[sl] (recorded behind the last packer that read the slot's previous table; a no-op before the first).
  DevBuf page_table[2];
  PinnedBuf h_page_table[2];
  hipEvent_t table_ev[2] = {nullptr, nullptr};
  void upload_page_table(const std::vector<Page>& pages, int sl);
  // every page's size, stride and canvas geometry checked and filled in; throws today's messages, and refuses pages that do not share one canvas
  void check_pages(std::vector<Page>& pages) const;
  static PageBatch mixed_batch(const ttr_page* pages, int n);

  // With a communicator attached a batch is a collective: a {status, pages} header travels before anything whose size depends on the
  // ranks' inputs, so that a rank that failed in its detector (`pre`: what detect_enqueue threw; or the box extraction below) or passed
  // another page count makes the call fail on EVERY rank - instead of leaving the others inside a gather that never completes.
  void detect_collect(PageBatch& B, std::exception_ptr pre = nullptr);
  void detect_collect_local(PageBatch& B);

  void recog_enqueue(PageBatch& B);
  // wide words: plans every crop of B from quads [N][8] (the word's quad: deskew_quad's on page calls, the caller's on region calls) under the engine's `wide`;
  // appends the extra rows to rects / coef / row_masks and fills wide / wide_of / X.  Host only; a no-op with wide off.
  void plan_wide(PageBatch& B, const float* quads);
  // curved words: one CurveIn per crop of B from quads [N][8] (the quads plan_wide takes) under the engine's `curved`.  Host only; a no-op with curved off.
  void plan_curved(PageBatch& B, const float* quads);
  // The ink readers of a batch - tables, selection marks, barcodes (DESIGN.md "Adding a page layer").  batch_bits says which rule formed this batch's tab_bits /
  // tab_bitsT: none yet, the local one, or the fixed one under that threshold (1..255); batch_offsets_up, that a batch without words has its zero offsets on
  // the device.  recog_enqueue resets both.  page_ink_enqueue is the only place that decides on a pass: it returns when the bitmaps in place are those of the
  // rule asked for (the local one when the batch has a radius, else the fixed one under `ink`), else enqueues the pass - and with the local rule its records -
  // and counts it in page_ink_passes
  static constexpr int kBitsNone = -1, kBitsLocal = 0;
  int batch_bits = kBitsNone;
  bool batch_offsets_up = false;
  void page_ink_enqueue(const PageBatch& B, int sl, int ink);
  // what a reader's launches take of the batch: the extent its workspaces are sized by, the first page, the page table (mixed batches, else null), 64 x the
  // words' centres [N][2] and the pages' offsets [n + 1] behind them (for a batch without words: n + 1 zeros, uploaded by the first reader that asks)
  struct LayerBatch { int n, N, Hcap, Wcap; const Page& P0; const PageRow* table; const int* centres; const int* first; };
  LayerBatch layer_batch(const PageBatch& B, int sl);
  void layer_batch_done(const LayerBatch& L, int sl);   // behind a reader's last kernel: the page table's last reader of this batch so far
  // each reader's two kernels of batch B behind its packer, or - marks and barcodes, for a batch without words - on their own; a no-op with the layer off
  void tables_enqueue(const PageBatch& B, int sl);
  void marks_enqueue(const PageBatch& B, int sl);
  void barcodes_enqueue(const PageBatch& B, int sl);
  // the stage form (ttr_barcodes_page, and the developer hook): through table_ink_kernel, barcode_scan_kernel and barcode_page_kernel -> side [kBcSideInts],
  // item_barcode [nq], hits [(h + w) 2 8][20], cnt [(h + w) 2][4]
  void barcodes_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_lines, int ink, int symbologies, const float* quads, int nq,
                      int32_t* side_out, int32_t* item_out, int32_t* hits_out, int32_t* cnt_out);
  // The opening every one-page stage call shares.  stage_page: a host image (row_stride 0 = packed rows) checked under the caller's `what` - "bad image size",
  // a page side of side_cap px or more (0 = no cap), `bad_args` (the layer's own range refusal, null = in range), "bad device offset or stride" - then copied
  // dev_offset bytes into staging_img with dev_stride bytes from row to row (0 = 3 w), on `stream`; returns where it lies.  check = false: the caller has made
  // the image check under a text of its own.  stage_centres: host quads checked, 64 x their centres [nq][2] and the page's offsets {0, nq} -> rects_dev
  struct StagedPage { uint8_t* data; int stride; };
  StagedPage stage_page(const char* what, const uint8_t* img, int h, int w, int row_stride, int dev_offset = 0, int dev_stride = 0, int side_cap = 0,
                        const char* bad_args = nullptr, bool check = true);
  void stage_centres(const char* what, const float* quads, int nq);
  const PageRow* staged_page_table(const StagedPage& pg, int h, int w);   // ... and the staged page as the one row of slot 0's page table (the stage calls' use_table)
  // The ink readers' stage forms open and close alike.  stage_ink_page: stage_page under the 32768 px cap and the layer's refusal, stage_centres, the two
  // bitmaps under the fixed rule - with `zero`, a workspace of zero_b bytes zeroed ahead of the ink pass, for a hook that returns whole lists.  stage_side_home: the side block [ints] | items [nq][item_ints] and the `extra` arrays whose host pointer is set come home,
  // one sync; the layer's validator ("the side block holds ..."), the items' range check (noun set: each item is -1 or a record below side[1]); then side_out
  // gets the counted part - hdr + rec * side[1] ints, the rest zero - and items_out the items
  StagedPage stage_ink_page(const char* what, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, const char* bad_args, int ink,
                            const float* quads, int nq, DevBuf* zero = nullptr, size_t zero_b = 0);
  struct StageSide { const DevBuf* dev; int ints, hdr, rec, item_ints; const char* noun; };
  struct StageBack { void* host; const DevBuf* dev; size_t bytes; };
  void stage_side_home(const char* what, const StageSide& s, int nq, std::initializer_list<StageBack> extra, const std::function<bool(const int32_t*, std::string*)>& valid,
                       int32_t* side_out, int32_t* items_out);
  // the stage form (ttr_marks_page, and the developer hook): as tables_stage, through table_ink_kernel, mark_cand_kernel and mark_page_kernel -> side
  // [kMarkSideInts], item_mark [nq], counts [ceil(h / 32)][2]
  void marks_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_side, int max_side, int fill, int ink, const float* quads,
                   int nq, int32_t* side_out, int32_t* item_mark_out, int32_t* counts_out);
  // the stage form (ttr_tables_page, and the developer hook): a host image, placed dev_offset bytes into a device buffer with dev_stride bytes from row to row
  // (0 = 3 w), and host quads through table_ink_kernel and table_grid_kernel -> side [kTabSideInts], items [nq][2], bits [h][ceil(w / 64)], runs [2][8192][3]
  // deskew: ink, scores, choice and resampling of batch B's pages ahead of its resize, on `stream`; redirects B.pages to the slot's upright copies
  void deskew_enqueue(PageBatch& B);
  const int* deskew_consts_dev();     // the (C, S) table on the device (uploaded by the first call)
  // the stage form (ttr_deskew_page, and the tests): a host image, placed dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 w),
  // through the pixel pass and the two kernels -> out [h][w][3] (packed rows), the record, scores [2 max_slope + 1]; any may be null
  void deskew_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int max_slope, int gain, int ink, uint8_t* out,
                    DeskewRec* rec, uint64_t* scores);
  // local ink's stage form (ttr_ink_page, ttr_dbg_ink_page): a host image, placed as above, through ink_rows_kernel and ink_local_kernel -> bits
  // [h][ceil(w / 64)], bitsT [w][ceil(h / 64)], the record; any may be null
  void ink_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int radius, int drop, int polarity, uint64_t* bits_out,
                 uint64_t* bitsT_out, InkRec* rec);
  void tables_stage(const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_len, int ink, const float* quads, int nq, int32_t* side_out,
                    int32_t* items_out, uint64_t* bits_out, int32_t* runs_out);
  // the stage form (ttr_curve_crops): a host image and host quads through the kind-1 packer and curve_crop_kernel -> flag [nq], hb [nq][2], spine [nq][2][9],
  // knots [nq][9][4], crops [nq][32][128][3]
  void curve_crops(const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, bool use_table, int32_t* flag, int32_t* hb, int32_t* spine,
                   int64_t* knots, uint8_t* crops_out);
  // the stage form (ttr_wide_cuts): a host image and host quads through wide_cut_kernel -> n [nq], cuts [nq][17], profiles [nq][2048], coef [nq][16][8]
  void wide_cuts(const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, float max_aspect, bool use_table, int32_t* n_out, int32_t* cuts,
                 uint16_t* profiles, int64_t* coef);
  // the crop packer of a batch whose rects / coef are known: copies them through the pinned staging of slot sl and enqueues
  // pack_crops_kernel (crop_mode 0) or pack_crops_rect_kernel (crop_mode 1) into `crops`
  void pack_batch_crops(const PageBatch& B, int sl);
  // word orientation: the twins' coefficients, rects and the pages' first words through the pinned staging of slot sl (one copy), then
  // pack_crops_rect_kernel on the (K - 1) N twin rows into `crops` behind the batch's N crops
  void pack_twin_crops(const PageBatch& B, int sl);

  // text lines: the words' fixed-point c, u, v and the pages' first words into the pinned staging of slot sl (host only; returns the largest
  // word count of a page), then one copy of them, line_group_kernel into the side block and its copy to the host (h_lines)
  int stage_batch_lines(const PageBatch& B, int sl);
  void group_batch_lines(const PageBatch& B, int sl, int max_words);
  // the stage form (ttr_group_lines): host quads [first[pages]][8] of several pages -> line, word [first[pages]], n_lines [pages]
  void group_lines(const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines);
  // text blocks: block_group_kernel behind line_group_kernel of the same batch (it reads lines_in and lines_side on the device) and the copy of its
  // side block to the host (h_blocks); the stage form (ttr_group_blocks): both kernels on host quads, block / pos [first[pages]] indexed by line within
  // each page's range, n_blocks / mode [pages]; any output may be null.  blocks = false: the lines' kernel alone, under ttr_group_lines' name (group_lines)
  void group_batch_blocks(const PageBatch& B, int sl, int max_words);
  void group_blocks(const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block, int32_t* pos,
                    int32_t* n_blocks, int32_t* mode, bool blocks = true);

  // character boxes: detect_enqueue keeps the batch's region planes (keep_batch_map, behind its CCL); stage_batch_chars writes every word's coefficients
  // (all four turns when orientation is on) and page into the pinned staging of slot sl (host only); cut_batch_chars copies them, runs char_cut_kernel
  // behind the recogniser (K and the turn are read on the device) and copies the side block to the host (h_chars)
  void keep_batch_map(const PageBatch& B);
  void stage_batch_chars(const PageBatch& B, int sl);
  void cut_batch_chars(const PageBatch& B, int sl, const int* ids, const int* turns);
  // the stage form (ttr_char_cuts): a host map and host quads / turns / nchars through char_cut_kernel
  void char_cuts(const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars, int n,
                 int32_t* cuts, int32_t* modes, uint8_t* profiles);

  void finish(PageBatch& B, std::vector<Result>& results);
  // the host copies of a batch's side blocks as finish takes them from the SideCopy records (view(slot)): null = the layer did not run for the batch
  struct SideViews {
    const int32_t *orient = nullptr, *lines = nullptr, *blocks = nullptr, *chars = nullptr, *alts = nullptr, *lex = nullptr, *wide_cuts = nullptr, *curve = nullptr, *tab = nullptr, *mark = nullptr, *barcode = nullptr;
    const float* pat_logp = nullptr; const InkRec* tab_ink = nullptr;
  };
  // results[pg] for every page of B from its boxes, the decoded rows of its crops (crop c is row c) and the side blocks: one function per layer, run page by
  // page in the order below - later layers read what earlier ones wrote (blocks the lines, chars `quad` and `orient`, wide rewrites `text` and `conf`)
  struct PageCtx { const PageBatch& B; const RecRows& rows; const SideViews& V; int pg, c0, cnt; };   // page pg owns crops [c0, c0 + cnt)
  void decode_pages(const PageBatch& B, const RecRows& rows, const SideViews& views, std::vector<Result>& results);
  // words: ids, prob, conf, alternatives, lexicon matches, pattern_logp, orientation, text, bbox, quad; records: the page's skew and ink records
  void decode_words(const PageCtx&, Result&) const, decode_records(const PageCtx&, Result&) const, decode_tables(const PageCtx&, Result&) const,
      decode_marks(const PageCtx&, Result&) const, decode_barcodes(const PageCtx&, Result&) const, decode_curved(const PageCtx&, Result&) const, decode_wide(const PageCtx&, Result&) const,
      decode_lines(const PageCtx&, Result&) const, decode_blocks(const PageCtx&, Result&) const, decode_chars(const PageCtx&, Result&) const;

  // the stage entry points (ttr_craft_heatmap, ttr_parseq_logits, ...) share workspaces with the batches: with the recogniser of a streamed batch on a stream of
  // its own they would race with it
  void refuse_while_streaming(const char* what) const { if (q1.live || q2.live) throw std::runtime_error(std::string(what) + ": streamed batches are in flight: call ttr_stream_flush until it returns none"); }
  void run_pages(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& results);
  void run_pages_v(const ttr_page* pages, int n, std::vector<Result>& results);   // pages of different sizes and strides that share one canvas
  void run_batch(PageBatch& B, std::vector<Result>& results);
  // Regions (DESIGN.md "Regions and per-row character sets"): n caller-given quads on n_pages device pages of any sizes -> the packer and the recogniser, no
  // detector; synchronous.  Every refusal happens before anything is enqueued.
  void run_regions(const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets, std::vector<Result>& results,
                   const char* const* patterns = nullptr, int n_patterns = 0, const int32_t* pattern_of = nullptr);   // (pattern_of: one entry per region; DESIGN.md "Patterns")
  // set_of[n] (-1 = the engine's own set) over sets[n_sets][3] -> the rows' blocked-complement masks: `table` [n][4] when they differ, else empty and `one` = the
  // mask they share (the by-value path).  Refuses a set index out of range, a mask without bit 0 and - a row that restricts - a bf16 engine.
  void resolve_row_masks(const char* what, const int32_t* set_of, int n, const uint32_t* sets, int n_sets, std::vector<uint32_t>& table, ClassMask& one) const;
  // the table through the pinned staging of slot sl to row_masks_dev (one copy on `stream`); returns the device table, or null for an empty one
  const RowMask* stage_row_masks(const std::vector<uint32_t>& table, int sl);
  DevBuf row_masks_dev;
  PinnedBuf h_row_masks[2];
  // Patterns (DESIGN.md "Patterns").  set_engine_pattern: compiles src under the mask `cm` allows and, when it compiles, replaces the engine's pattern and
  // its device table (null or empty src: none); throws and changes nothing otherwise.
  void set_engine_pattern(const char* src, const ClassMask& cm);
  // a call's rows -> one table: row i reads under patterns[pattern_of[i]] (pattern_of null or -1: the engine's own pattern, or none), compiled under the row's
  // mask - row i of `table` ([n][4], blocked complements), or `one` when the table is empty.  Each distinct (pattern, mask) pair is compiled once.  Returns false
  // - nothing built - when no row has a pattern.  Refuses a bad index, a bad pattern (naming the row) and more than 1024 states in all (naming the total).
  bool resolve_row_patterns(const char* what, const char* const* patterns, int n_patterns, const int32_t* pattern_of, int n, const std::vector<uint32_t>& table,
                            const ClassMask& one, PatRows& out) const;
  // the call's table and start states through the pinned staging of slot sl to pat_rows_dev (one copy on `stream`); with `ext` given (best mode) the rows'
  // extents travel in the same copy and *ext names them - without it the bytes are the ones greedy mode always sent
  PatDev stage_row_patterns(const PatRows& r, int sl, PatExtent* ext = nullptr);
  DevBuf pat_rows_dev, pat_state;
  PinnedBuf h_pat_rows[2];

  // Latency mode (the reference's 6-thread fan-out over chunks of the crop batch, tuatara.cpp:450-485, across
  // GPUs): rank 0 detects and packs the crop batch, the batch is broadcast, rank r recognises the contiguous shard r of
  // ceil(N / world) crops, the ids are all-gathered, rank 0 decodes and returns the pages' results (the other ranks pass no pages and
  // return n empty results).  Collective over the engine's communicator.
  void run_pages_sharded(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& results);

  // Streamed form: returns the results of the batch pushed TWO calls earlier (prev_n = its page count, 0 for the first two pushes).
  // The pages of a batch must stay valid until its results have been returned (the crop packer reads them one push later).
  void stream_push(const uint8_t* d_pages, int n, int h, int w, std::vector<Result>& prev_results, int& prev_n);
  void stream_push_v(const ttr_page* pages, int n, std::vector<Result>& prev_results, int& prev_n);   // mixes freely with stream_push
  void push_batch(PageBatch&& B, std::vector<Result>& prev_results, int& prev_n);
  // results of the oldest batch in flight (prev_n = 0: none left)
  void stream_flush(std::vector<Result>& prev_results, int& prev_n);

  // ---- image_to_data over a LIST of host images of any sizes (the reference loads both models per call, tuatara.cpp:336, :428, and
  // takes one image per call): images of equal size travel together as batches of <= images_batch pages through the streamed path above.  Staging: four
  // pinned host buffers + four device buffers; a helper thread gathers batch j + 1's rows into its pinned buffer and starts its host-to-device copy on the
  // upload stream while the caller's thread is inside stream_push(j) - the detector of a batch waits for its pages' copy event, nothing else does.
  struct HostImage { const uint8_t* data; int h, w; std::ptrdiff_t row_stride; };
  static constexpr int kStageSlots = 4;   // a batch's pages must outlive its recogniser (two pushes later) while the helper fills the next slot
  PinnedBuf stage_host[kStageSlots];
  DevBuf stage_dev[kStageSlots];
  hipStream_t up_stream = nullptr;
  hipEvent_t up_ev[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  // results[i] = what run_pages returns for image i alone.  An unreadable entry (null / empty / short stride: the reference's "Error reading image from file",
  // tuatara.cpp:344-347) and every image of a batch that failed on the GPU (e.g. the range guard) keep an empty result and are listed in `failed` (input
  // indices; first_error: the first failure's message); everything else is delivered - what a loop over image_to_data does with one bad image.
  // cfg.mixed_batches = 1: the buckets are canvases (h32, w32) instead of sizes, every batch's images are staged one after another at offsets rounded up to
  // 256 bytes and run through the table path; an image whose geometry is invalid fails alone, before bucketing.
  void run_images(const std::vector<HostImage>& imgs, std::vector<Result>& results, std::vector<int>& failed, std::string& first_error);
  std::vector<int32_t> last_batches;   // pages per batch of the last run_images call, in run order (ttr_last_images_batches)

  // ---- the scratch rows of kDevBufTable above as this engine's buffers: f(name, buffer, kind) for each, in the table's order.  Per-slot exceptions to a row's
  // kind and class (craft_ws_set, pq_ws) are the poison hook's to apply (capi_debug.cpp), which also checks that the names visited are the table's scratch rows
  template <class F> void for_scratch(F&& f) {
    for (auto& set : craft_ws_set) for (auto& d : set) f("craft_ws_set", *d, kElF16);
    f("canvas", canvas, kElU8); f("heat", heat, kElF32); f("tile_heat", tile_heat, kElF32);
    for (auto& d : tile_table) f("tile_table", d, kElAddr);
    for (auto& d : page_table) f("page_table", d, kElAddr);
    f("staging_img", staging_img, kElU8);
    for (auto& d : stage_dev) f("stage_dev", d, kElU8);
    for (auto& d : split_in) f("split_in", d, kElF16);
    f("dsk_bits", dsk_bits, kElU8); f("dsk_bitsT", dsk_bitsT, kElU8); f("dsk_scores", dsk_scores, kElI32); f("dsk_rec", dsk_rec, kElI32);
    f("dsk_ink_h", dsk_ink_h, kElU8); f("dsk_ink_rec", dsk_ink_rec, kElI32);
    for (auto& d : dsk_table) f("dsk_table", d, kElAddr);
    for (auto& d : dsk_pages) f("dsk_pages", d, kElU8);
    f("ccl.tnorm", ccl.tnorm, kElF32); f("ccl.flags", ccl.flags, kElU8); f("ccl.parent", ccl.parent, kElI32); f("ccl.mm", ccl.mm, kElI32);
    f("ccl.area", ccl.area, kElI32); f("ccl.bbox", ccl.bbox, kElI32); f("ccl.maxt", ccl.maxt, kElI32); f("ccl.cand_slot", ccl.cand_slot, kElI32);
    f("ccl.cand", ccl.cand, kElI32); f("ccl.counters", ccl.counters, kElI32); f("ccl.rows", ccl.rows, kElI32); f("ccl.rects", ccl.rects, kElI32);
    f("ccl.cal_pool", ccl.cal_pool, kElF32); f("ccl.cal_ctr", ccl.cal_ctr, kElI32);
    f("crops", crops, kElU8); f("rects_dev", rects_dev, kElI32); f("coef_dev", coef_dev, kElI32);
    for (auto& d : pq_ws) f("pq_ws", d, kElF32);
    f("logits", logits, kElF32); f("ar_logits", ar_logits, kElF32); f("ids_dev", ids_dev, kElI32); f("tokens", tokens, kElI32);
    f("row_masks_dev", row_masks_dev, kElI32); f("pat_rows_dev", pat_rows_dev, kElI32); f("pat_state", pat_state, kElI32);
    f("pat_best_scratch", pat_best_scratch, kElI32); f("pat_logp_dev", pat_logp_dev, kElF32);
    for (auto& d : gath_dev) f("gath_dev", d, kElI32);
    if (comm) { f("comm.d_in", comm->d_in, kElU8); f("comm.d_out", comm->d_out, kElU8); }
    f("orient_in", orient_in, kElI32); f("orient_cand", orient_cand, kElI32); f("orient_side", orient_side, kElI32);
    f("lines_in", lines_in, kElI32); f("lines_side", lines_side, kElI32); f("alts_side", alts_side, kElI32);
    f("lex_side", lex_side, kElI32); f("lex_part", lex_part, kElI32); f("wide_side", wide_side, kElI32); f("curve_side", curve_side, kElI32);
    f("tab_bits", tab_bits, kElU8); f("tab_bitsT", tab_bitsT, kElU8); f("tab_runs", tab_runs, kElI32); f("tab_side", tab_side, kElI32);
    f("tab_ink_h", tab_ink_h, kElU8); f("tab_ink_rec", tab_ink_rec, kElI32);
    f("mark_cand", mark_cand, kElI32); f("mark_counts", mark_counts, kElI32); f("mark_side", mark_side, kElI32);
    f("bc_hits", bc_hits, kElI32); f("bc_cnt", bc_cnt, kElI32); f("bc_side", bc_side, kElI32);
    f("blocks_side", blocks_side, kElI32);
    for (auto& d : chars_map) f("chars_map", d, kElF32);
    f("chars_in", chars_in, kElI32); f("chars_side", chars_side, kElI32);
  }
  int stream_fail_age = 0;   // set by stream_push / stream_flush before they throw: 0 = the batch being pushed never entered the pipeline, 2 = the batch whose results were due failed and has left it
};

}  // namespace ttr

// ---- shared by the C ABI translation units
struct ttr_engine { std::unique_ptr<ttr::Engine> e; };
struct ttr_result { ttr::Result r; };
// the C ABI's hand-over of results[0, n) to the caller: out[i] owns results[i] (ttr_result_free)
void hand_out(std::vector<ttr::Result>& results, int n, ttr_result** out);

// Every entry point: the engine's lock, and the engine's device made current for the calling thread (HIP's current device is per
// thread: allocations, hipFuncSetAttribute and device queries inside the call must hit the device the stream belongs to).
struct EngineScope {
  std::lock_guard<std::mutex> lk;
  explicit EngineScope(ttr::Engine& E) : lk(E.mu) {
    TTR_HIP_CHECK(hipSetDevice(E.cfg.device));
    ttr::range_ctx().flag = E.range_flag_ptr(); ttr::range_ctx().tag = 0;   // this thread's launches belong to this engine until the scope ends
  }
  ~EngineScope() { ttr::range_ctx().flag = nullptr; ttr::range_ctx().tag = 0; }
};

#define TTR_GUARD_BEGIN try {
#define TTR_GUARD_END(rc)                                   \
  }                                                         \
  catch (const std::exception& ex) { ttr::g_last_error = ex.what(); return rc; } \
  catch (...) { ttr::g_last_error = "unknown error"; return rc; }

struct ttr_comm { std::unique_ptr<ttr::Comm> c; };
