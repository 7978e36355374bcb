/* Developer diagnostics of the MI355X tuatara engine: unit-test hooks for single kernels, micro-benchmarks, phase stamps and the
 * PROCESS-WIDE kernel-variant switches of the .hip files.  Not part of the drop-in surface (include/tuatara_hip.h); exported by
 * the same library so that tests/ and tools/ can reach the kernels without the whole pipeline. */
#ifndef TUATARA_HIP_DEBUG_H
#define TUATARA_HIP_DEBUG_H

#include "tuatara_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- debug / unit-test hook: one implicit-GEMM conv layer on host tensors ------------------- */
/* in f32 NHWC [B][H][W][C0] (+ optional in1 [..][C1] virtual concat), wgt f32 [Cout][ks][ks][C0+C1],
 * out f32 NHWC [B][H][W][Cout].  act: 0 none, 1 relu, 2 gelu. */
int ttr_dbg_conv(ttr_engine* e, const float* in0, int C0, const float* in1, int C1, int relu0, int relu1, int B, int H, int W,
                 int ks, int dil, const float* wgt, const float* bias, int Cout, int act, float* out);

/* bf16 engines: one conv layer (single source) with the 2x2 max-pool fused into its epilogue, as CRAFT's trunk uses it.
 * out_full (optional) f32 [B][H][W][Cout] and out_pool f32 [B][H/2][W/2][Cout] receive the bf16 results widened to f32. */
/* One split-operand linear layer of the f16x4 engine on its own: out[M][N] = act(x w^T + bias (+ resid)), np = 3 (activation pairs) / 4 (triples),
 * out_planes = 0 (fp32 from the kernel) / 2 / 3 (f16 planes from the kernel, joined on the host), cfg = gemm2's tile configuration (0 = automatic). */
int ttr_dbg_split_gemm(ttr_engine* e, const float* x, int M, int K, const float* w, const float* bias, int N, int np, int act, int out_planes,
                       const float* resid, int cfg, float* out);
int ttr_dbg_conv_pool(ttr_engine* e, const float* in0, int C0, int B, int H, int W, int ks, const float* wgt, const float* bias,
                      int Cout, int act, int pool_relu, float* out_full, float* out_pool);
/* The row kernels under every f16x4 recogniser layer on their own (f16x4 engines; they refuse while batches stream, add no kernel and change no pass).
 * ttr_dbg_split_planes: split_planes_kernel over host rows x f32 [M][ld] (C <= ld channels of each, C % 8 == 0, ld % 4 == 0; relu != 0 = ReLU first) ->
 * raw_out u16 [M][planes * C], the f16 bits of the planes x0 | x1 (| x2) as the kernel wrote them (planes 2 = pair, 3 = exact triple).  The launch watches
 * a zeroed range word of its own: *tripped (may be NULL) = 1 when a value it split was not below 65504, and the engine's own words never see it.
 * ttr_dbg_layernorm_planes: layernorm_planes_kernel over x f32 [M][ld] (384 channels, ld >= 384), gamma / beta f32 [384] -> raw_out u16 [M * planes * 384]
 * exactly as the kernel laid it out: rows [M][planes][384], or with tiled != 0 (M % 8 == 0) the GEMM loader's pieces [M / 8][plane][6 blocks of 64][8 rows][64].
 * ttr_dbg_ln_linear: the decoder's LayerNorm + linear pair, K = 384: x f32 [M][384], w f32 [N][384], bias f32 [N] (may be NULL) -> out f32 [M][N];
 * fused = 0: the LayerNorm kernel (triples) followed by the skinny whole-K linear, fused = 1: the skinny linear with the LayerNorm as its prologue. */
int ttr_dbg_split_planes(ttr_engine* e, const float* x, int M, int C, int ld, int planes, int relu, uint16_t* raw_out, int* tripped);
int ttr_dbg_layernorm_planes(ttr_engine* e, const float* x, int M, int ld, const float* gamma, const float* beta, float eps, int planes, int tiled,
                             uint16_t* raw_out);
int ttr_dbg_ln_linear(ttr_engine* e, const float* x, int M, const float* gamma, const float* beta, float eps, const float* w, const float* bias, int N,
                      int fused, float* out);
/* The tap on the split detector (f16x4 engines): one forward pass over B canvases u8 [B][H][W][3] with every launch noting where its tensors live (inputs,
 * out, out_relu, out_pool, the low-resolution z of a commuted up-convolution, the heat map; tensors a fusion never writes have no record).  Returns the number
 * of records (-1 on error); heat_out (may be NULL) f32 [B][H/2][W/2][2].  Nothing is copied during the pass and no kernel is added; a pass without the tap is
 * unchanged.  The records hold until the engine's next detector pass. */
int ttr_dbg_craft_taps(ttr_engine* e, const uint8_t* canvas, int B, int H, int W, float* heat_out);
int ttr_dbg_craft_tap_count(ttr_engine* e);
/* record i: text = "layer\nrole\nkernel kind" (role: canvas, in0, in1, out, out_relu, out_pool, z, heat), dims = {B, H, W, real channels, row length in channels,
 * form (0 fp32, 1 packed pairs [x0 | x1], 2 pairs, 3 triples, 4 u8), f16 planes per value} */
int ttr_dbg_craft_tap_info(ttr_engine* e, int i, char* text, size_t cap, int dims[7]);
/* tensor i joined to fp32 on the host (split.h: join2 / join3, every step exact), f32 [B][H][W][row length]: padding channels included */
int ttr_dbg_craft_tap_read(ttr_engine* e, int i, float* out);
/* With the tuning key fc7_fold on (the default) the pass proper runs upconv1.0 as slice5.1 + slice5.2 + upconv1.0 folded into one 3x3 plus the skip half's 1x1;
 * a tapped pass additionally runs the three layers themselves into side workspaces nothing reads, and the records above are THEIRS.  The folded launches'
 * records are a second list: layer "upconv1.0", roles in0 (the 3x3 max-pool's output), in1 (relu5_3), z (the skip half, fp32) and out.  Same calls as above. */
int ttr_dbg_craft_fold_tap_count(ttr_engine* e);
int ttr_dbg_craft_fold_tap_info(ttr_engine* e, int i, char* text, size_t cap, int dims[7]);
int ttr_dbg_craft_fold_tap_read(ttr_engine* e, int i, float* out);
/* Which kernel serves bf16 layers: -1 = first-generation igemm only, 0 = automatic (default),
 * 1..6 = force that gemm2 tile configuration where it applies.  Process-wide; for tuning and tests. */
void ttr_set_gemm_config(int cfg);
/* PARSeq autoregressive loop in bf16 mode: 0 = one kernel per op (the f32 mode's schedule), 4 / 8 / 16 = the
 * fused persistent kernel with that many crops per workgroup, anything else = automatic (default). */
void ttr_set_decoder_mode(int mode);
/* Process-wide knobs by name: the defaults of engines created afterwards for the per-engine keys of ttr_engine_set_tuning, and the
 * kernel-variant switches that live in the kernel files.  Kernel selection: "gemm_config", "decoder_mode" (as above), "enc_chunk" (crops per PARSeq
 * encoder group, 0 = all at once), "sk_max_rows" / "ws_min_rows" (row counts up to / from which linears use the skinny / the
 * weight-stationary GEMM), "mlp_fused" (0 off, 1 = from "mlp_min_rows" rows on (default), 2 = always), "ln_fuse" (decoder
 * LayerNorms inside the skinny GEMM), "tok_fuse" (AR steps: argmax + token embedding + norm_c inside the self_kv skinny GEMM), "self_refine" (refinement-pass
 * self-attention as one workgroup per crop), "cross_mfma" (refinement-pass cross-attention on the matrix cores), "dec_mlp_fused" / "dec_mlp_min_rows" (refinement pass: cross_out + norm2 + FFN + final norm through the
 * fused block kernel from that many rows on; 1 = when its 128-row panels fill the CUs' last round to 65 %, 2 = always), "fuse_first", "ws_lean", "store_policy" (0 default, 1 streaming, 2 system-scope streaming
 * output stores), "g2_x_ring3", "c3_*" (conv3p variants: "c3_c32" 32-wide tiles for Cout <= 32, "c3_narrow64" 64-wide tiles on the
 * 16x16-patch maps: 0 never / 1 always / 2 when the chip would be under-filled), "c3s_wgs" (persistent conv3s workgroups per CU),
 * "upsample_block" (2x4-block bilinear kernel), "craft_group" (pages per CRAFT launch group), "ar_early_exit" / "ar_crop_exit" /
 * "ar_tail_step" (AR loop: batch-level exit, per-crop exit in the step's attention kernels, step from which the fused tail kernel
 * takes over), "mlp_store_nt".  Timing experiments (results unspecified): "mlp_stagger",
 * "mlp_ablate" / "pair_ablate" (libraries built with -DMLP_ABLATE_BUILDS).  Diagnostics: "dec_stamps" (1 fused decoder, 2 gemm_ws, 3 mlp_fused
 * phase stamps, read back with ttr_dbg_dec_stamps), "dbg_bf16_out", "ws_dbg_flags".
 * Returns 0, or -1 for an unknown key.  Selection knobs change fp32 summation order at most (never a rounding point). */
int ttr_set_tuning(const char* key, int value);
/* host wall-clock splits (microseconds) of the engine's last batch: [0] enqueue resize+CRAFT+CCL, [1] wait for the component
 * counters, [2] wait for candidates / row extremes, [3] calipers, [4] crop rectangles + PARSeq enqueue, [5] wait for the GPU,
 * [6] event read-back, [7] token decode */
void ttr_last_host_us(ttr_engine* e, float out[8]);
/* test hook for the ViT encoder self-attention kernels: qkv f32 [N][128][1152] (rounded to the engine's type) -> out [N][128][384].  f16x4 engines run
 * attn_split.hip the way the encoder does behind a separate qkv GEMM: the fp32 rows become exact triples (split_planes), the kernel reads and writes planes,
 * and the output triples are joined here.  f32 engines run the fp32 kernel, bf16 engines theirs. */
int ttr_dbg_attn_enc(ttr_engine* e, const float* qkv, int N, float* out);
/* test hook for the decoder's cross-attention kernels of the split-operand / fp32 engines (parseq_ops.hip, attn_cross_split.hip; which one runs follows the
 * tuning keys "cross_split", "cross_crop", "cross_rows_hsplit"): q f32 [N * R][384] (R query rows per crop), kvmem f32 [N * 128][768] (K | V of a crop's 128
 * memory tokens) -> out f32 [N * R][384], joined from the exact triples the kernels write */
int ttr_dbg_cross_attn(ttr_engine* e, const float* q, const float* kvmem, int N, int R, float* out);
/* test hook for the decoder's self-attention kernel of the split-operand / fp32 engines (parseq_ops.hip: dec_self_attn_kernel), launched the way the engine's
 * precision launches it (f16x4: exact triples out, joined here; f32: fp32 rows) and without the AR loop's skip counter: q f32 [26][384] (the projected position
 * queries), kvcache f32 [N][26][768] (K | V per context slot), tokens i32 [N][26] (read in mode 1: id 0 = EOS) -> out f32 [N * R][384].  mode 0 = AR step qi0
 * (R = 1: keys 0 .. qi0), mode 1 = the refinement pass (R query rows 0 .. R - 1 per crop, R <= 26: cloze mask + key padding from the first EOS on).  K / V rows of
 * masked keys are not read.  A row the kernel did not write comes back as NaN. */
/* test hook for the lexicon scorers' tables (lexicon_fuzzy.hip: lex_tile_tables, the function both the fuzzy scorer and this dump build them with): host logits
 * [n][26][95] through decode_conf_kernel, then lp f32 [n][26][96] as a workgroup forms it in LDS - lp[p][c] = (x[p][c] - x[p][id[p]]) + logf(prob[p]) for an
 * allowed class, -inf for a blocked one and for column 95.  sets / n_sets / set_of as in ttr_logits_lexicon.  So that a test can hold the fuzzy kernel to
 * ttr_lexicon_fuzzy_from_lp bit for bit.  Refuses while batches stream. */
int ttr_debug_lexicon_tables(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, float* lp);
int ttr_dbg_dec_self_attn(ttr_engine* e, const float* q, const float* kvcache, const int32_t* tokens, int N, int R, int qi0, int mode, float* out);
/* test hook for qkv_attn.hip (bf16 engines): x f32 [N][128][384], w [1152][384], b [1152] -> self-attention output [N][128][384] */
int ttr_dbg_qkv_attn(ttr_engine* e, const float* x, int N, const float* w, const float* b, float* out);
/* test hook for mlp_fused.hip (bf16 engines): x_out = x + fc2(GELU(fc1(LayerNorm(x)))) over f32 rows [M][384] with weights
 * w1 [1536][384], w2 [384][1536] (rounded to bf16 inside); nln_out (may be NULL) = LayerNorm(x_out; nln_g, nln_b), bf16 values as f32.
 * With att != NULL the attention output projection runs first in the same launch: x is replaced by x + att . wp^T + bp
 * (att f32 [M][384] and wp [384][384] rounded to bf16). */
int ttr_dbg_mlp(ttr_engine* e, const float* x, int M, const float* ln_g, const float* ln_b, float eps, const float* w1, const float* b1, const float* w2,
                const float* b2, const float* nln_g, const float* nln_b, float* x_out, float* nln_out, const float* att, const float* wp, const float* bp);
/* diagnostics: after ttr_set_tuning("dec_stamps", 1 / 2 / 3) workgroup 0 of the fused AR kernel / gemm_ws / mlp_fused records
 * shader-clock stamps into a 416-entry buffer ([26 steps][16 phases], [2 waves][24 panels][8], [48 chunks][8]); this copies them out.
 * Returns -1 when stamps are off. */
int ttr_dbg_dec_stamps(unsigned long long* out);
/* the first n (<= 4096) words of the same buffer: qkv_attn4.hip also records where and when each workgroup ran (words 512 + 4 b ..: start, end in 100 MHz ticks, HW_ID | XCC_ID << 32, shader clocks) */
int ttr_dbg_dec_stamps_ext(unsigned long long* out, int n);
/* Times one conv / linear layer on device-generated random data (no host traffic): average
 * microseconds per launch over `iters` back-to-back launches.  f32_resid != 0 selects the PARSeq
 * residual form (f32 residual in, f32 out) instead of a bf16/T output. */
int ttr_bench_conv(ttr_engine* e, int B, int H, int W, int C0, int C1, int ks, int dil, int Cout, int act, int f32_resid,
                   int iters, float* avg_us);

/* ---- host-side geometry hooks (no GPU touched; used by the CPU test-suite) -------------------- */
/* cv::minAreaRect stand-in used at tuatara.cpp:179,:248: n points (x,y) float32 -> {cx,cy,w,h,angle}. */
int ttr_dbg_min_area_rect(const float* xy, int n, float* rect5);
/* the TCP rendezvous of ttr_comm_create_tcp on its own (no GPU, no RCCL): rank 0 listens on addr:port and hands its `bytes` bytes to the
 * world - 1 ranks that connect.  Returns 0, or -1 (ttr_last_error).  tests/test_comm_cpu.py runs it with two processes. */
int ttr_dbg_tcp_share(int rank, int world, const char* addr, int port, void* buf, size_t bytes);
/* tuatara.cpp:162-179 for one component given its stats and per-row x extremes
 * rows[(y1-y0+1)][2] = {min x, max x} ({INT_MAX,-1} = empty row).  Returns 1 if a rect was produced. */
int ttr_dbg_component_rect(int area, int x0, int y0, int x1, int y1, const int32_t* rows, int H, int W, float* rect5);
/* adjust_result_coordinates + boundingRect + format (tuatara.cpp:236-274, :416): rect5 in heat-map
 * pixels -> adjusted rect5, crop xywh (unclamped) and the tesseract bbox. */
int ttr_dbg_box_geometry(const float* rect5, float ratio, float* adjusted5, int32_t* xywh, float* bbox4);
/* the rectified-crop rule on one rect {cx,cy,w,h,angle} in image pixels (geometry.h: deskew_quad): quad8 {tl, tr, br, bl}, coef6
 * {X0, Ax, Bx, Y0, Ay, By} in double, fixed6 the same in int64 units of 2^-16 px.  Returns the crop kind (0 or 1). */
int ttr_dbg_deskew(const float* rect5, float* quad8, double* coef6, int64_t* fixed6);
/* word orientation (geometry.h: box_edge_quad / turn_coef) on one rect {cx,cy,w,h,angle} in image pixels of an h x w page: the word's quad Q
 * (crop_mode 1: the deskewed quad; 0: the clamped boundingRect's pixel edges) turned by `turn` quarter turns, quad8 = Q_t, fixed6 its
 * coefficients as the engine hands them to pack_crops_rect_kernel.  Returns 0, -1 on bad arguments. */
int ttr_dbg_orient_quad(const float* rect5, int h, int w, int crop_mode, int turn, float* quad8, int64_t* fixed6);
/* tables (DESIGN.md "Tables"): table_ink_kernel and table_grid_kernel on a host image u8 [h][w][3] (row_stride bytes, 0 = 3 w), placed dev_offset bytes into a
 * device buffer with dev_stride bytes from row to row (0 = 3 w) - an offset or stride that is no multiple of 4 takes the kernel's byte-load path.  bits
 * [h][ceil(w / 64)] uint64 the ink bitmap, runs [2][8192][3] int32 the horizontal {y, x0, x1} and vertical {x, y0, y1} run lists (zero beyond their counts),
 * n_runs [2] (0, 0 for a page beyond the run cap), mode; any output may be NULL.  Refuses while batches stream.  Returns 0, -1 on error. */
int ttr_dbg_tables(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_len, int ink, uint64_t* bits, int32_t* runs,
                   int32_t* n_runs, int32_t* mode);
/* deskew (DESIGN.md "Deskew"): ttr_deskew_page with the host image placed dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 w),
 * so that the kernels see a window whose base and stride are no multiples of 4.  Outputs as ttr_deskew_page.  Refuses while batches stream.  Returns 0, -1 on error. */
int ttr_dbg_deskew_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int max_slope, int gain, int ink, uint8_t* out_img,
                   ttr_skew* rec, uint64_t* scores);
/* local ink (DESIGN.md "Local ink"): ttr_ink_page with the host image placed dev_offset bytes into a device buffer with dev_stride bytes from row to row (0 = 3 w),
 * as ttr_dbg_tables takes it.  Outputs as ttr_ink_page.  Refuses while batches stream.  Returns 0, -1 on error. */
int ttr_dbg_ink_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int radius, int drop, int polarity, uint64_t* bits,
                     uint64_t* bitsT, ttr_ink* rec);
/* selection marks (DESIGN.md "Selection marks"): table_ink_kernel, mark_cand_kernel and mark_page_kernel on a host image placed as ttr_dbg_tables takes it.
 * corners: the corners examined; band_counts [ceil(h / 32)][2]: per band of 32 rows the candidates kept and the corners examined, as the candidate pass wrote
 * them; mode; marks [512][12] (zero beyond the count); any output may be NULL.  Refuses while batches stream.  Returns 0, -1 on error. */
int ttr_dbg_marks(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_side, int max_side, int fill, int ink,
                  int32_t* corners, int32_t* band_counts, int32_t* mode, int32_t* marks);
/* barcodes (DESIGN.md "Barcodes"): table_ink_kernel, barcode_scan_kernel and barcode_page_kernel on a host image placed as ttr_dbg_tables takes it.  hits
 * [(h + w) 2 8][20]: the raw hits of every line (rows, then columns) and reading (forwards, backwards), eight slots each, as barcodes_rule.h lays a hit out (p0,
 * p1, module64, flags, len, symbology, the hit it chains to, its chain's first hit, text [12]; zero beyond a line's count); line_counts [(h + w) 2][4]: hits
 * kept, hits dropped, candidates, start patterns; side [1544]: the page's side block (zero beyond the count); any output may be NULL.  Refuses while batches
 * stream.  Returns 0, -1 on error. */
int ttr_dbg_barcodes(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int dev_offset, int dev_stride, int min_lines, int ink, int symbologies, int32_t* hits,
                     int32_t* line_counts, int32_t* side);
/* the ink passes (table_ink_kernel, or local ink's two kernels) the engine has enqueued for its batches' page layers since it was created: tables and selection
 * marks in one batch under one ink rule share one.  -1 for a null engine. */
int64_t ttr_dbg_page_ink_passes(const ttr_engine* e);
/* canvas_geometry on the host for any canvas_size / mag_ratio (what ttr_canvas_geometry answers for an engine of that config): h32 x w32, the ratio and
 * the resized page's target_h x target_w inside the canvas.  Any output may be NULL.  Returns 0, -1 for h <= 0 or w <= 0. */
int ttr_dbg_canvas_geometry(int h, int w, int canvas_size, float mag_ratio, int* H, int* W, float* ratio, int* target_h, int* target_w);
/* launch groups of the f16x4 engine on the host (DESIGN.md "Launch groups"): pages per CRAFT group for a batch of n_pages canvases of H x W (multiples of 32) and
 * crops per encoder group for n_crops crops, under the tuning values given - craft_group, first_fused (the effective switch), craft_products, up_commute; enc_chunk
 * (0 = the engine's default cap of 1820 crops; larger values lift it up to the window), enc_fc2_pairs, qkv_attn_split, enc_ln_pairs, sp_hidden16 - with the bytes
 * per page / per crop of the widest tensor the kernels address with 32-bit offsets.
 * group x bytes never exceeds 2^31 - 1, except where ONE page is already wider than that (2560 x 2560 as triples): the group is then 1 and the forward pass
 * refuses the page.  Any output may be NULL.  Returns 0, -1 on bad arguments. */
int ttr_dbg_launch_groups(int H, int W, int n_pages, int n_crops, int craft_group, int first_fused, int craft_products, int up_commute, int enc_chunk,
                          int enc_fc2_pairs, int qkv_attn_split, int enc_ln_pairs, int sp_hidden16, int* craft_pages, int* enc_crops, int64_t* page_bytes,
                          int64_t* crop_bytes);
/* the shape checks of the f16x4 layer launchers on the host (no GPU, nothing is launched): kernel 0 = the patch-stationary 3x3 kernel, 1 = the split GEMM loop, 2 = the 3x3 kernel with conv1_1 fused in front (pooled output only), on a
 * layer of B x H x W pixels, C0 -> Cout channels, ks x ks taps, products 3 (pairs) / 4 (triples), out_planes 0 / 2 / 3, pooled != 0 = with the fused 2x2 max-pool
 * output.  Returns 0 when the launcher takes the layer, 1 when it refuses (text, may be NULL, receives its reason), -1 on bad arguments. */
int ttr_dbg_split_layer_check(int kernel, int B, int H, int W, int C0, int Cout, int ks, int products, int out_planes, int pooled, char* text, size_t cap);
/* what the engine's last batch of pages and last recogniser pass ran with: pages per CRAFT launch group, crops per encoder group (0 = none yet) */
int ttr_dbg_last_groups(ttr_engine* e, int* craft_pages, int* enc_crops);
/* the heat maps of the engine's last batch of n pages, f32 [n][H/2][W/2][2], as its detector left them on the device.  Refuses while batches stream. */
int ttr_dbg_last_heat(ttr_engine* e, float* heat, size_t floats);
/* History invariance (tests/test_gpu_history.py): the engine's device buffers as the table of tuatara_amd/csrc/engine.h classifies them.
 * ttr_dbg_scratch_table: host only, no engine - one buffer per line, "name class kind" and, behind them, the row's note (for a kept row: the contract that makes it
 * so); class scratch / kept, kind f32 / f16 / u8 / i32 / addr.  Returns the text's length (what fits `cap` is copied, terminated).
 * ttr_dbg_poison_scratch (f16x4 engines; refuses while batches stream): synchronises the engine's streams, then fills every allocated scratch buffer to its full
 * capacity - pattern 0 zeros, 1 quiet NaN (f32 0x7FC00000, f16 0x7E00, u8 0xA5), 2 large finite (f32 1e4, f16 8192, u8 0x5A); i32 buffers always with zeros, addr
 * buffers not at all - with plain memsets and one synchronise: no kernel is added and no pass changes.  also_kept_once != 0 poisons the two write-once float
 * buffers as well (the detector's zero-padded head slots, the decoder's K/V cache): such an engine computes garbage from then on and is only good for showing that
 * the poison reaches memory the kernels read.  Returns the bytes filled, -1 on error. */
int ttr_dbg_scratch_table(char* text, size_t cap);
int64_t ttr_dbg_poison_scratch(ttr_engine* e, int pattern, int also_kept_once);


#ifdef __cplusplus
}
#endif
#endif
