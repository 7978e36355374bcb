// Per-character alternatives behind the recogniser's final decode (DESIGN.md "Character alternatives"): for every (crop, position) row of the refined
// logits the K best allowed classes and their softmax probabilities, where decode_conf_kernel keeps the winner alone.
//
//   alt_ids  [N][26][K]   the allowed classes in descending order of x[c] (fp32 comparison), ties to the lower class: argmax_kernel's comparison and
//                         wave reduction, repeated with the earlier winners removed - so slot 0 is the id of the standard block.  -1 where fewer than K
//                         classes can be chosen (blocked classes never appear; neither does a class whose logit is -inf or NaN, which no comparison picks)
//   alt_prob [N][26][K]   expf(x[alt_id] - x[id]) * prob in fp32 (full-precision expf), id and prob read from the standard block: slot 0 is
//                         expf(0.f) * prob = prob bit for bit, and no maximum or sum is formed a second time.  0.f in the empty slots
//   cm, row_masks         the class mask in force, as launch_decode_conf takes it (common.h: row_class_mask); the mask of row r is that of crop r / 26
//
// One wave per row, four rows per 256-thread block: a row's 95 logits are 380 contiguous bytes, lane and lane + 64 as in decode_conf_kernel (whose
// one-wave-per-crop form is latency-bound; K rounds per position would make it K times worse).  Each round is one wave arg-max over the classes not yet
// taken; lane j keeps slot j and stores it.  No scratch memory, no LDS; the launch only reads the logits and the standard block.
#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {
constexpr int kPos = 26, kCls = 95, kRows = 4;   // positions per crop, classes, rows (waves) per 256-thread block
}

__global__ void __launch_bounds__(256) decode_alts_kernel(const float* __restrict__ logits, int rows, const int* __restrict__ ids, const float* __restrict__ prob,
                                                          int K, int* __restrict__ alt_ids, float* __restrict__ alt_prob, ClassMask cm,
                                                          const RowMask* __restrict__ row_masks) {
  const int r = blockIdx.x * kRows + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const RowClassMask rm = row_class_mask(cm, row_masks, r / kPos);   // (wave-uniform: a block's four waves may hold rows of different crops, so different sets)
  const float* x = logits + (int64_t)r * kCls;
  const bool hi = lane + 64 < kCls;
  const float v0 = x[lane], v1 = hi ? x[64 + lane] : 0.f;
  bool a0 = rm.allows(lane), a1 = hi && rm.allows(lane + 64);       // still to be chosen: allowed and not taken by an earlier round
  const int id0 = ids[r];
  const float pr = prob[r];
  // x[id]: from the lane that holds it (an id outside the 95 classes cannot come out of decode_conf_kernel; the shuffle keeps even that inside the wave)
  const float lo_v = __shfl(v0, id0 & 63), hi_v = __shfl(v1, id0 & 63);
  const float xid = id0 >= 64 ? hi_v : lo_v;
  int my_id = -1;
  float my_pr = 0.f;
  for (int j = 0; j < K; ++j) {
    float best = -INFINITY; int bi = 0x7fffffff;                    // argmax_kernel's per-lane loop: c = lane, then c = lane + 64
    if (a0 && v0 > best) { best = v0; bi = lane; }
    if (a1 && v1 > best) { best = v1; bi = lane + 64; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (bi == 0x7fffffff) break;                                    // wave-uniform: nothing left to choose, the remaining slots stay -1 / 0.f
    if (bi == lane) a0 = false;
    if (bi == lane + 64) a1 = false;
    if (lane == j) { my_id = bi; my_pr = expf(best - xid) * pr; }
  }
  if (lane < K) {
    alt_ids[(int64_t)r * K + lane] = my_id;
    alt_prob[(int64_t)r * K + lane] = my_pr;
  }
}

void launch_decode_alts(const float* logits, int N, const int* ids, const float* prob, int K, int* alt_ids, float* alt_prob, hipStream_t s, ClassMask cm,
                        const RowMask* row_masks) {
  if (N <= 0) return;
  if (K < 2 || K > 8) throw std::runtime_error("decode_alts: K must lie in 2..8");
  if (N > (1 << 24)) throw std::runtime_error("decode_alts: more than 2^24 crops in one launch");   // (rows = 26 N is an int)
  const int rows = N * kPos;
  hipLaunchKernelGGL(decode_alts_kernel, dim3((rows + kRows - 1) / kRows), dim3(256), 0, s, logits, rows, ids, prob, K, alt_ids, alt_prob, cm, row_masks);
}

}  // namespace ttr
