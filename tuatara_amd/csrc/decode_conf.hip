// The recogniser's final decode with its confidence (DESIGN.md "Recognition confidence"): the argmax of the refined logits
// (tuatara.cpp:486, Tokenizer::max_dist :101-106) and the softmax probability the reference computes and throws away.
//
//   ids  [N][26]   first maximal index of each row - the comparison and the wave reduction of argmax_kernel (parseq_ops.hip), so the ids
//                  are bit-identical to it
//   prob [N][26]   1 / sum_c expf(x[c] - x[id]) in fp32 (full-precision expf)
//   cm             the class mask (DESIGN.md "Character sets"): the maximum and the sum run over the allowed classes only; none blocked = the bits of before
//   row_masks      optional [N] table of per-crop masks (common.h: RowMask) that replaces cm crop by crop; null = cm for every crop
//   conf [N]       fp32 product, in position order from 1.0f, of prob over the characters of the text (positions before the first EOS,
//                  id 0, whose id is not 88 and lies in [0, 98): Tokenizer::filter + decode), times prob[EOS] when there is one
//
// One wave per crop: its 26 x 95 logits (9.9 KB, contiguous) are loaded up front, 2 values per lane and row, and each row is reduced
// across the wave (max + index, then the exp-sum; xor butterflies, so every lane holds the same bits).  Every lane forms the product
// in the same sequential order; lane p stores row p's id and prob, lane 0 the conf.  ttr_confidence_from_probs (capi.cpp) is the host
// restatement of the product.
#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {
constexpr int kPos = 26, kCls = 95, kCrops = 4;   // positions, classes, crops (waves) per 256-thread block
}

__global__ void __launch_bounds__(256) decode_conf_kernel(const float* __restrict__ logits, int N, int* __restrict__ ids, float* __restrict__ prob,
                                                          float* __restrict__ conf, ClassMask cm, const RowMask* __restrict__ row_masks) {
  const int n = blockIdx.x * kCrops + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const RowClassMask rm = row_class_mask(cm, row_masks, n);   // (crop n's own set, when a row table travels with the launch: a block's four waves may hold four sets)
  const float* x = logits + (int64_t)n * kPos * kCls;
  const bool hi = lane + 64 < kCls;
  const bool a0 = rm.allows(lane), a1 = hi && rm.allows(lane + 64);   // a blocked class: -inf in the comparison, exactly 0 in the sum (same lanes, same butterflies)
  float v0[kPos], v1[kPos];
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    v0[p] = x[p * kCls + lane];
    v1[p] = hi ? x[p * kCls + 64 + lane] : 0.f;
  }
  float cf = 1.f;
  bool ended = false;
  int my_id = 0;
  float my_prob = 0.f;
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    float best = -INFINITY; int bi = 0x7fffffff;                 // argmax_kernel's per-lane loop: c = lane, then c = lane + 64
    if (a0 && v0[p] > best) { best = v0[p]; bi = lane; }
    if (a1 && v1[p] > best) { best = v1[p]; bi = lane + 64; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    float s = (a0 ? expf(v0[p] - best) : 0.f) + (a1 ? expf(v1[p] - best) : 0.f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float pr = 1.f / s;
    if (lane == p) { my_id = bi; my_prob = pr; }
    if (!ended) {                                                  // wave-uniform: the same sequential product on every lane
      if (bi == 0) { cf *= pr; ended = true; }
      else if (bi != 88 && bi >= 0 && bi < 98) cf *= pr;
    }
  }
  if (lane < kPos) {
    ids[(int64_t)n * kPos + lane] = my_id;
    prob[(int64_t)n * kPos + lane] = my_prob;
  }
  if (lane == 0) conf[n] = cf;
}

void launch_decode_conf(const float* logits, int N, int* ids, float* prob, float* conf, hipStream_t s, ClassMask cm, const RowMask* row_masks) {
  if (N <= 0) return;
  hipLaunchKernelGGL(decode_conf_kernel, dim3((N + kCrops - 1) / kCrops), dim3(256), 0, s, logits, N, ids, prob, conf, cm, row_masks);
}

}  // namespace ttr
