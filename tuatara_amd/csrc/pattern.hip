// Patterns (DESIGN.md "Patterns"): the two places that choose a token when a pattern is in force.  They stand in for argmax_kernel (parseq_ops.hip) and
// decode_conf_kernel (decode_conf.hip), which stay as they are: without a pattern neither kernel here is launched.
//
// The table (pattern.h): delta u16 [S][96] - column 0 the EOS, 1..94 the characters, 0xFFFF = no transition - and mind u8 [S], the least number of characters
// from a state to acceptance, 255 for a DONE state.  The choice rule, at character position p (0..25) in state s: class c with t = delta[s][c] may be chosen iff
//   t != 0xFFFF  and  (c == 0  or  mind[t] == 255  or  p + 1 + mind[t] <= 25)
// The token is the first maximal index among those classes - argmax_kernel's comparison and butterfly; a class that may not be chosen is -inf in the comparison
// and adds exactly 0.0f to the exponential sum.  Then s = t.
//
// Where the rows live: in global memory, read through L2.  A state's row is 192 bytes - lane l reads columns l and l + 64, so one row is two coalesced
// wave loads - and the states are wave-uniform, so a wave touches one row and at most 95 bytes of mind per position.  A call's table may hold 1024 states
// (192 KiB of delta: more than the 160 KiB of LDS), and a block's four crops may walk four different automata, so staging "the table" per block would move
// more bytes than the 26 rows a wave ever reads; the serial chain is 2 dependent loads per position either way (the row, then the gathered mind).
#include "common.h"
#include "kernels.h"

namespace ttr {

namespace {
constexpr int kPos = 26, kCls = 95, kCrops = 4, kCols = 96;   // positions, classes, crops (waves) per 256-thread block, columns of a table row
constexpr unsigned kNone = 0xFFFFu, kFree = 255u;
constexpr int kMaxChars = 25;

// the successors of state s on this lane's two classes (lane and lane + 64; columns 95 is padding and holds 0xFFFF), and whether each may be chosen at position p
struct LaneChoice { unsigned t0, t1; bool a0, a1; };
__device__ __forceinline__ LaneChoice lane_choice(const uint16_t* __restrict__ delta, const uint8_t* __restrict__ mind, int s, int p, int lane) {
  const uint16_t* row = delta + (int64_t)s * kCols;
  LaneChoice c;
  c.t0 = row[lane];
  c.t1 = lane < kCols - 64 ? (unsigned)row[lane + 64] : kNone;
  const unsigned m0 = c.t0 != kNone ? (unsigned)mind[c.t0] : 0u;   // (no load behind a missing transition)
  const unsigned m1 = c.t1 != kNone ? (unsigned)mind[c.t1] : 0u;
  c.a0 = c.t0 != kNone && (lane == 0 || m0 == kFree || p + 1 + (int)m0 <= kMaxChars);
  c.a1 = c.t1 != kNone && (m1 == kFree || p + 1 + (int)m1 <= kMaxChars) && lane + 64 < kCls;
  return c;
}
}  // namespace

// ------------------------------------------------------------------ the AR step's choice under a pattern (argmax_kernel's contract)
__global__ void __launch_bounds__(256) argmax_pat_kernel(const float* __restrict__ logits, int ld, int C, int* __restrict__ tokens, int tok_ld, int col, int N,
                                                         const int* skip, int skip_n, int* done_count, int eos, PatDev pt, int* __restrict__ state) {
  if (skip && __builtin_nontemporal_load(skip) >= skip_n) return;   // AR early exit (see ConvParams::skip)
  const int n = blockIdx.x * kCrops + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const int s = __builtin_amdgcn_readfirstlane(col == 1 ? (pt.start_of ? pt.start_of[n] : pt.start) : state[n]);
  const LaneChoice ch = lane_choice(pt.delta, pt.mind, s, col - 1, lane);   // column col holds character position col - 1
  const float* x = logits + (int64_t)n * ld;
  float best = -INFINITY; int bi = 0x7fffffff;
  if (lane < C) { const float v = x[lane]; if (ch.a0 && v > best) { best = v; bi = lane; } }
  if (lane + 64 < C) { const float v = x[lane + 64]; if (ch.a1 && v > best) { best = v; bi = lane + 64; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  const bool chosen = (unsigned)bi < (unsigned)kCls;   // (the budget invariant leaves a class at every reachable (state, position); NaN logits choose none: EOS, state kept)
  if (!chosen) bi = 0;
  const unsigned t = __shfl(bi < 64 ? ch.t0 : ch.t1, bi & 63);
  if (lane == 0) {
    tokens[n * tok_ld + col] = bi;
    state[n] = chosen && t != kNone ? (int)t : s;
    if (done_count && bi == eos) {   // upstream PARSeq's break (system.py): count the crops whose FIRST EOS is this token
      bool first = true;
      for (int c = 1; c < col; ++c) first = first && tokens[n * tok_ld + c] != eos;
      if (first) atomicAdd(done_count, 1);
    }
  }
}

void launch_argmax_pat(const float* logits, int ld, int C, int* tokens, int tok_ld, int col, int N, hipStream_t s, const int* skip, int skip_n, int* done_count,
                       int eos, PatDev pt, int* state) {
  if (N <= 0) return;
  hipLaunchKernelGGL(argmax_pat_kernel, dim3((N + kCrops - 1) / kCrops), dim3(256), 0, s, logits, ld, C, tokens, tok_ld, col, N, skip, skip_n, done_count, eos, pt, state);
}

// ------------------------------------------------------------------ the final decode under a pattern (decode_conf_kernel's layouts and product)
__global__ void __launch_bounds__(256) decode_pat_kernel(const float* __restrict__ logits, int N, int* __restrict__ ids, float* __restrict__ prob,
                                                         float* __restrict__ conf, PatDev pt) {
  const int n = blockIdx.x * kCrops + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const float* x = logits + (int64_t)n * kPos * kCls;
  const bool hi = lane + 64 < kCls;
  float v0[kPos], v1[kPos];
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    v0[p] = x[p * kCls + lane];
    v1[p] = hi ? x[p * kCls + 64 + lane] : 0.f;
  }
  int s = __builtin_amdgcn_readfirstlane(pt.start_of ? pt.start_of[n] : pt.start);
  float cf = 1.f;
  bool ended = false;
  int my_id = 0;
  float my_prob = 0.f;
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    const LaneChoice ch = lane_choice(pt.delta, pt.mind, s, p, lane);
    float best = -INFINITY; int bi = 0x7fffffff;                 // argmax_kernel's per-lane loop: c = lane, then c = lane + 64
    if (ch.a0 && v0[p] > best) { best = v0[p]; bi = lane; }
    if (ch.a1 && v1[p] > best) { best = v1[p]; bi = lane + 64; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    float sum = (ch.a0 ? expf(v0[p] - best) : 0.f) + (ch.a1 ? expf(v1[p] - best) : 0.f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float pr = 1.f / sum;
    const bool chosen = (unsigned)bi < (unsigned)kCls;           // (see argmax_pat_kernel)
    if (!chosen) bi = 0;
    const unsigned t = __shfl(bi < 64 ? ch.t0 : ch.t1, bi & 63);
    if (chosen && t != kNone) s = __builtin_amdgcn_readfirstlane((int)t);   // the wave-uniform winner moves the state
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

void launch_decode_pat(const float* logits, int N, int* ids, float* prob, float* conf, hipStream_t s, PatDev pt) {
  if (N <= 0) return;
  hipLaunchKernelGGL(decode_pat_kernel, dim3((N + kCrops - 1) / kCrops), dim3(256), 0, s, logits, N, ids, prob, conf, pt);
}

}  // namespace ttr
