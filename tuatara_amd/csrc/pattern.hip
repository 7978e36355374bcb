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

// ------------------------------------------------------------------ the final decode under a pattern, best mode (DESIGN.md "Patterns": the likeliest member)
// One workgroup (256 threads) per crop; thread s owns local state s of the crop's automaton (states first .. first + count - 1 of the table, count <= 256) and
// keeps that state's delta row in registers (48 dwords).  LDS: lp, the lexicon's table of this crop - 26 rows of 96 floats, built from the standard block
// launch_decode_conf left in id0 / prob0; two arrays of 256 keys (the level being read and the level being formed); the back-pointers [26][256] u16; the path.
//   key = order-preserving image of the fp32 score << 32 | (127 - class) << 8 | (255 - source state)
// A thread pushes V[p][s] + lp[p][c] to the key of its target with a 64-bit LDS maximum: the largest key is the largest score, then the lower class, then
// the lower source state, whatever the order of arrival.  0 is "not reached" (the image of any score that may be chosen is not 0: -inf and NaN are never
// pushed).  Every score has + 0.0f added before its image is formed (a -0.0f would rank below +0.0f; the host rule does the same), so equal scores have equal images.  The word's end is the
// same maximum over (image of V[L][s] + lp[L][0], 25 - L, 255 - s).  No global atomics; nothing depends on how the work is divided.
// Wave 0 then walks the positions as decode_pat_kernel does, with the class forced along the chosen path up to the EOS and free behind it; a crop without a
// pattern (count == 0) or without a member of finite score is walked free from the start: decode_pat_kernel's bits.
namespace {
constexpr int kBestStates = 256, kRowWords = kCols / 2;
__device__ __forceinline__ unsigned f32_image(float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float f32_of_image(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
}  // namespace

__global__ void __launch_bounds__(256) pattern_best_kernel(const float* __restrict__ logits, int N, const int* __restrict__ id0, const float* __restrict__ prob0,
                                                           int* __restrict__ ids, float* __restrict__ prob, float* __restrict__ conf, float* __restrict__ logp,
                                                           PatDev pt, PatExtent ex, ClassMask cm, const RowMask* __restrict__ row_masks) {
  __shared__ float lp[kPos * kCols];                       // 9984 bytes
  __shared__ unsigned long long keys[2][kBestStates];      // 4096
  __shared__ uint16_t back[kPos][kBestStates];             // 13312
  __shared__ unsigned long long fin;
  __shared__ float row_x[kPos], row_l[kPos];
  __shared__ int path[kPos];
  __shared__ int path_len;
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;   // (the grid has N blocks)
  const float* x = logits + (int64_t)n * kPos * kCls;
  const int first = ex.extent_of ? ex.extent_of[2 * n] : ex.first;
  const int count = min(ex.extent_of ? ex.extent_of[2 * n + 1] : ex.count, kBestStates);
  const int start = pt.start_of ? pt.start_of[n] : pt.start;
  // ---- lp: the rows' constants first, then the table (lexicon_score_kernel's expression on the same inputs)
  if (tid < kPos) {
    const int r = n * kPos + tid;
    const int id = min(max(id0[r], 0), kCls - 1);
    row_x[tid] = x[tid * kCls + id];
    row_l[tid] = logf(prob0[r]);
  }
  keys[0][tid] = 0ull;
  if (tid == 0) fin = 0ull;
  __syncthreads();
  {
    const RowClassMask rm = row_class_mask(cm, row_masks, n);
    for (int e = tid; e < kPos * kCols; e += 256) {
      const int p = e / kCols, c = e - p * kCols;
      float v = -INFINITY;
      if (c < kCls && rm.allows(c)) v = (x[p * kCls + c] - row_x[p]) + row_l[p];
      lp[e] = v;
    }
  }
  // ---- this thread's state: its delta row, 96 u16 as 48 dwords (a row is 192 bytes, 16-byte aligned)
  unsigned row[kRowWords];
  const bool owns = tid < count;
#pragma unroll
  for (int i = 0; i < kRowWords; ++i) row[i] = 0xFFFFFFFFu;
  if (owns) {
    const uint4* src = reinterpret_cast<const uint4*>(pt.delta + (int64_t)(first + tid) * kCols);
#pragma unroll
    for (int i = 0; i < kRowWords / 4; ++i) { const uint4 q = src[i]; row[4 * i] = q.x; row[4 * i + 1] = q.y; row[4 * i + 2] = q.z; row[4 * i + 3] = q.w; }
  }
  const bool accepts = (row[0] & 0xFFFFu) != kNone;
  if (owns && tid == start - first) keys[0][tid] = (unsigned long long)f32_image(0.0f) << 32;   // V[0][start] = 0 (no other thread writes keys[0] before the barrier)
  __syncthreads();
  // ---- the levels: keys[cur] holds V[l]
  for (int l = 0; l < kPos; ++l) {
    const int cur = l & 1;
    // (the row's words pass through an empty asm at every level: what is derived from them - 94 successors, their key addresses and the keys' low words - is then formed
    // where it is used; hoisted out of this loop it would hold some 300 registers for the whole kernel)
#pragma unroll
    for (int i = 0; i < kRowWords; ++i) asm volatile("" : "+v"(row[i]));
    unsigned inv_s = 255u - (unsigned)tid;
    asm volatile("" : "+v"(inv_s));
    const unsigned long long k = keys[cur][tid];
    keys[cur ^ 1][tid] = 0ull;                                        // (level l - 1: every thread read its key before the last barrier)
    __syncthreads();
    if (k != 0ull) {                                                  // (a key is only ever pushed to a state of this automaton, so tid < count)
      back[l][tid] = (uint16_t)k;
      const float vs = f32_of_image((unsigned)(k >> 32));
      const float* lrow = lp + l * kCols;
      if (accepts) {
        const float f = (vs + lrow[0]) + 0.0f;                     // (+ 0.0f: a -0.0f sum becomes +0.0f, so equal scores have equal images by construction)
        if (f > -INFINITY) atomicMax(&fin, (unsigned long long)f32_image(f) << 32 | ((unsigned)(kMaxChars - l) << 8 | inv_s));
      }
      if (l < kMaxChars) {
#pragma unroll
        for (int c = 1; c < kCls; ++c) {
          const unsigned t = (row[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;
          if (t != kNone) {
            const float v = (vs + lrow[c]) + 0.0f;
            const unsigned tl = t - (unsigned)first;
            if (v > -INFINITY && tl < (unsigned)kBestStates)          // (false for -inf and NaN; a successor lies inside the automaton)
              atomicMax(&keys[cur ^ 1][tl], (unsigned long long)f32_image(v) << 32 | ((unsigned)(127 - c) << 8 | inv_s));
          }
        }
      }
    }
    __syncthreads();
  }
  // ---- the path, backwards from the end
  if (tid == 0) {
    int L = -1;
    if (fin != 0ull) {
      L = kMaxChars - (int)((fin >> 8) & 0xFFu);
      int s = 255 - (int)(fin & 0xFFu);
      path[L] = 0;
      for (int l = L; l > 0; --l) {
        const unsigned b = back[l][s];
        path[l - 1] = 127 - (int)(b >> 8);
        s = 255 - (int)(b & 0xFFu);
      }
    }
    path_len = L;
  }
  __syncthreads();
  if (tid >= 64) return;
  // ---- the standard block: decode_pat_kernel's walk, the class forced for p <= L
  const int L = path_len;
  const bool hi = lane + 64 < kCls;
  float v0[kPos], v1[kPos];
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    v0[p] = x[p * kCls + lane];
    v1[p] = hi ? x[p * kCls + 64 + lane] : 0.f;
  }
  int s = __builtin_amdgcn_readfirstlane(start);
  float cf = 1.f, sc = 0.0f;
  bool ended = false;
  int my_id = 0;
  float my_prob = 0.f;
#pragma unroll
  for (int p = 0; p < kPos; ++p) {
    const LaneChoice ch = lane_choice(pt.delta, pt.mind, s, p, lane);
    float best = -INFINITY; int bi = 0x7fffffff;
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
    float pr = 1.f / sum;
    if (p <= L) {                                                   // (wave-uniform) the chosen path's class: allowed here, as the path ends in an EOS within 25 characters
      const int f = path[p];
      if (f != bi) { bi = f; pr = expf(__shfl(f < 64 ? v0[p] : v1[p], f & 63) - best) / sum; }
    }
    const bool chosen = (unsigned)bi < (unsigned)kCls;
    if (!chosen) bi = 0;
    const unsigned t = __shfl(bi < 64 ? ch.t0 : ch.t1, bi & 63);
    if (chosen && t != kNone) s = __builtin_amdgcn_readfirstlane((int)t);
    if (lane == p) { my_id = bi; my_prob = pr; }
    if (!ended) {
      sc += lp[p * kCols + bi];                                      // rule 2's score of the reading that is written
      if (bi == 0) { cf *= pr; ended = true; }
      else if (bi != 88 && bi >= 0 && bi < 98) cf *= pr;
    }
  }
  if (lane < kPos) {
    ids[(int64_t)n * kPos + lane] = my_id;
    prob[(int64_t)n * kPos + lane] = my_prob;
  }
  if (lane == 0) {
    conf[n] = cf;
    logp[n] = count > 0 && ended ? sc : -INFINITY;                   // (a row without a pattern has no score)
  }
}

void launch_pattern_best(const float* logits, int N, const int* id0, const float* prob0, int* ids, float* prob, float* conf, float* logp, hipStream_t s, PatDev pt,
                         PatExtent ex, ClassMask cm, const RowMask* row_masks) {
  if (N <= 0) return;
  hipLaunchKernelGGL(pattern_best_kernel, dim3(N), dim3(256), 0, s, logits, N, id0, prob0, ids, prob, conf, logp, pt, ex, cm, row_masks);
}

}  // namespace ttr
