// Word orientation (DESIGN.md "Word orientation"): the choice between the candidate readings of every word of a batch, and the page vote.
//
//   in   the standard recogniser block of the batch (turn 0: ids [rows][26] | prob [rows][26] | conf [rows], Engine::rec_out) and the
//        candidate block of the twins ((K - 1) N rows, candidate-major: row (j - 1) N + c = word c read at candidate j)
//   out  the standard block's rows of every word whose chosen candidate is not turn 0 are overwritten, in place, with that candidate's 26 ids,
//        26 prob and conf (so the batch's single device-to-host copy and all-gather carry the chosen readings); the side block
//        [N] int32 turn | [N][K] f32 candidate conf | [pages] int32 page turn
//
// One workgroup per page.  Phase 1, a thread per word: the largest conf, strict > in ascending turn order (ties to the lower turn), and a vote
// in LDS when the winning text has >= 2 characters (|S| of the confidence rule: positions before the first EOS, id 0, whose id is not 88 and
// lies in [0, 98)).  Phase 2 (after the barrier, so no row of the page is overwritten before every winner of the page is known): the page turn,
// then every word's chosen reading.  geometry.cpp: orient_select is the host restatement.
#include "common.h"
#include "kernels.h"

namespace ttr {

__global__ __launch_bounds__(256) void orient_select_kernel(int* __restrict__ ids, float* __restrict__ prob, float* __restrict__ conf,
                                                            const int* __restrict__ cids, const float* __restrict__ cprob, const float* __restrict__ cconf,
                                                            const int* __restrict__ first, int N, int K, int per_page, int* __restrict__ side) {
  __shared__ int votes[4];
  __shared__ int page_col;
  const int pg = blockIdx.x;
  const int c0 = first[pg], c1 = first[pg + 1];
  int* turn = side;
  float* cand = reinterpret_cast<float*>(side + N);
  int* page_turn = side + N + (size_t)N * K;
  const int step = K == 2 ? 2 : 1;                                 // candidate column -> turn: {0, 2} or {0, 1, 2, 3}
  if (threadIdx.x < 4) votes[threadIdx.x] = 0;
  __syncthreads();
  for (int c = c0 + (int)threadIdx.x; c < c1; c += blockDim.x) {
    float best = conf[c];
    int bj = 0;
    cand[(size_t)c * K] = best;
    for (int j = 1; j < K; ++j) {
      const float v = cconf[(size_t)(j - 1) * N + c];
      cand[(size_t)c * K + j] = v;
      if (v > best) { best = v; bj = j; }
    }
    const int* w = bj == 0 ? ids + (size_t)c * 26 : cids + ((size_t)(bj - 1) * N + c) * 26;
    int chars = 0;
    for (int p = 0; p < 26; ++p) {
      const int id = w[p];
      if (id == 0) break;
      if (id != 88 && id >= 0 && id < 98) ++chars;
    }
    if (chars >= 2) atomicAdd(&votes[bj], 1);
    turn[c] = bj;                                                  // (the column; phase 2 of this same thread makes it the chosen turn)
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int pt = 0;
    for (int j = 1; j < K; ++j) if (votes[j] > votes[pt]) pt = j;
    page_col = pt;
    page_turn[pg] = step * pt;
  }
  __syncthreads();
  for (int c = c0 + (int)threadIdx.x; c < c1; c += blockDim.x) {
    const int j = per_page ? page_col : turn[c];
    turn[c] = step * j;
    if (j == 0) continue;
    const size_t r = (size_t)(j - 1) * N + c;
    for (int p = 0; p < 26; ++p) {
      ids[(size_t)c * 26 + p] = cids[r * 26 + p];
      prob[(size_t)c * 26 + p] = cprob[r * 26 + p];
    }
    conf[c] = cconf[r];
  }
}

void launch_orient_select(int* ids, float* prob, float* conf, const int* cids, const float* cprob, const float* cconf, const int* first, int pages, int N,
                          int K, int per_page, int* side, hipStream_t s) {
  if (pages <= 0 || N <= 0) return;
  if (K != 2 && K != 4) throw std::runtime_error("orient_select: K must be 2 or 4");
  hipLaunchKernelGGL(orient_select_kernel, dim3(pages), dim3(256), 0, s, ids, prob, conf, cids, cprob, cconf, first, N, K, per_page, side);
}

}  // namespace ttr
