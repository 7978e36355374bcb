// Barcodes (DESIGN.md "Barcodes"): Code 128 and Code 39 read off single lines of the pages' ink bitmaps in all four directions, the lines' hits chained into
// barcodes, and every item's barcode.
//
// barcode_scan_kernel  the line pass.  pages x bands of 32 lines, 256 threads; a page's lines are its Hcap rows (bits), then its Wcap columns (bitsT).  Thread t
//                      owns line t / 8 of the band and the t % 8-th eighth of the line's words, so lane order IS position order.  For either reading a thread
//                      forms its words' candidates (bc_candidates: shifts and an and a word), tests each one's first six runs in line, puts the few that pass
//                      through steps 4 - 5 out of line (bc_decode, barcodes_rule.h: ctz / clz over the runs, the lookup tables in LDS) and counts its hits; the counts are scanned over the line's eight lanes, and a second walk
//                      writes the hits into the line's eight slots in order.  out: hits [page][line][2][8][20] and cnt [page][line][2][4] = kept, dropped,
//                      candidates, starts.  A line is read through its own ceil(len / 64) words and never beyond; a line beyond the page has four zero counters.
// barcode_page_kernel  one workgroup of 256 per page: sums the counters, gives every hit its partner (bc_pred) and its chain's first hit, has every first hit
//                      collect its chain (bc_chain), keeps the chains of min_lines hits in LDS through a block scan, ranks them in (y0, x0, dir) order into the
//                      side block, applies the cap, then a thread an item for the items' barcodes (bc_item).
// No atomic anywhere: every slot is a scan's or a rank's.  Integer arithmetic only: the outputs are the host rule's (geometry.cpp: barcodes_from_bits,
// barcodes_items) bit for bit.
#include "common.h"
#include "kernels.h"
#include "barcodes_rule.h"
#include "page_table.h"

namespace ttr {

namespace {

constexpr int kBcThreads = 256, kBcSegs = kBcThreads / kBcBandLines;
static_assert(kBcSegs == 8, "a line's lanes are eight of a wave: the shuffles below are eight wide");

// exclusive scan of one value per thread over the workgroup of 256; *total = the sum.  Two barriers.
__device__ __forceinline__ int bc_scan(int v, int* wsum, int tid, int* total) {
  const int lane = tid & 63, wv = tid >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < kBcThreads / 64; ++k) { const int s = wsum[k]; base += k < wv ? s : 0; tot += s; }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}
// the sum of v over the line's eight lanes
__device__ __forceinline__ int bc_sum8(int v) {
  for (int d = 1; d < kBcSegs; d <<= 1) v += __shfl_xor(v, d, kBcSegs);
  return v;
}

// steps 4 - 5 on one candidate, out of line and in one copy: almost every candidate dies at its first six runs, and the walk's registers are not the scan's
__device__ __noinline__ bool bc_decode_one(const uint8_t* tab, const uint64_t* line, int len, int rev, int u0, int symbologies, int32_t* hit, int* starts) {
  return bc_decode(tab, line, len, rev, u0, symbologies, hit, starts);
}

// a thread's words [k0, k1) of one line under one reading: counts its hits (slots null), or writes them from slot `at` on and stops behind the `want`-th
__device__ __forceinline__ int bc_walk(const uint8_t* tab, const uint64_t* line, int len, int nw, int rev, int k0, int k1, int symbologies, int32_t* slots, int at, int want,
                                    int* cands, int* starts) {
  int hits = 0;
  for (int k = k0; k < k1 && hits < want; ++k) {
    uint64_t c = bc_candidates(line, nw, k, rev);
    *cands += mark_popc(c);
    while (c && hits < want) {
      const int x = 64 * k + mark_ctz(c);
      c &= c - 1;
      const int u0 = rev ? len - 1 - x : x;
      // the start test, in line: the candidate's first six runs must be a Code 128 start or the first six of Code 39's `*` (narrow, wide, narrow, narrow,
      // wide, narrow - a wide run is longer than every narrow one, whatever the three runs behind them are).  Necessary for either decode, so the counters
      // and the hits are the rule's; almost every candidate ends here
      int r[6];
      const int S = bc_read(line, len, rev, u0, 6, r);
      if (!S) continue;
      bool maybe = false;
      if (symbologies & 1) { const int v = bc128_value(tab, r, S); maybe = v >= 103 && v <= 105; }
      if (!maybe && (symbologies & 2))
        maybe = r[1] > r[0] && r[1] > r[2] && r[1] > r[3] && r[1] > r[5] && r[4] > r[0] && r[4] > r[2] && r[4] > r[3] && r[4] > r[5];
      if (!maybe) continue;
      // (a decode that fails may have begun a text: a slot is handed over only once the candidate is known to hit, or a lane that has written its last hit
      // would scribble on the next slot, which is the next lane's)
      if (!bc_decode_one(tab, line, len, rev, u0, symbologies, nullptr, starts)) continue;
      if (slots && at + hits < kBcLineHits) {
        int32_t* const out = slots + (size_t)(at + hits) * kBcHit;
        int unused = 0;
        (void)bc_decode_one(tab, line, len, rev, u0, symbologies, out, &unused);
        out[6] = -1; out[7] = -1;
      }
      ++hits;
    }
  }
  return hits;
}

}  // namespace

__global__ __launch_bounds__(kBcThreads) void barcode_scan_kernel(const unsigned long long* __restrict__ bits_all, const unsigned long long* __restrict__ bitsT_all, int h_, int w_,
                                                                  const PageRow* __restrict__ table, int Hcap, int Wcap, int bands, int symbologies, int* __restrict__ hits_all,
                                                                  int* __restrict__ cnt_all) {
  __shared__ uint8_t tab[kBcTableBytes];
  const int pg = (int)blockIdx.y, band = (int)blockIdx.x, tid = (int)threadIdx.x;
  bc_tables_clear(tab, tid, kBcThreads);
  __syncthreads();
  bc_tables_fill(tab, tid, kBcThreads);
  __syncthreads();
  const int h = table ? table[pg].h : h_, w = table ? table[pg].w : w_;
  const int nwx = (w + 63) >> 6, nwy = (h + 63) >> 6, lines = Hcap + Wcap;
  const int L = band * kBcBandLines + tid / kBcSegs, seg = tid % kBcSegs;
  const bool col = L >= Hcap;
  const bool live = L < lines && (col ? L - Hcap < w : L < h);          // (the launch covers the largest page of a mixed batch)
  const uint64_t* const line = !live ? nullptr
                               : col ? reinterpret_cast<const uint64_t*>(bitsT_all) + (size_t)pg * ((size_t)Wcap * (size_t)((Hcap + 63) >> 6)) + (size_t)(L - Hcap) * nwy
                                     : reinterpret_cast<const uint64_t*>(bits_all) + (size_t)pg * ((size_t)Hcap * (size_t)((Wcap + 63) >> 6)) + (size_t)L * nwx;
  const int len = col ? h : w, nw = col ? nwy : nwx;
  const int per = (nw + kBcSegs - 1) / kBcSegs;
  const int k0 = seg * per, k1 = live ? (k0 + per < nw ? k0 + per : nw) : 0;   // this thread's words [k0, k1) of its line; none beyond the page
  for (int rev = 0; rev < 2; ++rev) {
    int cands = 0, starts = 0, unused = 0;
    const int mine = bc_walk(tab, line, len, nw, rev, k0, k1, symbologies, nullptr, 0, 0x7fffffff, &cands, &starts);
    int inc = mine;
    for (int d = 1; d < kBcSegs; d <<= 1) { const int t = __shfl_up(inc, d, kBcSegs); if (seg >= d) inc += t; }
    const int total = bc_sum8(mine), all_cands = bc_sum8(cands), all_starts = bc_sum8(starts);
    if (L >= lines) continue;
    const size_t q = (size_t)pg * lines * 2 + (size_t)(2 * L + rev);
    if (seg == 0) {
      int* const c = cnt_all + q * kBcCnt;
      c[0] = total < kBcLineHits ? total : kBcLineHits; c[1] = total < kBcLineHits ? 0 : total - kBcLineHits; c[2] = all_cands; c[3] = all_starts;
    }
    if (mine && inc - mine < kBcLineHits) (void)bc_walk(tab, line, len, nw, rev, k0, k1, symbologies, hits_all + q * (kBcLineHits * kBcHit), inc - mine, mine, &unused, &unused);
  }
}

__global__ __launch_bounds__(kBcThreads) void barcode_page_kernel(int* hits_all, const int* __restrict__ cnt_all, int h_, int w_, const PageRow* __restrict__ table,
                                                                  int Hcap, int Wcap, int min_lines, const int* __restrict__ centres, const int* __restrict__ first, int* side_all,
                                                                  int* item_barcode) {
  __shared__ int wsum[kBcThreads / 64];
  __shared__ int32_t list[kBcCap][kBcRec];
  __shared__ int ids[kBcCap];
  const int pg = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int h = table ? table[pg].h : h_, w = table ? table[pg].w : w_;
  const int lines = Hcap + Wcap, pairs = 2 * lines;
  int32_t* const hits = hits_all + (size_t)pg * pairs * (kBcLineHits * kBcHit);
  const int32_t* const cnt = cnt_all + (size_t)pg * pairs * kBcCnt;
  int* const side = side_all + (size_t)pg * kBcSideInts;
  // the header's counters
  int sums[4] = {0, 0, 0, 0};
  for (int q0 = 0; q0 < pairs; q0 += kBcThreads) {
    const int q = q0 + tid;
    for (int j = 0; j < 4; ++j) { int t; (void)bc_scan(q < pairs ? cnt[kBcCnt * q + j] : 0, wsum, tid, &t); sums[j] += t; }
  }
  // 7: every hit's partner, then its chain's first hit.  A line of the page's own (others have no hits) chains inside its kind: rows 0..h - 1, columns Hcap..Hcap + w - 1
  for (int q = tid; q < pairs; q += kBcThreads) {
    const int L = q >> 1, rev = q & 1;
    for (int s = 0; s < cnt[kBcCnt * q]; ++s) hits[(size_t)(q * kBcLineHits + s) * kBcHit + 6] = bc_pred(hits, cnt, L < Hcap ? 0 : Hcap, L, rev, s);
  }
  __syncthreads();
  for (int q = tid; q < pairs; q += kBcThreads)
    for (int s = 0; s < cnt[kBcCnt * q]; ++s) {
      int root = q * kBcLineHits + s;
      for (int p = hits[(size_t)root * kBcHit + 6]; p >= 0; p = hits[(size_t)root * kBcHit + 6]) root = p;
      hits[(size_t)(q * kBcLineHits + s) * kBcHit + 7] = root;
    }
  __syncthreads();
  // 7 - 8: the chains of min_lines hits or more, into LDS in thread order, then ranked
  int n = 0, below = 0;
  int32_t rec[kBcRec];
  for (int q0 = 0; q0 < pairs; q0 += kBcThreads) {
    const int q = q0 + tid, L = q >> 1, rev = q & 1;
    const int L0 = L < Hcap ? 0 : Hcap, L1 = L < Hcap ? h : Hcap + w;
    int keep = 0, low = 0;
    if (q < pairs)
      for (int s = 0; s < cnt[kBcCnt * q]; ++s) {
        if (hits[(size_t)(q * kBcLineHits + s) * kBcHit + 6] >= 0) continue;
        if (bc_chain(hits, cnt, L0, L1, L, rev, s, L >= Hcap, rec) >= min_lines) ++keep; else ++low;
      }
    int total, lows;
    int at = n + bc_scan(keep, wsum, tid, &total);
    (void)bc_scan(low, wsum, tid, &lows);
    n += total; below += lows;
    if (keep)
      for (int s = 0; s < cnt[kBcCnt * q]; ++s) {
        if (hits[(size_t)(q * kBcLineHits + s) * kBcHit + 6] >= 0) continue;
        for (int j = 0; j < kBcRec; ++j) rec[j] = 0;
        if (bc_chain(hits, cnt, L0, L1, L, rev, s, L >= Hcap, rec) < min_lines) continue;
        if (at < kBcCap) {
          for (int j = 0; j < kBcRec; ++j) list[at][j] = rec[j];
          ids[at] = q * kBcLineHits + s;
        }
        ++at;
      }
  }
  __syncthreads();
  const bool over = n > kBcCap;
  if (!over && tid < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += j != tid && bc_before(list[j], ids[j], list[tid], ids[tid]) ? 1 : 0;
    for (int j = 0; j < kBcRec; ++j) side[kBcHdr + rank * kBcRec + j] = list[tid][j];
  }
  if (tid < kBcHdr)
    side[tid] = tid == 0 ? (over ? -7 : 1) : tid == 1 ? (over ? 0 : n) : tid == 2 ? sums[2] : tid == 3 ? sums[3] : tid == 4 ? sums[0] : tid == 5 ? sums[1] : tid == 6 ? below : 0;
  __syncthreads();                                                       // (the records and the header, written above, are read below)
  // 9: the items' barcodes
  const int i0 = first[pg], ni = first[pg + 1] - i0;
  for (int i = tid; i < ni; i += kBcThreads) item_barcode[i0 + i] = bc_item(side, centres[2 * (i0 + i)], centres[2 * (i0 + i) + 1]);
}

void launch_barcode_scan(const uint64_t* bits, const uint64_t* bitsT, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int symbologies, int* hits, int* cnt,
                         hipStream_t s) {
  if (pages <= 0) return;
  if (Hcap <= 0 || Wcap <= 0 || Hcap >= 32768 || Wcap >= 32768 || (!table && (h > Hcap || w > Wcap))) throw std::runtime_error("barcode_scan: a page side outside 1..32767");
  if (!barcodes_args_ok(kBcMinLo, 128, symbologies)) throw std::runtime_error("barcode_scan: bad parameters");
  const int bands = barcodes_bands(Hcap, Wcap);
  hipLaunchKernelGGL(barcode_scan_kernel, dim3(bands, pages), dim3(kBcThreads), 0, s, reinterpret_cast<const unsigned long long*>(bits),
                     reinterpret_cast<const unsigned long long*>(bitsT), h, w, table, Hcap, Wcap, bands, symbologies, hits, cnt);
}

void launch_barcode_page(int* hits, const int* cnt, int h, int w, const PageRow* table, int pages, int Hcap, int Wcap, int min_lines, const int* centres, const int* first,
                         int* side, int* item_barcode, hipStream_t s) {
  if (pages <= 0) return;
  if (min_lines < kBcMinLo || min_lines > kBcMinHi) throw std::runtime_error("barcode_page: bad parameters");
  hipLaunchKernelGGL(barcode_page_kernel, dim3(pages), dim3(kBcThreads), 0, s, hits, cnt, h, w, table, Hcap, Wcap, min_lines, centres, first, side, item_barcode);
}

}  // namespace ttr
