// Tables (DESIGN.md "Tables"): the constants, the side block's layout, the predicates of steps 1 - 5 and the whole of steps 6 - 7 of the rule, one statement of
// each, shared by the host rule (geometry.cpp: tables_from_page) and the two kernels (tables.hip).  Steps 2 - 5 are loops on the host and parallel passes in
// table_grid_kernel, both over the predicates below; steps 6 - 7 work on a few hundred rulings at the most and are one function, tables_grid, which the host
// calls and which one lane of the kernel runs on the side block, so the two agree bit for bit by construction.  Integer arithmetic only; every value is below
// 2^21.  tests/tables_ref.py restates all of it in Python integers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TTR_TAB_HD __host__ __device__ inline
#else
#define TTR_TAB_HD inline
#endif

namespace ttr {

constexpr int kTabR = 12, kTabJ = 6;                       // the shortest run; the join tolerance in px
constexpr int kTabRunCap = 8192, kTabRulingCap = 256;      // per direction and page
constexpr int kTabTableCap = 32, kTabLineCap = 64;         // tables per page; lines per axis and table
constexpr int kTabCellCap = 1024;                          // cells per page
constexpr int kTabMinLenLo = 16, kTabMinLenHi = 4096;

// The side block of one page, int32: a header, then fixed-capacity arrays.
//   header  [0] mode (1, or -(step) of the cap that overflowed)  [1] nh  [2] nv  [3] tables  [4] cells  [5] horizontal runs  [6] vertical runs
//   rulings [2 * 256][6]  dir (0 = horizontal, 1 = vertical), x0, y0, x1, y1 (inclusive), table; the nh horizontal ones first, then the nv vertical ones
//   tables  [32][8]       x0, y0, x1, y1, rows, cols, first cell, cell count
//   lines   [32][2][64]   per table its rows + 1 row lines, then its cols + 1 column lines, in doubled px
//   cells   [1024][9]     table, row, col, rowspan, colspan, x0, y0, x1, y1
constexpr int kTabHdr = 16;
constexpr int kTabRulings = kTabHdr, kTabTables = kTabRulings + 2 * kTabRulingCap * 6, kTabLines = kTabTables + kTabTableCap * 8;
constexpr int kTabCells = kTabLines + kTabTableCap * 2 * kTabLineCap, kTabSideInts = kTabCells + kTabCellCap * 9;
constexpr int kTabScratchInts = 32768;                     // what tables_grid needs beside the block
// a batch's side blocks: [pages][kTabSideInts] | [N][2] every word's table, cell
constexpr size_t tables_side_bytes(int pages, int N) { return ((size_t)pages * kTabSideInts + (size_t)N * 2) * 4; }

// 1: ink.  s = the sum of a pixel's three bytes
TTR_TAB_HD bool tab_ink(int s, int ink) { return s < 3 * ink; }
// 3: two runs [a0, a1], [b0, b1] of one direction on adjacent lines link (8-connectivity)
TTR_TAB_HD bool tab_link(int a0, int a1, int b0, int b1) { return a0 <= b1 + 1 && b0 <= a1 + 1; }
// 4: a component of length L, thickness T and area A is a ruling
TTR_TAB_HD bool tab_is_ruling(int L, int T, int A, int min_len) { return L >= min_len && 8 * T <= L && A <= 16 * L; }
// 5: a horizontal ruling h and a vertical ruling v (x0, y0, x1, y1 at [1..4]) meet
TTR_TAB_HD bool tab_meet(const int32_t* h, const int32_t* v) {
  return v[1] - kTabJ <= h[3] && h[1] <= v[3] + kTabJ && h[2] - kTabJ <= v[4] && v[2] <= h[4] + kTabJ;
}
// 8: the cell of a word at (cx, cy) = 64 x its centre; out[0] = table, out[1] = cell, -1 / -1 outside every table
TTR_TAB_HD void tab_word_cell(const int32_t* side, int cx, int cy, int32_t* out) {
  out[0] = -1; out[1] = -1;
  if (side[0] != 1) return;
  for (int t = 0; t < side[3]; ++t) {
    const int32_t* T = side + kTabTables + 8 * t;
    const int32_t* Y = side + kTabLines + 2 * kTabLineCap * t;
    const int32_t* X = Y + kTabLineCap;
    const int rows = T[4], cols = T[5];
    if (cx < 32 * X[0] || cx >= 32 * X[cols] || cy < 32 * Y[0] || cy >= 32 * Y[rows]) continue;
    int i = 0, j = 0;
    while (cy >= 32 * Y[i + 1]) ++i;
    while (cx >= 32 * X[j + 1]) ++j;
    for (int c = T[6]; c < T[6] + T[7]; ++c) {
      const int32_t* C = side + kTabCells + 9 * c;
      if (i >= C[1] && i < C[1] + C[3] && j >= C[2] && j < C[2] + C[4]) { out[0] = t; out[1] = c; return; }
    }
    return;   // (cells tile the grid: not reached)
  }
}

TTR_TAB_HD int tab_find(int32_t* parent, int i) {
  while (parent[i] != i) i = parent[i];
  return i;
}
TTR_TAB_HD bool tab_union(int32_t* parent, int a, int b) {   // the smaller root wins; true when two components became one
  a = tab_find(parent, a); b = tab_find(parent, b);
  if (a == b) return false;
  if (a < b) parent[b] = a; else parent[a] = b;
  return true;
}

// The lines of one axis of one candidate table: its n rulings (indices into the ruling list, ascending) in list[], each one's doubled centre in key[].
// Sorts list by (key, index), chains while consecutive keys differ by at most 2 J, writes each line's position (smallest + largest) / 2 to pos[] and each
// ruling's line to line_of[].  Returns the number of lines, or kTabLineCap + 1 when there are more than the cap.
TTR_TAB_HD int tab_chain(int32_t* list, int n, const int32_t* key, int32_t* line_of, int32_t* pos) {
  for (int a = 1; a < n; ++a) {   // insertion sort: stable, so equal keys stay in index order
    const int r = list[a];
    int b = a;
    while (b > 0 && key[list[b - 1]] > key[r]) { list[b] = list[b - 1]; --b; }
    list[b] = r;
  }
  int nl = 0, lo = 0;
  for (int a = 0; a < n; ++a) {
    const int k = key[list[a]];
    if (a == 0 || k - key[list[a - 1]] > 2 * kTabJ) {
      if (nl == kTabLineCap) return kTabLineCap + 1;
      lo = k; ++nl;
    }
    pos[nl - 1] = (lo + k) / 2;
    line_of[list[a]] = nl - 1;
  }
  return nl;
}

// Steps 6 - 7.  In: side[1] = nh, side[2] = nv and the nh + nv rulings, each one's table field holding the root of its component of the meet graph (the
// smallest ruling index in it; horizontal rulings count from 0, vertical ones from nh).  Out: the rulings' table fields, the tables, lines and cells and
// side[3], side[4].  Returns 1, or -6 / -7 when a cap of that step overflows (the block is then left half written: the caller clears it).
TTR_TAB_HD int tables_grid(int32_t* side, int32_t* scratch) {
  const int nh = side[1], nv = side[2], n = nh + nv;
  int32_t* const rul = side + kTabRulings;
  int32_t* const cnt_h = scratch;                  // [512] members per root
  int32_t* const cnt_v = cnt_h + 2 * kTabRulingCap;
  int32_t* const key = cnt_v + 2 * kTabRulingCap;     // [512] doubled centre
  int32_t* const line_of = key + 2 * kTabRulingCap;   // [512]
  int32_t* const list = line_of + 2 * kTabRulingCap;  // [512]
  int32_t* const comp = list + 2 * kTabRulingCap;     // [512] a copy of the roots
  int32_t* const ttab = comp + 2 * kTabRulingCap;     // [32][8] candidate tables in root order: box, rows, cols, root, -
  int32_t* const tlin = ttab + kTabTableCap * 8;      // [32][2][64]
  int32_t* const par = tlin + kTabTableCap * 2 * kTabLineCap;   // [4096] base cells
  int32_t* const br0 = par + 4096;                    // [4096] x 4: a component's base-cell box
  int32_t* const br1 = br0 + 4096;
  int32_t* const bc0 = br1 + 4096;
  int32_t* const bc1 = bc0 + 4096;
  side[3] = 0; side[4] = 0;
  for (int r = 0; r < n; ++r) { cnt_h[r] = 0; cnt_v[r] = 0; comp[r] = rul[6 * r + 5]; rul[6 * r + 5] = -1; line_of[r] = -1; }
  for (int r = 0; r < n; ++r) {
    if (r < nh) { ++cnt_h[comp[r]]; key[r] = rul[6 * r + 2] + rul[6 * r + 4]; }
    else { ++cnt_v[comp[r]]; key[r] = rul[6 * r + 1] + rul[6 * r + 3]; }
  }
  // 6: grid lines of every component with at least two rulings of either direction
  int nt = 0;
  for (int root = 0; root < n; ++root) {
    if (comp[root] != root || cnt_h[root] < 2 || cnt_v[root] < 2) continue;
    // (a 33rd candidate overflows only if it survives the chaining, so it is chained too: into br0 / br1, which are free until step 7)
    int32_t* const Y = nt < kTabTableCap ? tlin + 2 * kTabLineCap * nt : br0;
    int32_t* const X = nt < kTabTableCap ? Y + kTabLineCap : br1;
    int m = 0;
    for (int r = root; r < nh; ++r) if (comp[r] == root) list[m++] = r;
    const int rows1 = tab_chain(list, m, key, line_of, Y);
    if (rows1 > kTabLineCap) return -6;
    int x0 = 32768, y0 = 32768, x1 = -1, y1 = -1;
    for (int a = 0; a < m; ++a) {
      const int32_t* q = rul + 6 * list[a];
      x0 = q[1] < x0 ? q[1] : x0; y0 = q[2] < y0 ? q[2] : y0; x1 = q[3] > x1 ? q[3] : x1; y1 = q[4] > y1 ? q[4] : y1;
    }
    m = 0;
    for (int r = nh; r < n; ++r) if (comp[r] == root) list[m++] = r;
    const int cols1 = tab_chain(list, m, key, line_of, X);
    if (cols1 > kTabLineCap) return -6;
    for (int a = 0; a < m; ++a) {
      const int32_t* q = rul + 6 * list[a];
      x0 = q[1] < x0 ? q[1] : x0; y0 = q[2] < y0 ? q[2] : y0; x1 = q[3] > x1 ? q[3] : x1; y1 = q[4] > y1 ? q[4] : y1;
    }
    if (rows1 < 2 || cols1 < 2) {   // dropped: its rulings stay loose
      for (int r = root; r < n; ++r) if (comp[r] == root) line_of[r] = -1;
      continue;
    }
    if (nt == kTabTableCap) return -6;
    int32_t* T = ttab + 8 * nt;
    T[0] = x0; T[1] = y0; T[2] = x1; T[3] = y1; T[4] = rows1 - 1; T[5] = cols1 - 1; T[6] = root; T[7] = 0;
    ++nt;
  }
  // ... numbered by (y0, x0, root): candidates are in root order, so the rank is a count
  for (int a = 0; a < nt; ++a) {
    const int32_t* A = ttab + 8 * a;
    int rank = 0;
    for (int b = 0; b < nt; ++b) {
      const int32_t* B = ttab + 8 * b;
      rank += (B[1] < A[1] || (B[1] == A[1] && (B[0] < A[0] || (B[0] == A[0] && b < a)))) ? 1 : 0;
    }
    int32_t* T = side + kTabTables + 8 * rank;
    for (int k = 0; k < 6; ++k) T[k] = A[k];
    T[6] = 0; T[7] = 0;
    int32_t* L = side + kTabLines + 2 * kTabLineCap * rank;
    for (int k = 0; k < 2 * kTabLineCap; ++k) L[k] = tlin[2 * kTabLineCap * a + k];
    for (int r = A[6]; r < n; ++r) if (comp[r] == A[6]) rul[6 * r + 5] = rank;
  }
  side[3] = nt;
  // 7: cells, table by table
  int nc = 0;
  for (int t = 0; t < nt; ++t) {
    int32_t* T = side + kTabTables + 8 * t;
    const int32_t* Y = side + kTabLines + 2 * kTabLineCap * t;
    const int32_t* X = Y + kTabLineCap;
    const int rows = T[4], cols = T[5], nb = rows * cols;
    for (int b = 0; b < nb; ++b) par[b] = b;
    for (int i = 0; i < rows; ++i)
      for (int j = 0; j < cols; ++j) {
        if (j + 1 < cols) {   // the border to (i, j + 1): a vertical ruling of column line j + 1 across the row's middle
          const int mid = (Y[i] + Y[i + 1]) / 2;
          bool present = false;
          for (int r = nh; r < n && !present; ++r)
            present = rul[6 * r + 5] == t && line_of[r] == j + 1 && 2 * (rul[6 * r + 2] - kTabJ) <= mid && mid <= 2 * (rul[6 * r + 4] + kTabJ);
          if (!present) tab_union(par, i * cols + j, i * cols + j + 1);
        }
        if (i + 1 < rows) {   // the border to (i + 1, j): a horizontal ruling of row line i + 1 across the column's middle
          const int mid = (X[j] + X[j + 1]) / 2;
          bool present = false;
          for (int r = 0; r < nh && !present; ++r)
            present = rul[6 * r + 5] == t && line_of[r] == i + 1 && 2 * (rul[6 * r + 1] - kTabJ) <= mid && mid <= 2 * (rul[6 * r + 3] + kTabJ);
          if (!present) tab_union(par, i * cols + j, (i + 1) * cols + j);
        }
      }
    // a component that is not a rectangle takes in its bounding box, until every component is one: the cells then tile the grid
    for (bool changed = true; changed;) {
      changed = false;
      for (int b = 0; b < nb; ++b) { br0[b] = rows; br1[b] = -1; bc0[b] = cols; bc1[b] = -1; }
      for (int b = 0; b < nb; ++b) {
        const int r = tab_find(par, b), i = b / cols, j = b % cols;
        br0[r] = i < br0[r] ? i : br0[r]; br1[r] = i > br1[r] ? i : br1[r]; bc0[r] = j < bc0[r] ? j : bc0[r]; bc1[r] = j > bc1[r] ? j : bc1[r];
      }
      for (int b = 0; b < nb; ++b) {
        if (par[b] != b || br1[b] < 0) continue;
        for (int i = br0[b]; i <= br1[b]; ++i)
          for (int j = bc0[b]; j <= bc1[b]; ++j) changed = tab_union(par, b, i * cols + j) || changed;
      }
    }
    T[6] = nc;
    for (int b = 0; b < nb; ++b) {   // roots in row-major order: a cell's first base cell
      if (par[b] != b) continue;
      if (nc == kTabCellCap) return -7;
      int32_t* C = side + kTabCells + 9 * nc;
      C[0] = t; C[1] = br0[b]; C[2] = bc0[b]; C[3] = br1[b] - br0[b] + 1; C[4] = bc1[b] - bc0[b] + 1;
      C[5] = X[bc0[b]] / 2; C[6] = Y[br0[b]] / 2; C[7] = X[bc1[b] + 1] / 2; C[8] = Y[br1[b] + 1] / 2;
      ++nc;
    }
    T[7] = nc - T[6];
  }
  side[4] = nc;
  return 1;
}

// what a page that overflowed a cap reports: the mode, and nothing else
TTR_TAB_HD void tables_clear(int32_t* side, int mode) {
  for (int k = 0; k < kTabHdr; ++k) side[k] = 0;
  side[0] = mode;
}

}  // namespace ttr
