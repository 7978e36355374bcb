// Host-side geometry and text decoding of the engine (no GPU, no OpenCV).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tile_plan.h"

namespace ttr {

// cv::RotatedRect stand-in: centre, size, angle in degrees, all float32.
struct RRect { float cx = 0, cy = 0, w = 0, h = 0, angle = 0; };
struct Pt2f { float x, y; };

void rect_points(const RRect& r, Pt2f pt[4]);                 // cv::RotatedRect::points      (tuatara.cpp:181,:241,:258)
void bounding_rect(const RRect& r, int xywh[4]);              // cv::RotatedRect::boundingRect (tuatara.cpp:416)
void tesseract_bbox(const RRect& r, float bbox[4]);           // rotated_rect_to_tesseract_format (tuatara.cpp:256-274)
RRect min_area_rect(const Pt2f* pts, int n);                  // cv::minAreaRect              (tuatara.cpp:179,:248)
// the tail of cv::minAreaRect behind the hull: kind 1 = the rotating calipers' raw result out[6] (corner + two side vectors), 3 = a two-point hull
// (x0, y0, x1, y1), 4 = one point -> centre, sides (double sqrt), angle (double atan2, degrees).  min_area_rect ends in it; the GPU calipers
// (post_ops.hip: ccl_rects_kernel) hand their raw result to it, so that sqrt / atan2 are the host's libm on both paths
RRect finish_min_area_rect(int kind, const float v[6]);
RRect adjust_coordinates(const RRect& r, float ratio_w, float ratio_h, float ratio_net = 2.f);  // tuatara.cpp:236-253

// Rectified crops (ttr_config.crop_mode = TTR_CROP_RECTIFIED; DESIGN.md "Rectified crops").  quad = the word's corners tl, tr, br, bl
// (clockwise on screen, fp32 from rect_points): the baseline tl -> tr is the side nearest horizontal, skew in [-45, 45] degrees, x
// component positive; tl -> bl points down.  coef = {X0, Ax, Bx, Y0, Ay, By} in image pixels: output pixel (u, v) of the 32 x 128 crop
// samples (X0 + u Ax + v Bx, Y0 + u Ay + v By).  Returns the crop kind: 0 when r.angle is a multiple of 90 (the boundingRect crop,
// bit for bit the reference's), else 1 (the affine sampler, post_ops.hip: pack_crops_rect_kernel).
int deskew_quad(const RRect& r, Pt2f quad[4], double coef[6]);
// the coefficients as the kernel takes them: llrint to int64 in units of 2^-16 px
void deskew_fixed(const double coef[6], int64_t fixed[6]);
// the quad -> coefficients step of deskew_quad on its own (any quad tl, tr, br, bl): the sampler's rule in double, in deskew_quad's order
void quad_coef(const Pt2f quad[4], double coef[6]);

// Regions (DESIGN.md "Regions and per-row character sets"): a caller's quad tl, tr, br, bl as 8 floats in image pixels.  region_quad_ok: every coordinate is
// finite and has |x| < 32768 (the bound of the other quad rules).  region_coef: quad_coef on the floats, then deskew_fixed - the kind-1 crop's coefficients.
// region_bbox: {min x, min y, max x, max y} of the four corners.  region_inside: every corner within the page's pixel edges [-0.5, w - 0.5] x [-0.5, h - 0.5].
bool region_quad_ok(const float* quad8);
void region_coef(const float* quad8, int64_t fixed[6]);
void region_bbox(const float* quad8, float bbox[4]);
bool region_inside(const float* quad8, int h, int w);

// Word orientation (ttr_config.orient; DESIGN.md "Word orientation").  A turn t = the quarter turns clockwise by which the word lies on the
// page.  box_edge_quad: the crop_mode = 0 quad of a clamped boundingRect [x0, x1) x [y0, y1) as pixel edges (rect_points' coordinates:
// pixel centres at integers).  turn_coef: the fixed-point coefficients of the turned quad Q_t[k] = Q[(k + t) mod 4] (quad_coef +
// deskew_fixed), sampled by the kind-1 rule.
void box_edge_quad(int x0, int y0, int x1, int y1, Pt2f quad[4]);
void turn_coef(const Pt2f quad[4], int turn, int64_t fixed[6]);
// The choice between the k candidate readings of n words of one page (orient_select_kernel, orient.hip, makes the same choice): conf [n][k],
// ids [n][k][26], candidates in ascending turn order ({0}, {0, 2} or {0, 1, 2, 3}) -> turns[n], *page_turn as turns 0..3.  Per word: the
// largest conf, strict > in ascending order.  Page: argmax of the votes of the words whose winning text has >= 2 characters (|S| of the
// confidence rule), ties to the lower turn, 0 without votes; per_page: every turn = it.
void orient_select(const float* conf, const int32_t* ids, int n, int k, int per_page, int32_t* turns, int32_t* page_turn);

// Text lines (ttr_config.lines; DESIGN.md "Text lines").  lines_cuv: one quad tl, tr, br, bl (8 floats, image pixels) in the rule's fixed point
// (llrint(16 x) per coordinate) -> cuv = {c.x, c.y, u.x, u.y, v.x, v.y}: c = tl + tr + br + bl (4 x the centre), u = (tr - tl) + (br - bl) (2 x the
// width vector), v = (bl - tl) + (br - tr) (2 x the height vector).  Returns false for a coordinate that is not finite or has |x| >= 32768 (every
// product of the rule then stays far inside int64).  lines_from_cuv: the rule on n words of ONE page (line_group_kernel, lines.hip, computes the
// same): line[n] = each word's line in line order, word[n] = its position inside its line, *n_lines.  Integer arithmetic only.
bool lines_cuv(const float* quad8, int32_t cuv[6]);
void lines_from_cuv(const int32_t* cuv, int n, int32_t* line, int32_t* word, int32_t* n_lines);
// ... derived from line / word: order[n] = the item indices in reading order (each line's members consecutive, in word order) and
// line_first[n_lines + 1] = the lines' offsets into it.  Returns false when line / word are not a numbering of n_lines non-empty lines.
bool lines_reading_order(const int32_t* line, const int32_t* word, int n, int n_lines, int32_t* order, int32_t* line_first);

// Text blocks (ttr_config.blocks; DESIGN.md "Text blocks").  blocks_from_lines: the rule on ONE page from the words' cuv and the line rule's
// outputs (block_group_kernel, blocks.hip, computes the same): block[l] = the rank of line l's block in reading order, pos[l] = the line's rank
// inside its block, for l < n_lines (both arrays hold n entries, the rest is -1: lines never outnumber words), *n_blocks, *mode = 1 when the
// blocks are ordered by the precedence relation, 0 when there are more than kBlocksMaxOrdered and they are ordered by their keys alone.
constexpr int kBlocksMaxOrdered = 512;
void blocks_from_lines(const int32_t* cuv, int n, const int32_t* line, const int32_t* word, int n_lines, int32_t* block, int32_t* pos, int32_t* n_blocks,
                       int32_t* mode);
// ... derived from block / pos: order[n_lines] = the line indices in block reading order (each block's lines consecutive, by pos) and
// block_first[n_blocks + 1].  Returns false when block / pos are not a numbering of n_blocks non-empty blocks.
inline bool blocks_reading_order(const int32_t* block, const int32_t* pos, int n_lines, int n_blocks, int32_t* order, int32_t* block_first) {
  return lines_reading_order(block, pos, n_lines, n_blocks, order, block_first);
}

// Character boxes (ttr_config.chars; DESIGN.md "Character boxes").  The word's profile is the normalised region map sampled on a 128 x 16 grid
// over the turned quad Q'[j] = Q[(j + t) mod 4] (column maximum, as a byte); the K cells are cut from it.  Constants of the rule:
constexpr int kCharsU = 128, kCharsV = 16, kCharsLam = 64, kCharsMax = 26;
// |S| of the confidence rule: the characters of a row of 26 ids (positions before the first id 0, id 88 and ids outside [0, 98) dropped)
int text_chars(const int32_t* ids);
// the image-pixel -> heat-pixel scale of a canvas ratio: k = 1 / (double)(ratio_w * 2.f), ratio_w = 1.f / ratio (adjust_coordinates' inverse)
double chars_scale(float ratio);
// one quad (8 floats, tl tr br bl, image pixels) at turn t -> fixed = {X0, Ax, Bx, Y0, Ay, By} in 2^-16 heat pixels: column u, row v samples
// (X0 + u Ax + v Bx, Y0 + u Ay + v By).  Double, one rounding per statement, then llrint(65536 x).  Returns false for a coordinate that is not
// finite or has |x| >= 32768, and for a scale outside (0, 1024] (every sum of the sampler then stays far inside int64).
bool chars_coef(const float* quad8, int turn, double k, int64_t fixed[6]);
// the profile q[128] of one word on T [H2][W2] (char_cut_kernel, chars.hip, computes the same bytes)
void chars_profile(const float* T, int H2, int W2, const int64_t fixed[6], uint8_t q[128]);
// q[128], K (0..26), qlow -> cuts[27] in 1/256 column (b[0..K], -1 beyond K) and *mode (0 uniform, 1 valley cuts).  Integer arithmetic only.
void chars_cuts_from_profile(const uint8_t* q, int K, int qlow, int32_t cuts[27], int32_t* mode);
// the K cells of one word as quads [K][8] (tl, tr, br, bl) and bboxes [K][4] (min x, min y, max x, max y), in double, cast to float
void chars_quads_from_cuts(const float* quad8, int turn, const int32_t* cuts, int K, float* quads, float* bboxes);
// what decode_pages accepts from the device: K + 1 ascending entries in [0, 32768], then -1
bool chars_cuts_valid(const int32_t cuts[27], int K);

// Wide words (ttr_engine_set_wide; DESIGN.md "Wide words").  A quad far wider than the recogniser's 4:1 crop is read in n pieces cut at ink gaps found in
// the page's own pixels.  Constants of the rule: at most kWideMaxPieces pieces, kWideV rows, kWideCols nominal columns per piece, widths in [kWideWLo, kWideWHi].
constexpr int kWideMaxPieces = 16, kWideV = 32, kWideCols = 128, kWideWLo = 64, kWideWHi = 192, kWideMaxU = kWideMaxPieces * kWideCols, kWideInf = 0x3fffffff;
// the setter's domain: 0 (off) or a finite value in [2, 64]
bool wide_aspect_ok(float max_aspect);
// one quad (8 floats tl, tr, br, bl) -> n, the pieces (1 = not wide), and frame = {X0f, Axf, Bxf, Y0f, Ayf, Byf} in 2^-16 px over U = 128 n columns and 32 rows:
// double, one rounding per statement, then llrint(65536 x).  For n = 1 the frame is region_coef's.
int wide_plan(const float* quad8, float max_aspect, int64_t frame[6]);
// the contrast profile q[128 n] of the frame on a page u8 [h][w][3] (row stride in bytes): per column max - min over the 32 rows of R + 2 G + B at the nearest
// pixel, clamped to the page (wide_cut_kernel, wide.hip, computes the same words)
void wide_profile(const uint8_t* image, int h, int w, int stride, const int64_t frame[6], int n, uint16_t* q);
// q[128 n], n (1..16) -> cuts[17]: c_0 = 0 < ... < c_n = 128 n, -1 beyond n.  int32 arithmetic only; ties go to the smallest width.
void wide_cuts_from_profile(const uint16_t* q, int n, int32_t cuts[17]);
// the packer row {1, X0_p, Ax_p, Bx_p, Y0_p, Ay_p, By_p, 0} of the piece over columns [c0, c1) of the frame (int64, arithmetic shifts)
void wide_piece_coef(const int64_t frame[6], int c0, int c1, int64_t row[8]);
// the n pieces' quads [n][8] of a word's quad from its cuts, in double, cast to float
void wide_piece_quads(const float* quad8, const int32_t* cuts, int n, float* quads);
// what decode_pages accepts from the device: c_0 = 0, ascending, c_n = 128 n, every width in [64, 192], -1 beyond n
bool wide_cuts_valid(const int32_t cuts[17], int n);

// Curved words (ttr_engine_set_curved; DESIGN.md "Curved words").  A word set on an arc is straightened along a spine found in the page's own pixels; the integer
// steps live in curve_rule.h, shared with curve_crop_kernel (curve.hip).  What the rule gives for one word:
struct CurveWord {
  int32_t flag;                 // 1 = curved: the crop is resampled along the knot table
  int32_t hb[2];                // the half band of pass 1 (frame rows) and of pass 2 (band rows); 0 = the pass did not run or found no ink
  int32_t spine[2][9];          // the nine spine rows of either pass, in 1/256 row
  int64_t table[9][4];          // the knot table {Cx, Cy, Hx, Hy} in 2^-16 px (zeros when pass 2 did not run)
};
// quad (8 floats tl, tr, br, bl) -> frame = {X0, Ax, Bx, Y0, Ay, By} in 2^-16 px over 128 columns and 64 rows: double, one rounding per statement, llrint(65536 x)
void curve_frame(const float* quad8, int64_t frame[6]);
// the column statistics G | M | first | last, [4][128] int32, of a page u8 [h][w][3] (row stride in bytes): table null = pass 1 over the frame, else pass 2
// over the band of the knot table [9][4]
void curve_columns(const uint8_t* image, int h, int w, int stride, const int64_t frame[6], const int64_t* table, int32_t* stats);
// the whole rule on one frame; table1 (may be null) receives pass 1's knot table [9][4]
void curve_word(const uint8_t* image, int h, int w, int stride, const int64_t frame[6], CurveWord* out, int64_t* table1 = nullptr);
// the crop u8 [32][128][3] of a knot table: the kind-1 sampler's arithmetic at the table's positions
void curve_crop(const uint8_t* image, int h, int w, int stride, const int64_t* table, uint8_t* crop);
// the outline [18][2]: flag != 0: C_j - H_j left to right, then C_j + H_j right to left; else the quad's long sides at the same nine stations
void curve_outline(const float* quad8, int flag, const int64_t* table, float* out36);
// what decode_pages accepts from the device: flag 0 or 1, half bands in 0..32, and with flag 1 every knot's C -+ H inside the int32 pixel range
bool curve_word_valid(const CurveWord& w);

// The ink rule as a value: what forms a page's ink bitmaps for tables, deskew, selection marks and barcodes.  radius 0 = the fixed rule (a pixel is ink when it is
// darker than `ink`, 1..255), else the local rule (DESIGN.md "Local ink") under radius, drop, polarity - `ink` is then not read, and a layer's own range check
// receives 128 in its place.  The *_from_page functions below refuse a local rule that ink_args_ok refuses
struct InkRule {
  int ink = 0, radius = 0, drop = 0, polarity = 0;
  InkRule(int ink_) : ink(ink_) {}   // the fixed rule: a threshold is a rule, so a caller with an `ink` passes it as it is
  static InkRule local(int radius, int drop, int polarity) { InkRule r(0); r.radius = radius; r.drop = drop; r.polarity = polarity; return r; }
  int layer_ink() const { return radius ? 128 : ink; }
};
// bits [h][ceil(w / 64)] and - unless null - bitsT [w][ceil(h / 64)] of a page u8 [h][w][3] under `rule` (tables_ink + marks_transpose, or ink_from_page)
void ink_bits(const uint8_t* image, int h, int w, int stride, const InkRule& rule, uint64_t* bits, uint64_t* bitsT);

// Tables (ttr_engine_set_tables; DESIGN.md "Tables").  Ruling lines are found in the page's own pixels, grouped into tables, each table's grid and merged cells
// derived, and every word given its cell.  The integer steps live in tables_rule.h, shared with table_ink_kernel and table_grid_kernel (tables.hip); the side
// block's layout (kTabSideInts int32) is described there.  All of it is integer arithmetic; min_len must lie in 16..4096 and ink in 1..255.
bool tables_args_ok(int min_len, int ink);
inline size_t tables_bitmap_words(int h, int w) { return (size_t)h * (size_t)((w + 63) / 64); }
// 1: the ink bitmap of a page u8 [h][w][3] (row stride in bytes): bits [h][ceil(w / 64)] uint64, bit x % 64 of word x / 64, zero beyond w
void tables_ink(const uint8_t* image, int h, int w, int stride, int ink, uint64_t* bits);
// 2: the runs of one direction (dir 0: rows, listed in (y, x0) order as {y, x0, x1}; dir 1: columns, in (x, y0) order as {x, y0, y1}) into runs [cap][3];
// returns their number, or kTabRunCap + 1 when there are more than the cap
int tables_runs(const uint64_t* bits, int h, int w, int dir, int32_t* runs);
// 1 - 7 on one page: side receives the block (kTabSideInts int32), runs (may be null) [2][kTabRunCap][3] the run lists, bits (may be null) the bitmap.  Returns
// the mode: 1, or -(step) of the cap that overflowed (the block then holds the mode alone).
int tables_from_page(const uint8_t* image, int h, int w, int stride, int min_len, const InkRule& rule, int32_t* side, int32_t* runs = nullptr, uint64_t* bits = nullptr);
// 8: {cx, cy} = 64 x the centre of a quad (8 floats): the sums of llrint(16 x) over its corners; then the words' cells, out [n][2] = table, cell (-1, -1 outside)
void tables_word_centre(const float* quad8, int32_t c[2]);
void tables_words(const int32_t* side, const int32_t* centres, int n, int32_t* out);
// what decode_pages accepts from the device: a legal mode, counts within the caps, every index in range, lines ascending, and each table's cells tiling its
// base grid exactly once.  why (may be null) receives the reason.
bool tables_side_valid(const int32_t* side, std::string* why = nullptr);
// the counted part of a block as flat arrays: counts [4] = {rulings, tables, cells, line values}, rulings [..][6], tables [..][8], lines (per table its rows + 1
// row lines, then its cols + 1 column lines), cells [..][9]; any output may be null
void tables_export(const int32_t* side, int32_t counts[4], int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells);

// Deskew (ttr_engine_set_deskew; DESIGN.md "Deskew").  A page's skew is estimated from its ink bitmap - the slope k in -M..M (px per 512 px) under which the
// ink's row profile is sharpest - and a page found tilted is resampled upright about its centre, at its own size.  The steps live in deskew_rule.h, shared
// with deskew_score_kernel and deskew_rotate_kernel (deskew.hip); integers throughout, but for the table below.
struct DeskewRec;
// 4: the 257 (C, S) pairs, cs [257][2], pair k + 128 for slope k: llrint(65536 * 512 / d), llrint(65536 k / d), d = sqrt(512^2 + k^2) in double
void deskew_consts(int32_t* cs);
// 2: scores [2 M + 1] of a bitmap as tables_ink forms it (score of slope k at k + M)
void deskew_scores(const uint64_t* bits, int h, int w, int max_slope, uint64_t* scores);
// 3: the record of a page from its scores
void deskew_choose(const uint64_t* scores, int max_slope, int gain, int h, int w, const int32_t* cs, DeskewRec* rec);
// 5: out u8 [h][w][3] (rows out_stride bytes apart) = the page turned by the slope whose constants are C, S
void deskew_resample(const uint8_t* image, int h, int w, int stride, int C, int S, uint8_t* out, int out_stride);
// 1 - 5 on one page; out, rec, scores may be null
void deskew_from_page(const uint8_t* image, int h, int w, int stride, int max_slope, int gain, const InkRule& rule, uint8_t* out, int out_stride, DeskewRec* rec,
                      uint64_t* scores);
// what decode_pages accepts from the device; why (may be null) receives the reason
bool deskew_rec_valid(const DeskewRec& r, int max_slope, int h, int w, const int32_t* cs, std::string* why = nullptr);
// 6: n points (x, y) of the upright page -> the caller's page, computed in double
void deskew_to_page(const DeskewRec& r, const float* xy_in, int n, float* xy_out);

// Local ink (ttr_engine_set_ink; DESIGN.md "Local ink").  The adaptive threshold of ink_rule.h, shared with ink_rows_kernel and ink_local_kernel (ink.hip):
// a pixel is ink when it is darker - or, inverted, lighter - than its window's mean by `drop` 256ths.  radius 1..64, drop 1..255, polarity 0 dark, 1 light, 2 auto.
struct InkRec;
// the bitmap of a page u8 [h][w][3] in tables_ink's layout; bitsT (may be null) [w][ceil(h / 64)] the same bits along y; rec (may be null) the page's record
void ink_from_page(const uint8_t* image, int h, int w, int stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, InkRec* rec);
// what decode_pages accepts from the device: the parameters asked for, the page's size, and an `inverted` that follows from polarity and sum
bool ink_rec_valid(const InkRec& r, int radius, int drop, int polarity, int h, int w, std::string* why = nullptr);
// tables_from_page and deskew_from_page behind a ready bitmap (tables_ink's layout): the one body of each rule
int tables_from_bits(const uint64_t* bits, int h, int w, int min_len, int32_t* side, int32_t* runs = nullptr);
void deskew_from_bits(const uint64_t* bits, const uint8_t* image, int h, int w, int stride, int max_slope, int gain, uint8_t* out, int out_stride, DeskewRec* rec, uint64_t* scores);

// Selection marks (ttr_engine_set_marks; DESIGN.md "Selection marks").  Checkboxes are found on the ink bitmap as small square frames, their state read from the
// ink inside, every item given its mark and every mark its label.  Every step lives in marks_rule.h, shared with mark_cand_kernel and mark_page_kernel
// (marks.hip); the side block's layout (kMarkSideInts int32) is described there.  min_side 8..64, max_side min_side..128, fill 1..255, ink 1..255.
// bitsT [w][ceil(h / 64)] from bits [h][ceil(w / 64)]: the same bits along y
void marks_transpose(const uint64_t* bits, int h, int w, uint64_t* bitsT);
// steps 2 - 6 behind ready bitmaps: side receives the block (labels -1), counts (may be null) [ceil(h / 32)][2] the kept candidates and corners of every band of
// 32 rows.  Returns the mode: 1, or -6 for a page of more than 512 marks (the block then holds the header alone).
int marks_from_bits(const uint64_t* bits, const uint64_t* bitsT, int h, int w, int min_side, int max_side, int fill, int32_t* side, int32_t* counts = nullptr);
// step 7: item_mark [n] from the centres [n][2] (tables_word_centre), and every mark's label into the block
void marks_items(int32_t* side, const int32_t* centres, int n, int32_t* item_mark);
// 1 - 6 on one page under either ink rule
int marks_from_page(const uint8_t* image, int h, int w, int stride, int min_side, int max_side, int fill, const InkRule& rule, int32_t* side, int32_t* counts = nullptr);
// what decode_pages accepts from the device: a legal mode, a count within the cap, boxes inside the h x w page with x0 <= x1 and y0 <= y1, interiors inside their
// boxes, inked <= area = the interior's pixel count, state the rule's on inked / area / fill, labels in -1..items - 1, marks in (y, x) order.  why (may be null)
// receives the reason.
bool marks_side_valid(const int32_t* side, int h, int w, int fill, int items, std::string* why = nullptr);

// Barcodes (ttr_engine_set_barcodes; DESIGN.md "Barcodes").  Code 128 and Code 39 are read off single lines of the ink bitmaps in all four directions, and the
// lines' hits chained into barcodes.  Every step lives in barcodes_rule.h, shared with barcode_scan_kernel and barcode_page_kernel (barcodes.hip); the side
// block's layout (kBcSideInts int32) and the hits' are described there.  min_lines 4..256, ink 1..255, symbologies 1..3.
// steps 2 - 8 behind ready bitmaps: side receives the block; hits (may be null) [(h + w) 2 8][20] the lines' hit slots and cnt (may be null) [(h + w) 2][4]
// their counters, rows first, as the scan kernel leaves them.  Returns the mode: 1, or -7 for a page of more than 64 barcodes (the block then holds the header alone).
int barcodes_from_bits(const uint64_t* bits, const uint64_t* bitsT, int h, int w, int min_lines, int symbologies, int32_t* side, int32_t* hits = nullptr, int32_t* cnt = nullptr);
// step 9: item_barcode [n] from the centres [n][2] (tables_word_centre)
void barcodes_items(const int32_t* side, const int32_t* centres, int n, int32_t* item_barcode);
// 1 - 8 on one page under either ink rule
int barcodes_from_page(const uint8_t* image, int h, int w, int stride, int min_lines, const InkRule& rule, int symbologies, int32_t* side, int32_t* hits = nullptr,
                       int32_t* cnt = nullptr);
// what decode_pages accepts from the device: a legal mode, a count within the cap, boxes inside the h x w page, (y0, x0, dir) order, symbology 1 or 2 and one
// that was asked for, dir 0..3, lines >= min_lines, flags within the mask, len <= 48 and zero bytes beyond it, counters that are not negative.  why (may be
// null) receives the reason.
bool barcodes_side_valid(const int32_t* side, int h, int w, int min_lines, int symbologies, std::string* why = nullptr);

// One CCL candidate as the GPU reports it (post_ops.hip): stats of the combined-map
// component and the per-row x extremes of its link-masked pixels.
struct Component {
  int root, area, x0, y0, x1, y1;       // bbox inclusive
  const int* rows;                      // [(y1-y0+1)][2] = {min x, max x}; {INT_MAX,-1} for an empty row
};
// tuatara.cpp:162-179 on the row extremes: niter (integer arithmetic), ROI, rectangular
// dilation with OpenCV's anchor, findNonZero + minAreaRect.  Returns false if nothing is left.
bool component_to_rect(const Component& c, int H, int W, RRect* out);

// resize_aspect_ratio's integer/float bookkeeping (tuatara.cpp:206-234)
struct CanvasGeom { int target_h, target_w, h32, w32; float ratio; };
CanvasGeom canvas_geometry(int height, int width, int square_size, float mag_ratio);

// Tiled pages (ttr_engine_set_tiled; DESIGN.md "Tiled pages"): a page larger than the detector canvas is read at full size as overlapping tiles that share one
// canvas; their heat maps are stitched into one page map.  Integers only.  With S = canvas_size, O = overlap, c32(x) = x rounded up to a multiple of 32, one
// axis of length L: L <= S gives one tile at 0 on a canvas of c32(L); otherwise D = S - O, n = ceil((L - S) / D) + 1, origins k D for k < n - 1, the last one
// c32(L - S), canvas S.  tile_plan throws std::runtime_error naming the condition and the figure: S % 32, O % 32 or O outside [64, S / 4], mag_ratio != 1,
// a side above 8192, more than 16 tiles on an axis or 64 on the page.
TilePlan tile_plan(int h, int w, int canvas_size, int overlap, float mag_ratio);
// a plan from given origins (the stage calls): every condition the stitch relies on is checked - at most 16 origins per axis, multiples of 32, ascending, an
// overlap of at least 32 between neighbours, feather bands that do not touch, the last tile ending at the map's end.  Throws naming the axis and the figure.
TilePlan tile_plan_from_origins(int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2);
// the stitch on the host: tiles f32 [pages][ny nx][Hc / 2][Wc / 2][2] -> out f32 [pages][H2][W2][2].  Outside the bands a copy, bit for bit; inside
// lerp(a, b, t) = a + t (b - a), x first, then y, every operation rounded on its own (no FMA) - what tile_stitch_kernel computes (tiles.hip)
void stitch_tiles(const float* tiles, int pages, const TilePlan& plan, float* out);

// Tokenizer (tuatara.cpp:25-117) with the reference's id table quirks.
struct Tokenizer {
  std::string itos;          // 98 entries
  int eos_id, bos_id, pad_id;  // 88, 96, 97
  Tokenizer();
  // argmax ids of one row -> filter(eos_id) -> ids2tok -> cut at first EOS char (tuatara.cpp:108-116, :93-99, :497-502)
  std::string decode(const int* ids, int n) const;
};

// The class mask of a character set (DESIGN.md "Character sets"): bit c & 31 of mask[c >> 5] = logit class c may be chosen.  Bit 0 (EOS) is always set; for
// 1 <= i <= 94 bit i is set iff Tokenizer::itos[i] occurs in allow (null or empty: every character) and not in deny (null or empty: none).  Through the
// table's quirks: a backslash sets ids 69 and 87, ']' sets id 88 (which decodes to nothing).  Throws std::runtime_error, naming the character, when
// allow or deny holds one that names no class in 1..94 ('~', a blank, any non-ASCII byte), or when only EOS is left.  Returns the character classes set.
int charset_mask(const Tokenizer& tok, const char* allow, const char* deny, uint32_t mask[3]);

// The confidence rule (DESIGN.md "Recognition confidence") on the host, for any ids: the characters of decode(ids) are the positions before the
// first id 0 (the EOS) whose id is not 88 and lies in [0, 98); char_conf (n entries suffice) receives their probs in position order, *conf the fp32
// product from 1.0f of those probs, in order, times probs[EOS] when there is an EOS.  decode_conf_kernel forms the same product.  Returns the
// number of characters (= decode(ids, n).size()).
int confidence_from_probs(const int* ids, const float* probs, int n, float* char_conf, float* conf);

// N-best readings of one word from its alternatives (DESIGN.md "Character alternatives"; host only, exact): alt_ids / alt_prob [26][k].  S = the positions
// before the first position whose slot-0 id is 0 (the EOS) whose slot-0 id is a character (in [1, 95), not 88): the confidence rule's S.  The options of a
// position of S are its slots whose id is a character, ranked by (alt_prob descending, slot ascending).  A reading picks one option per position of S: its text
// is the picked characters in position order, its score the fp32 product, in position order from 1.0f, of the picked probabilities, times the EOS position's
// slot-0 probability when there is an EOS - so the all-first reading is the item's (text, conf) bit for bit.  Returns the m best (fewer when fewer exist) by
// (score descending, rank tuple ascending lexicographically), found by a best-first walk over "raise one position's rank by one": lowering one factor never
// raises an fp32 product, and a tuple's parents sort before it, so the walk is exact; it pushes at most m |S| tuples.
struct Reading { std::string text; float score; };
std::vector<Reading> nbest_from_alts(const Tokenizer& tok, const int32_t* alt_ids, const float* alt_prob, int k, int m);

// The device records of a word list (DESIGN.md "Lexicon matching"; host only): records receives n records of 32 bytes - byte 0 the word's length L (1..25),
// bytes 1..L its classes, the rest zero (so the byte behind the last class reads as the EOS, class 0).  Every byte of a word must name exactly one class in
// [1, 95) other than 88: Tokenizer::itos as charset_mask reads it, without ']' (ids 0 and 88) and without the backslash, which the table lists twice (ids 69 and
// 87) - a lexicon entry has to say which position class it means, and a backslash cannot.  Throws std::runtime_error naming the first offending word's index
// for an empty or null word, a word over 25 bytes, and a byte that names no such class; n must lie in 1..2^20.
constexpr int kLexMaxWords = 1 << 20, kLexMaxLen = 25, kLexRecord = 32;
void lexicon_encode(const Tokenizer& tok, const char* const* words, int n, uint8_t* records);

// Fuzzy alignment of lexicon entries (DESIGN.md "Lexicon matching", Fuzzy alignment; host only): the rule of lexicon_fuzzy.hip for n records against one
// table lp f32 [26][96] (a crop's, as the scorers form it).  A cell D[j][p] - j characters of the entry and p positions of the reading consumed - exists for
// 0 <= j <= L, 0 <= p <= 25, |j - p| <= band, and holds a pair (score fp32, edits int): D[0][0] = (0.0f, 0), every other cell starts at (-inf, 0); a candidate
// replaces a cell's value iff its score is greater, or equal with fewer edits (a NaN is never taken up).  Candidates of D[j][p], each only from a cell that
// exists: match (D[j-1][p-1].score + lp[p-1][w[j-1]], edits), extra character in the reading (D[j][p-1].score + gap, edits + 1), dropped character
// (D[j-1][p].score + gap, edits + 1).  The end: over the cells D[L][p] that exist, (D[L][p].score + lp[p][0], edits) under the same rule from (-inf, 0): the
// winner is logp[i] / edits[i].  Every operation is one fp32 addition or comparison.  Returns 0, -1 for a null argument, a band outside 0..3, a gap that is
// not finite or is > 0, or a record whose length byte is outside 1..25 (nothing is written then).
constexpr int kLexMaxBand = 3;
int lexicon_fuzzy_from_lp(const float* lp, const uint8_t* records, int n, int band, float gap, float* logp, int32_t* edits);

}  // namespace ttr
