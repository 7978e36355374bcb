/* C ABI of the MI355X-native tuatara engine (libtuatara_hip.so).
 *
 * This is the drop-in boundary for the reference's one hot path,
 *   std::vector<OutputItem> image_to_data(cv::Mat, std::string, std::string)
 *   (/root/reference/tuatara.h:8-13, implemented at tuatara.cpp:314-512),
 * exported as plain C so any host language can bind it (INTEGRATION.md shows the
 * C++ shim that keeps tuatara.h's signature and the pybind11 module `pytuatara`
 * of bindings/python.cpp:43-58).  No exceptions cross this boundary: every call
 * returns 0 on success or a negative code and ttr_last_error() holds the message.
 * Inputs are borrowed for the duration of the call; results are engine-allocated
 * and released with ttr_result_free.
 */
#ifndef TUATARA_HIP_H
#define TUATARA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ttr_engine ttr_engine;
typedef struct ttr_result ttr_result;

/* TTR_PREC_F16X4: fp32-equivalent results on the f16 matrix cores - every fp32 activation as three f16 planes, every weight as an
   f16 pair, four MFMAs per product into one fp32 accumulator (tuatara_amd/csrc/split.h).  The reference computes in fp32
   (tuatara.cpp:363-376, :443-446, :307); this mode meets its outputs at the level of fp32 rounding noise and is the default.
   TTR_PREC_BF16: operands rounded to bf16 (fastest; logits differ by up to ~1e-1).  TTR_PREC_F32: fp32 MFMA throughout. */
enum { TTR_PREC_BF16 = 0, TTR_PREC_F32 = 1, TTR_PREC_F16X4 = 2 };
/* ttr_config.crop_mode.  TTR_CROP_BOUNDING: the recogniser sees the axis-aligned boundingRect of each word's rotated rectangle, resized to
   32 x 128 - the reference's crop (tuatara.cpp:408-418, :440), bit for bit; the default.  TTR_CROP_RECTIFIED: a word whose rectangle is
   tilted is sampled on its own quadrilateral, deskewed by up to 45 degrees (DESIGN.md "Rectified crops"); axis-aligned words keep the
   reference's crop.  The items, their order and their bboxes are the same in both modes; only text / ids may change.  Text rotated by more
   than 45 degrees, or upside down, is recovered only by word orientation (ttr_config.orient below; geometry alone cannot tell 90 from
   270 degrees, or 0 from 180). */
enum { TTR_CROP_BOUNDING = 0, TTR_CROP_RECTIFIED = 1 };
/* ttr_config.orient (DESIGN.md "Word orientation").  TTR_ORIENT_OFF: the default; the same kernels and bits as without the field.
   TTR_ORIENT_FLIP: every word is also read turned by 180 degrees; TTR_ORIENT_QUARTER: by 90, 180 and 270 degrees.  A turn t is the number
   of quarter turns clockwise by which the word lies on the page relative to upright.  Each word keeps the reading the recogniser is most sure
   of (the largest conf; ties to the lower turn).  The items, their order, bbox and quad are those of orient = 0; only text, ids, prob and conf
   may change.  ttr_config.orient_page = 1 decides once per page (a vote of the words) and reports every word at the page's turn. */
enum { TTR_ORIENT_OFF = 0, TTR_ORIENT_FLIP = 1, TTR_ORIENT_QUARTER = 2 };
enum { TTR_ORDER_AS_IS = 0 };  /* channel order: the engine reproduces "swap, detect; swap back, recognise"
                                  (tuatara.cpp:349, :441) relative to whatever the caller passes */

/* The constants the reference hard-codes (tuatara.cpp:352-353, :397-399, :148). */
typedef struct ttr_config {
  int precision;         /* TTR_PREC_F16X4 (default), TTR_PREC_BF16 or TTR_PREC_F32 */
  int device;            /* HIP device ordinal */
  int canvas_size;       /* 1024   tuatara.cpp:352 */
  float mag_ratio;       /* 1.0    tuatara.cpp:353 */
  float text_threshold;  /* 0.7    tuatara.cpp:397 */
  float link_threshold;  /* 0.4    tuatara.cpp:398 */
  float low_text;        /* 0.4    tuatara.cpp:399 */
  int min_area;          /* 10     tuatara.cpp:148 */
  int strict_crops;      /* 0: clamp crops to the image; 1: fail like the reference's cv::Exception at :416 */
  int max_components;    /* capacity for CCL candidates per page (default 4096) */
  int verbose;           /* 1: the reference's progress lines on stdout (tuatara.cpp:328-329, :342, :386, :421, :434, :488, :509); TUATARA_VERBOSE=1 does the same */
  int crop_mode;         /* TTR_CROP_BOUNDING (default) or TTR_CROP_RECTIFIED (appended last: the fields above keep their offsets) */
  int orient;            /* TTR_ORIENT_OFF (default), TTR_ORIENT_FLIP or TTR_ORIENT_QUARTER; other values make ttr_create fail */
  int orient_page;       /* 0 (default): the turn is chosen per word; 1: once per page */
  int lines;             /* 0 (default): off, the same kernels and bits as without the field; 1: the words are also grouped into text lines in
                            reading order (DESIGN.md "Text lines"); other values make ttr_create fail.  Needs max_components <= 4096 */
  int chars;             /* 0 (default): off, the same kernels and bits as without the field; 1: every item also carries one quadrilateral and one bbox per
                            character of its text (DESIGN.md "Character boxes"); other values make ttr_create fail */
  int blocks;            /* 0 (default): off, the same kernels and bits as without the field; 1: the text lines are also grouped into blocks (paragraphs,
                            column pieces) in reading order (DESIGN.md "Text blocks"); other values make ttr_create fail.  Needs lines = 1 */
  int mixed_batches;     /* 0 (default): ttr_images_to_data batches images of equal size, as without the field; 1: it batches images that share one
                            detector canvas, whatever their sizes (DESIGN.md "Mixed-size batches"); other values make ttr_create fail.  Every result is
                            the same either way; only the batching changes */
} ttr_config;

void ttr_config_default(ttr_config* cfg);

/* weights_dir holds craft.ttrw + parseq.ttrw (tools/convert_weights.py makes them from the
 * reference's craft_traced_torchscript_model.pt / parseq_torchscript.bin, tuatara.cpp:333,:423). */
ttr_engine* ttr_create(const char* weights_dir, const ttr_config* cfg);
void ttr_destroy(ttr_engine* e);
const char* ttr_last_error(void);
const char* ttr_version(void);

/* ---- the hot path: replaces image_to_data (tuatara.cpp:314-512) ---------------------------- */
/* Host image, u8 HWC 3 channels, row_stride in bytes.  Not modified (the reference swaps
 * the caller's channels in place at :349; callers never rely on that). */
int ttr_image_to_data(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, ttr_result** out);
/* Batch of n same-sized pages already resident in device memory (contiguous [n][h][w][3] u8).
 * out[i] receives page i's result. */
int ttr_pages_to_data_dev(ttr_engine* e, const uint8_t* d_pages, int n, int h, int w, ttr_result** out);
/* Streamed form of ttr_pages_to_data_dev for a sequence of batches (same contract per batch, results two calls later):
 * ttr_stream_push(j) enqueues the detector of batch j, then the recogniser of batch j-1, turns batch j's components into boxes on the
 * host while the GPU works, and returns batch j-2's results in out_prev[0 .. *n_prev) (*n_prev = 0 on the first two pushes).  The
 * GPU always has a whole detector or recogniser pass queued while the host decodes, returns and comes back with the next batch.  Two
 * streams by default (tuning key "recog_overlap"): batch j-1's recogniser runs on a stream of its own beside batch j's detector (they
 * share no buffer); results are identical to the synchronous call's.  The pages of a batch must stay valid until its results have been returned.
 * ttr_stream_flush returns the oldest batch still in flight (*n_prev = 0: none left; call it until then).  out_prev must hold as many
 * entries as the largest batch.  The synchronous calls refuse to run while streamed batches are in flight. */
int ttr_stream_push(ttr_engine* e, const uint8_t* d_pages, int n, int h, int w, ttr_result** out_prev, int* n_prev);
int ttr_stream_flush(ttr_engine* e, ttr_result** out_prev, int* n_prev);
/* image_to_data over a LIST of host images of any sizes (u8 HWC, 3 channels each; hs[i] x ws[i]; row_strides in bytes, NULL = tightly packed):
 * what a caller of the reference writes as a loop over image_to_data (/root/reference/bindings/run_ocr.py:92, examples/resume.cpp:11), with the models
 * loaded once (the reference reloads both per call, tuatara.cpp:336, :428).  Images of equal size travel together as batches through the streamed path
 * above; their rows are gathered into pinned staging buffers and copied to the device on an upload stream of their own while the previous batch is on the
 * GPU.  out[i] receives image i's result - input order, whatever the batching.  Every result equals what ttr_image_to_data returns for that image.
 * Returns 0; -1 when the call itself could not run (out[] untouched); k > 0 when k images failed - an unreadable entry (NULL, empty, a stride shorter than
 * a row: the reference's "Error reading image from file", tuatara.cpp:344-347) or the images of a batch that failed on the GPU: those keep EMPTY results, every
 * other out[i] is delivered, and ttr_last_error() lists the failed indices with the first failure's message - what a loop over image_to_data gives. */
int ttr_images_to_data(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n, ttr_result** out);

/* Mixed-size batches (DESIGN.md "Mixed-size batches").  The detector never sees a page's size, only its canvas: H x W = the page scaled by `ratio`
 * (so that its longer side is at most canvas_size), each side rounded up to a multiple of 32.  Pages of different sizes and row strides that share
 * one canvas can therefore travel as one batch.  A ttr_page is one such page in device memory; with a row stride it can be a window of a larger
 * device image.
 * ttr_canvas_geometry: host only, no GPU work - the canvas and ratio the engine gives an h x w page (e = NULL: an engine of the default config).
 * Returns 0; -1 for h <= 0, w <= 0 or a page too thin to resize (ttr_last_error).
 * ttr_pages_to_data_dev_v / ttr_stream_push_v: ttr_pages_to_data_dev / ttr_stream_push for n such pages; every result equals the page's own
 * single call.  A batch whose pages do not share one canvas is refused before anything is enqueued (the message names the first offending page and
 * both canvases); a page with h <= 0, w <= 0, a row stride shorter than 3 w or too thin to resize fails the call.  Streamed batches of both kinds
 * mix freely and are returned by the same ttr_stream_flush; the pages must stay valid until their batch's results have been returned.  With a
 * communicator attached they are collectives like their twins.
 * ttr_images_to_data with ttr_config.mixed_batches = 1 batches by canvas instead of by size: same results, fewer and larger batches for lists
 * of many sizes.  ttr_last_images_batches: the pages per batch of the last ttr_images_to_data call, in run order (at most cap entries are
 * written); returns their number. */
typedef struct ttr_page { const uint8_t* data; int h, w; int row_stride; } ttr_page;   /* device memory, u8 HWC 3 channels; row_stride in bytes, 0 = 3 * w */
int ttr_canvas_geometry(const ttr_engine* e, int h, int w, int* H, int* W, float* ratio);
int ttr_pages_to_data_dev_v(ttr_engine* e, const ttr_page* pages, int n, ttr_result** out);
int ttr_stream_push_v(ttr_engine* e, const ttr_page* pages, int n, ttr_result** out_prev, int* n_prev);
int ttr_last_images_batches(ttr_engine* e, int32_t* pages_per_batch, int cap);

int ttr_result_count(const ttr_result* r);
const char* ttr_result_text(const ttr_result* r, int i);
const float* ttr_result_bbox(const ttr_result* r, int i);   /* {x1,y1,x2,y2}, tuatara.cpp:272 */
const int32_t* ttr_result_ids(const ttr_result* r, int i);  /* 26 argmax token ids of crop i */
/* the word's quadrilateral {tl.x, tl.y, tr.x, tr.y, br.x, br.y, bl.x, bl.y} in image pixels, unrounded: tl -> tr is the baseline (the side
 * of the rotated rectangle nearest horizontal, skew in [-45, 45] degrees, pointing right), tl -> bl points down.  Filled in every crop
 * mode; ttr_result_quads is the bulk view [count][8] (NULL when the result is empty). */
const float* ttr_result_quad(const ttr_result* r, int i);
const float* ttr_result_quads(const ttr_result* r);
/* Recognition confidence (DESIGN.md "Recognition confidence"), every crop mode and entry point; a probability in (0, 1], never 0-100.
 * ttr_result_prob: 26 floats parallel to ttr_result_ids - prob[p] = 1 / sum_c exp(x[c] - x[id[p]]), the softmax value of the argmax id
 * over the refined logits x of position p (the reference's Tokenizer::max_dist, tuatara.cpp:101-106, which it computes and discards).
 * ttr_result_conf: the word's confidence - the fp32 product, in position order from 1.0f, of prob over the positions that make up the
 * text (before the first EOS, id 0, and not id 88), times prob[EOS] when the row has an EOS (upstream PARSeq's convention).  Bulk views:
 * ttr_result_confs [count], ttr_result_probs_all [count][26] (NULL when the result is empty). */
float ttr_result_conf(const ttr_result* r, int i);
const float* ttr_result_prob(const ttr_result* r, int i);
const float* ttr_result_confs(const ttr_result* r);
const float* ttr_result_probs_all(const ttr_result* r);
void ttr_result_free(ttr_result* r);
/* bulk views for bindings (valid until ttr_result_free): all boxes [count][4], all ids [count][26]; the texts of all
 * items, each followed by '\n' (no token maps to '\n'), copied into buf when cap suffices; returns the bytes needed. */
const float* ttr_result_bboxes(const ttr_result* r);
const int32_t* ttr_result_ids_all(const ttr_result* r);
int ttr_result_texts(const ttr_result* r, char* buf, size_t cap);
/* the same for a batch of results in one call (any output may be NULL): counts[n], bboxes[total][4], ids[total][26], texts as
 * above ('\n' after each item, copied when texts_cap >= *texts_need).  Returns the total item count. */
int ttr_results_gather(ttr_result* const* rs, int n, int32_t* counts, float* bboxes, int32_t* ids, char* texts, size_t texts_cap,
                       size_t* texts_need);
/* ... and their confidences (either output may be NULL): conf[total], probs[total][26], in ttr_results_gather's item order.  Returns the total. */
int ttr_results_gather_conf(ttr_result* const* rs, int n, float* conf, float* probs);
/* The confidence rule on the host, no GPU: ids / probs of n_pos positions -> char_conf[*n_chars] (prob of each character of
 * ttr_decode_ids(ids), in order; n_pos entries always suffice) and *conf (the product above; bit-equal to ttr_result_conf given the same
 * probs).  Takes any ids: ids outside [0, 98) are dropped as ttr_decode_ids drops them.  Outputs may be NULL.  Returns *n_chars, -1 on bad arguments. */
int ttr_confidence_from_probs(const int32_t* ids, const float* probs, int n_pos, float* char_conf, int* n_chars, float* conf);

/* Word orientation (DESIGN.md "Word orientation"), every entry point but ttr_pages_to_data_dev_sharded (which refuses orient != 0).
 * ttr_result_orient: the chosen turn of item i, 0..3 (quarter turns clockwise; 0 when orient is off); ttr_result_orients: [count] (NULL
 * when orient is off or the result is empty).  ttr_result_orient_candidates: K, the candidate turns per word (1 when off, 2 with
 * TTR_ORIENT_FLIP - turns {0, 2} -, 4 with TTR_ORIENT_QUARTER).  ttr_result_orient_confs: [count][K] the conf of every candidate reading, in
 * ascending turn order (column 0 is the orient = 0 conf; when off, the same as ttr_result_confs).  ttr_result_page_orient: the page's turn
 * (the vote; 0 when off), reported in both orient_page modes. */
int ttr_result_orient(const ttr_result* r, int i);
const int32_t* ttr_result_orients(const ttr_result* r);
int ttr_result_orient_candidates(const ttr_result* r);
const float* ttr_result_orient_confs(const ttr_result* r);
int ttr_result_page_orient(const ttr_result* r);
/* ... for a batch of results in one call (any output may be NULL): turns[total], cand_conf[total][K] (K of the results' engine),
 * page_turns[n], in ttr_results_gather's item order.  Returns the total item count, -1 when the results differ in K. */
int ttr_results_gather_orient(ttr_result* const* rs, int n, int32_t* turns, float* cand_conf, int32_t* page_turns);
/* The choice on the host, no GPU: the n words of ONE page, conf[n][k] and ids[n][k][26] of their k candidate readings in ascending turn
 * order (k = 1: turn {0}; 2: turns {0, 2}; 4: turns {0, 1, 2, 3}) -> turns[n] and *page_turn, as turns 0..3.  Per word: the largest conf,
 * strict > in ascending turn order.  Page: the argmax of the votes of the words whose winning text has at least 2 characters, ties to the
 * lower turn, 0 without votes; per_page = 1: every turns[i] = *page_turn.  Returns 0, -1 on bad arguments. */
int ttr_orient_select(const float* conf, const int32_t* ids, int n, int k, int per_page, int32_t* turns, int32_t* page_turn);

/* Text lines (ttr_config.lines = 1; DESIGN.md "Text lines"), every entry point but ttr_pages_to_data_dev_sharded (which refuses lines != 0).
 * The items, their order and every other output are those of lines = 0; the result also says which line of its page each item belongs to and
 * which word of that line it is, and gives the page's lines in reading order.  Lines depend only on the page's own quads (ttr_result_quads).
 * ttr_result_line_count: the page's lines.  ttr_result_lines / ttr_result_words: [count] each item's line (in line order) and its position
 * inside that line.  ttr_result_reading_order: [count] the item indices in reading order, each line's members consecutive.
 * ttr_result_line_first: [lines + 1] the lines' offsets into the reading order.  ttr_result_line_bboxes: [lines][4] min / max of the members'
 * bbox.  With lines = 0, or for an empty result, the pointers are NULL and the count is 0. */
int ttr_result_line_count(const ttr_result* r);
const int32_t* ttr_result_lines(const ttr_result* r);
const int32_t* ttr_result_words(const ttr_result* r);
const int32_t* ttr_result_reading_order(const ttr_result* r);
const int32_t* ttr_result_line_first(const ttr_result* r);
const float* ttr_result_line_bboxes(const ttr_result* r);
/* The text of line l (its members' text in word order, joined by one space) and of the page (its lines joined by '\n'), without a
 * terminator.  Both return the bytes needed, like ttr_result_texts: buf is written only when cap suffices.  0 with lines = 0. */
int ttr_result_line_text(const ttr_result* r, int l, char* buf, size_t cap);
int ttr_result_page_text(const ttr_result* r, char* buf, size_t cap);
/* ... for a batch of results in one call (any output may be NULL): n_lines[n]; line, word and order [total] in ttr_results_gather's item
 * order (order holds indices local to its result); line_first: per result its n_lines + 1 offsets (local), result after result - total
 * lines + n entries, at most total + n; line_bboxes [total lines][4].  A result without lines (lines = 0, or empty) contributes 0 lines, its
 * single line_first entry 0, and -1 for line / word / order of any items it has.  Returns the total line count, -1 on bad arguments. */
int ttr_results_gather_lines(ttr_result* const* rs, int n, int32_t* n_lines, int32_t* line, int32_t* word, int32_t* order, int32_t* line_first,
                             float* line_bboxes);
/* The rule on the host, no GPU: the n words of ONE page as quads [n][8] (tl, tr, br, bl in image pixels, as ttr_result_quad gives them) ->
 * line[n], word[n], *n_lines.  Integer arithmetic on llrint(16 x): exact, the same as line_group_kernel's.  Returns 0; -1 on bad arguments, a
 * coordinate that is not finite or one with |x| >= 32768. */
int ttr_lines_from_quads(const float* quads, int n, int32_t* line, int32_t* word, int32_t* n_lines);
/* The rule on the GPU as a stage entry point, whatever the engine's `lines`: host quads of several pages - page p owns quads
 * [first[p], first[p + 1]), first[0] = 0, at most 4096 per page - are uploaded, line_group_kernel runs once, and line[first[pages]],
 * word[first[pages]] and n_lines[pages] come back.  Returns 0, -1 on error (ttr_last_error). */
int ttr_group_lines(ttr_engine* e, const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines);

/* Character boxes (ttr_config.chars = 1; DESIGN.md "Character boxes"), every entry point but ttr_pages_to_data_dev_sharded (which refuses chars != 0).
 * The items, their order and every other output are those of chars = 0; every item also carries one quadrilateral and one bbox per character of its
 * text, in text order, cut from the detector's region map along the word's baseline (of the turned quad when orientation is on).
 * ttr_result_char_count: the characters of item i (= strlen of its text).  ttr_result_char_first: [count + 1] offsets of the items' characters.
 * ttr_result_char_quads: [total][8] tl, tr, br, bl in image pixels.  ttr_result_char_bboxes: [total][4] min x, min y, max x, max y of those corners.
 * ttr_result_char_cuts: [count][27] the cuts b[0..K] along the baseline in 1/256 of the 128 profile columns (0..32768), -1 beyond K.
 * ttr_result_char_modes: [count] 0 = even split of the inked extent (no ink, or fewer than two columns per character), 1 = valley cuts.
 * ttr_result_char_profiles: [count][128] the word's profile.  With chars = 0, or for an empty result, the pointers are NULL and the count is 0. */
int ttr_result_char_count(const ttr_result* r, int i);
const int32_t* ttr_result_char_first(const ttr_result* r);
const float* ttr_result_char_quads(const ttr_result* r);
const float* ttr_result_char_bboxes(const ttr_result* r);
const int32_t* ttr_result_char_cuts(const ttr_result* r);
const int32_t* ttr_result_char_modes(const ttr_result* r);
const uint8_t* ttr_result_char_profiles(const ttr_result* r);
/* ... for a batch of results in one call (any output may be NULL): char_first: per result its count + 1 offsets (local to the result), result
 * after result - total items + n entries; char_quads [total characters][8], char_bboxes [..][4]; cuts [total items][27], modes [total items],
 * profiles [total items][128] in ttr_results_gather's item order.  A result without characters (chars = 0, or empty) contributes zeros to
 * char_first, -1 cuts, 0 modes and profiles.  Returns the total character count, -1 on bad arguments. */
int ttr_results_gather_chars(ttr_result* const* rs, int n, int32_t* char_first, float* char_quads, float* char_bboxes, int32_t* cuts, int32_t* modes,
                             uint8_t* profiles);
/* The rule on the host, no GPU.  ttr_char_cuts_from_profile: one profile q128, K in 0..26 and qlow = (int)(low_text * 255.f) -> cuts27, *mode.
 * ttr_chars_from_map: n words on ONE region plane tnorm [H2][W2] (f32, normalised) of a page whose canvas ratio is `ratio`; quads [n][8] as
 * ttr_result_quad gives them, turns [n] in 0..3, nchars [n] in 0..26 -> cuts [n][27], modes [n], profiles [n][128].
 * ttr_char_quads_from_cuts: one word's quad, turn and cuts -> quads_out [K][8], bboxes_out [K][4].  Each returns 0; -1 on bad arguments, a
 * coordinate that is not finite or has |x| >= 32768, or a ratio outside (0, 2048]. */
int ttr_char_cuts_from_profile(const uint8_t* q128, int K, int qlow, int32_t* cuts27, int32_t* mode);
int ttr_chars_from_map(const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars, int n,
                       int32_t* cuts, int32_t* modes, uint8_t* profiles);
int ttr_char_quads_from_cuts(const float* quad, int turn, const int32_t* cuts27, int K, float* quads_out, float* bboxes_out);
/* The rule on the GPU as a stage entry point, whatever the engine's `chars`: the same arguments as ttr_chars_from_map, the map and the words are
 * uploaded and char_cut_kernel runs once.  Refuses while batches stream.  Returns 0, -1 on error (ttr_last_error). */
int ttr_char_cuts(ttr_engine* e, const float* tnorm, int H2, int W2, float ratio, float low_text, const float* quads, const int32_t* turns, const int32_t* nchars,
                  int n, int32_t* cuts, int32_t* modes, uint8_t* profiles);

/* Text blocks (ttr_config.blocks = 1 with lines = 1; DESIGN.md "Text blocks"), every entry point but ttr_pages_to_data_dev_sharded (which refuses
 * blocks != 0).  Every other output is that of blocks = 0; the result also groups the page's text lines into blocks and gives the blocks in reading
 * order: a column is read to its end before the next begins.  Blocks depend only on the page's own quads (ttr_result_quads).
 * ttr_result_block_count: the page's blocks.  ttr_result_block_mode: 1 when the blocks were ordered by the precedence relation, 0 when the page has
 * more than 512 blocks and they are ordered by their top-left corners alone.  ttr_result_line_blocks / ttr_result_line_pos: [lines] each line's
 * block (in block order) and its position inside that block.  ttr_result_blocks: [count] each item's block.  ttr_result_block_order: [lines] the
 * line indices in block reading order, each block's lines consecutive.  ttr_result_block_first: [blocks + 1] the blocks' offsets into it.
 * ttr_result_block_bboxes: [blocks][4] min / max of the member lines' bboxes.  With blocks = 0, or for an empty result, the pointers are NULL, the
 * counts are 0 and ttr_result_block_mode is 0 (the stage calls ttr_blocks_from_quads / ttr_group_blocks report mode 1 for an empty page, as the
 * rule states it). */
int ttr_result_block_count(const ttr_result* r);
int ttr_result_block_mode(const ttr_result* r);
const int32_t* ttr_result_line_blocks(const ttr_result* r);
const int32_t* ttr_result_line_pos(const ttr_result* r);
const int32_t* ttr_result_blocks(const ttr_result* r);
const int32_t* ttr_result_block_order(const ttr_result* r);
const int32_t* ttr_result_block_first(const ttr_result* r);
const float* ttr_result_block_bboxes(const ttr_result* r);
/* The text of block b (its lines in order, joined by '\n') and of the page read by blocks (the blocks joined by "\n\n"), without a terminator.
 * Both return the bytes needed, like ttr_result_texts: buf is written only when cap suffices.  0 with blocks = 0.  ttr_result_page_text is unchanged. */
int ttr_result_block_text(const ttr_result* r, int b, char* buf, size_t cap);
int ttr_result_page_text_blocks(const ttr_result* r, char* buf, size_t cap);
/* ... for a batch of results in one call (any output may be NULL): n_blocks[n], modes[n]; blocks [total items] in ttr_results_gather's item order;
 * line_blocks, line_pos and block_order [total lines] in ttr_results_gather_lines' line order (block_order holds line indices local to its result);
 * block_first: per result its n_blocks + 1 offsets (local), result after result; block_bboxes [total blocks][4].  A result without blocks
 * (blocks = 0, or empty) contributes 0 blocks, no lines, its single block_first entry 0, and -1 for the blocks of any items it has.  Returns the
 * total block count, -1 on bad arguments. */
int ttr_results_gather_blocks(ttr_result* const* rs, int n, int32_t* n_blocks, int32_t* modes, int32_t* blocks, int32_t* line_blocks, int32_t* line_pos,
                              int32_t* block_order, int32_t* block_first, float* block_bboxes);
/* The rule on the host, no GPU: the n words of ONE page as quads [n][8] -> the line rule's line[n], word[n], *n_lines, then block[n], pos[n] (per
 * line: entries [0, *n_lines), the rest -1), *n_blocks, *mode.  Any output may be NULL.  Integer arithmetic, exact, the same as
 * block_group_kernel's.  Returns 0; -1 for the inputs ttr_lines_from_quads refuses. */
int ttr_blocks_from_quads(const float* quads, int n, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block, int32_t* pos, int32_t* n_blocks,
                          int32_t* mode);
/* The rule on the GPU as a stage entry point, whatever the engine's config: host quads of several pages (as ttr_group_lines) are uploaded,
 * line_group_kernel and block_group_kernel run once each, and line, word, block, pos [first[pages]] (block and pos per line within each page's
 * range, -1 beyond its lines), n_lines, n_blocks and mode [pages] come back.  Any output may be NULL.  Refuses while batches stream.  Returns 0,
 * -1 on error (ttr_last_error). */
int ttr_group_blocks(ttr_engine* e, const float* quads, const int32_t* first, int pages, int32_t* line, int32_t* word, int32_t* n_lines, int32_t* block,
                     int32_t* pos, int32_t* n_blocks, int32_t* mode);

/* ---- multi-GPU: RCCL in the C++ host -----------------------------------------------------------------
 * One process per GPU, one engine per process.  The OCR path has no data-path collective: pages are independent.  The one exchange is
 * the gather of the decoded token ids, and it runs device buffer to device buffer with ncclAllGather (/opt/rocm/include/rccl/rccl.h:678)
 * on the engine's stream: attach a communicator and every batch's ids are gathered behind its recogniser pass.  Records are variable
 * length - every rank's crops-per-page counts travel first, then the payload (the largest rank total rows of 26 ids per rank); nothing
 * is truncated.  There is no torch in this path. */
typedef struct ttr_comm ttr_comm;
#define TTR_COMM_ID_BYTES 256
/* ncclGetUniqueId (x2: a data and a control communicator): call on ONE rank and hand the bytes to the others by any means ... */
int ttr_comm_unique_id(void* id256);
ttr_comm* ttr_comm_create(ttr_engine* e, int rank, int world, const void* id256);
/* ... or let rank 0 listen on addr:port (TCP) and hand them over itself (single node: addr = 127.0.0.1) */
ttr_comm* ttr_comm_create_tcp(ttr_engine* e, int rank, int world, const char* addr, int port);
/* The same communicator over a TCP transport through rank 0 instead of RCCL (device buffers staged through host memory, every collective
 * framed with a sequence number and its size: a mismatched call sequence raises instead of hanging).  For ranks that share ONE GPU - RCCL
 * refuses two ranks on a device -, which is how the multi-rank paths run at world size 2 on a single-GPU box, and as a fallback.
 * Rendezvous (both forms): rank 0 listens on addr:port for TUATARA_COMM_TIMEOUT seconds (default 120). */
ttr_comm* ttr_comm_create_socket(ttr_engine* e, int rank, int world, const char* addr, int port);
const char* ttr_comm_transport(const ttr_comm* c);   /* "rccl" or "socket" */
/* one JSON object about this rank's end of the communicator: {"rank", "world", "transport", "rccl_version" (ncclGetVersion), "device" (HIP ordinal),
 * "pci_bus_id", "gpu" (gcnArchName), "pid"} - what a scaling run prints so that its rank -> GPU map can be read afterwards.  Returns the length. */
int ttr_comm_describe(const ttr_comm* c, char* buf, size_t cap);
void ttr_comm_destroy(ttr_comm* c);
int ttr_comm_rank(const ttr_comm* c);
int ttr_comm_world(const ttr_comm* c);
/* c != NULL: from now on ttr_pages_to_data_dev / ttr_stream_push / ttr_stream_flush all-gather the token ids of every batch (every rank
 * must then make the same sequence of calls with the same page counts: a {status, pages} header travels first, and a rank that failed in
 * its detector or passed another page count makes the call fail on EVERY rank instead of leaving the others in the collective);
 * c == NULL: detach. */
int ttr_engine_attach_comm(ttr_engine* e, ttr_comm* c);
/* The gathered ids of the batch whose results the last such call returned: counts[world][pages] crops per page, ids[sum][26] in
 * (rank, page, crop) order.  Returns the number of id rows (and the sizes through world / pages / ids_need); buffers that are too
 * small or NULL are not written. */
int ttr_last_gathered(ttr_engine* e, int* world, int* pages, int32_t* counts, size_t counts_cap, int32_t* ids, size_t ids_cap, size_t* ids_need);
/* ... and the same rows' confidences, gathered in the same collective as the ids: conf[rows], probs[rows][26] (same order as ids).  Returns
 * the number of rows; buffers that are too small or NULL are not written. */
int ttr_last_gathered_conf(ttr_engine* e, float* conf, size_t conf_cap, float* probs, size_t probs_cap);
/* bytes of every rank concatenated by rank into all[world * bytes] (small host buffers; also the barrier of the benchmark) */
int ttr_comm_allgather_host(ttr_comm* c, const void* mine, size_t bytes, void* all);
/* the framing of a gathered batch, host logic only (no GPU): counts[world][pages] -> cap (payload rows per rank), total[world],
 * first[world * pages + 1] (row of each page's first crop in the compacted array) */
int ttr_gather_layout(const int32_t* counts, int world, int pages, int* cap, int32_t* total, int64_t* first);
/* Latency mode (the reference's 6-thread fan-out over the crop batch, tuatara.cpp:450-485, across GPUs): rank 0 passes the pages, detects
 * and packs the crop batch; it is broadcast, rank r recognises shard r of ceil(N / world) crops, the ids are all-gathered and rank 0
 * receives the pages' results (the other ranks pass d_pages = NULL and get n empty results).  Collective.  Returns the result count. */
int ttr_pages_to_data_dev_sharded(ttr_comm* c, const uint8_t* d_pages, int n, int h, int w, ttr_result** out);

/* ---- stage-level entry points (BASELINE.json configs 2-3; used by the parity tests) -------- */
/* CRAFT forward (tuatara.cpp:363-394): canvas u8 [H][W][3] (H,W multiples of 32, already resized,
 * padded and in the channel order CRAFT must see) -> heat f32 [H/2][W/2][2]. */
int ttr_craft_heatmap(ttr_engine* e, const uint8_t* canvas, int H, int W, float* heat);
/* get_detected_boxes (tuatara.cpp:119-204): heat f32 [H2][W2][2] -> rects {cx,cy,w,h,angle} in heat-map
 * pixels, ordered by component label (raster order of first pixel).  Returns count in *n. */
int ttr_ccl_boxes(ttr_engine* e, const float* heat, int H2, int W2, float* rects5, int max_rects, int* n);
/* resize_aspect_ratio + channel swap (tuatara.cpp:349, :206-234): image -> canvas u8 [*H][*W][3] */
int ttr_resize_canvas(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, uint8_t* canvas, size_t canvas_cap,
                      int* H, int* W, float* ratio);
/* adjust_result_coordinates + boundingRect + crop + cv::resize (tuatara.cpp:406-418, :436-441):
 * rects in heat-map pixels -> crops u8 [n][32][128][3] in the order PARSeq sees; boxes_out (optional)
 * receives the adjusted rects {cx,cy,w,h,angle} in image pixels. */
int ttr_pack_crops(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const float* rects5, int n,
                   float ratio, uint8_t* crops, float* boxes_out);
/* The TTR_CROP_RECTIFIED twin of ttr_pack_crops, whatever the engine's crop_mode: the same rects and clamp, each crop made by the
 * rectified rule (kind 0 = ttr_pack_crops's crop for an axis-aligned rect, kind 1 = the deskewed quadrilateral); quads_out (optional)
 * receives the quads [n][8] as ttr_result_quad gives them.  A rect whose clamped boundingRect is empty yields a zero crop. */
int ttr_pack_crops_rectified(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const float* rects5, int n,
                             float ratio, uint8_t* crops, float* quads_out);
/* The crop of a word read at `turn` (0..3 quarter turns clockwise), whatever the engine's crop_mode and orient: the same rects and clamp
 * as ttr_pack_crops.  Turn 0 is ttr_pack_crops's crop (crop_mode 0) or ttr_pack_crops_rectified's (crop_mode 1) bit for bit.  Turn t >= 1
 * samples the turned quad Q_t[k] = Q[(k + t) mod 4] by the rectified sampler, Q being the deskewed quad (crop_mode 1) or the clamped
 * boundingRect's pixel edges (crop_mode 0).  quads_out (optional) receives Q_t [n][8].  A rect whose clamped boundingRect is empty yields
 * a zero crop. */
int ttr_pack_crops_oriented(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const float* rects5, int n,
                            float ratio, int crop_mode, int turn, uint8_t* crops, float* quads_out);
/* The table kernels of a mixed-size batch as stage entry points (DESIGN.md "Mixed-size batches"); both refuse while batches stream.
 * ttr_resize_canvas_batch: n host images of different sizes that share one canvas (row_strides in bytes, NULL = tightly packed; the pages keep
 * their strides on the device) -> canvases u8 [n][*H][*W][3] and ratios [n], by ONE launch of resize_pad_pages_kernel; canvas i is byte for byte
 * ttr_resize_canvas's of image i.
 * ttr_pack_crops_batch: n rects in heat-map pixels, rect i on page page_of[i] of n_pages such images, each page at its own ratio
 * (ttr_canvas_geometry) -> crops [n][32][128][3] and quads_out (optional) [n][8], by ONE launch of the table packer; crop i is byte for byte
 * ttr_pack_crops_oriented's for the same crop_mode and turn on its page alone. */
int ttr_resize_canvas_batch(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n, uint8_t* canvases,
                            size_t cap, int* H, int* W, float* ratios);
int ttr_pack_crops_batch(ttr_engine* e, const uint8_t* const* images, const int* hs, const int* ws, const int* row_strides, int n_pages,
                         const float* rects5, const int32_t* page_of, int n, int crop_mode, int turn, uint8_t* crops, float* quads_out);
/* PARSeq forward (tuatara.cpp:443-446 + :307): crops u8 [n][32][128][3] -> logits f32 [n][26][95];
 * ar_logits (optional) receives the autoregressive pass's logits - per crop defined up to and including its EOS step (upstream leaves
 * its loop when every crop has emitted EOS; behind a crop's own EOS the bf16 engine skips it, and zero-fills the steps behind the batch's
 * exit) -, ids (optional) the argmax ids [n][26]. */
int ttr_parseq_logits(ttr_engine* e, const uint8_t* crops, int n, float* logits, float* ar_logits, int32_t* ids);
/* The recogniser's final decode on host logits f32 [n][26][95] (uploaded, decode_conf_kernel, downloaded): ids [n][26] as the engine forms
 * them, probs [n][26] and conf [n] as ttr_result_prob / ttr_result_conf give them.  Any output may be NULL. */
int ttr_logits_confidence(ttr_engine* e, const float* logits, int n, int32_t* ids, float* probs, float* conf);
/* Character sets (DESIGN.md "Character sets"): restrict what the recogniser may emit - "this field holds digits", "never emit |" - where each token is
 * chosen (the AR steps' argmax, the refinement pass's inputs, the final decode), not on the finished strings.
 * The class mask has 95 bits, one per logit class: class c is bit c & 31 of mask[c >> 5].  Bit 0 (the end of the text) is always set; for 1 <= i <= 94 bit
 * i is set iff the engine's tokenizer table has at i a character that occurs in allow (NULL or "": every character) and not in deny (NULL or "": none).
 * The table reproduces the reference's quirks: a backslash sets ids 69 and 87; ']' sets id 88, which decodes to nothing; '~', a blank and any non-ASCII
 * byte name no class - a list that holds one fails, and the message names the character.  A set that leaves only the end of the text fails too.
 * ttr_charset_mask: the rule on the host, no engine needed; returns the number of character classes set (1..94), or -1 (ttr_last_error).
 * ttr_engine_set_charset: the engine's set, one at a time, honoured by ttr_parseq_logits and every page entry point (ids, text, prob and conf are those
 * of the constrained choice: prob = 1 / sum over the allowed classes; the logits themselves are never altered).  NULL, NULL resets it; all 95 bits set is
 * "off": the kernels, launches and bits of an engine that never had a set.  It fails, and leaves the previous set in place, while streamed batches are in
 * flight, on a bad list, and - a restricting set only - on a bf16 engine (f16x4 and f32 engines take sets).
 * ttr_engine_get_charset: the mask in force (all 95 bits when none).
 * ttr_logits_confidence_masked: ttr_logits_confidence under a mask of the caller's (bit 0 must be set); the engine's own set is not consulted. */
int ttr_charset_mask(const char* allow, const char* deny, uint32_t mask[3]);
int ttr_engine_set_charset(ttr_engine* e, const char* allow, const char* deny);
int ttr_engine_get_charset(const ttr_engine* e, uint32_t mask[3]);
int ttr_logits_confidence_masked(ttr_engine* e, const float* logits, int n, const uint32_t mask[3], int32_t* ids, float* probs, float* conf);
/* Regions and per-row character sets (DESIGN.md "Regions and per-row character sets"): read quadrilaterals the caller already knows - a form's fields -
 * with no detector, each under its own character set, in ONE recogniser pass.
 * A ttr_region is a quad tl, tr, br, bl in image pixels (pixel centres at integers, as ttr_result_quad returns it) on page `page` of the call, read
 * under set `set`: an index into the call's masks sets[n_sets][3] (ttr_charset_mask's form; bit 0 must be set), or -1 for the engine's own set
 * (ttr_engine_set_charset).  The crop is the rectified sampler's (the kind-1 crop of "Rectified crops") whatever the engine's crop_mode; outside the page
 * the border pixel is replicated.  ttr_region_from_rect: the pixel-edge quad of the pixels [x0, x1) x [y0, y1) (host; -1 for an empty rectangle).
 * ttr_region_geometry (host, no engine): what a region call derives from one quad - fixed[6] = the sampler's coefficients {X0, Ax, Bx, Y0, Ay, By} in 2^-16 px
 * (output pixel (u, v) of the 32 x 128 crop samples (X0 + u Ax + v Bx, Y0 + u Ay + v By)), bbox[4], and *inside = 1 when every corner lies within the pixel
 * edges of an h x w page (the strict_crops test); any output may be NULL.  -1, naming the reason, for a quad the calls refuse.
 * ttr_regions_to_data_dev: n regions on n_pages device pages of ANY sizes and strides (no canvas is shared: no detector runs) -> out[n_pages]; page
 * p's result holds its regions in the caller's order (count 0 for a page without regions): quad = the caller's floats verbatim, bbox = {min x, min y,
 * max x, max y} of the corners, ids / text / prob / conf as on every page entry point, and the item's set index (ttr_result_sets).
 * ttr_image_regions_to_data: the same for one host image (every region's page must be 0) -> *out.
 * Both are synchronous and refuse - before anything is enqueued, the engine stays as it was - while streamed batches are in flight, with a
 * communicator attached, with orient, lines, chars or blocks set (group regions with ttr_group_lines / ttr_group_blocks on their quads), on a
 * coordinate that is not finite or has |x| >= 32768, on a page or set index out of range, on a mask without bit 0, on a restricting mask on a bf16
 * engine, and - strict_crops = 1 - on a region with a corner outside the page's pixel edges [-0.5, w - 0.5] x [-0.5, h - 0.5].
 * ttr_result_sets: [count] each item's set index; NULL for results of the detecting entry points.
 * Stage twins (each refuses while batches stream): ttr_pack_regions - a host image and quads [n][8] -> crops [n][32][128][3]; ttr_parseq_logits_sets -
 * ttr_parseq_logits where crop i chooses under sets[set_of[i]] (-1: the engine's own set); ttr_logits_confidence_sets - ttr_logits_confidence_masked
 * where row i decodes under sets[set_of[i]] (-1: the engine's own set; set_of is not NULL). */
typedef struct ttr_region { float quad[8]; int32_t page; int32_t set; } ttr_region;
int ttr_region_from_rect(int x0, int y0, int x1, int y1, float quad[8]);
int ttr_region_geometry(const float quad[8], int h, int w, int64_t fixed[6], float bbox[4], int* inside);
int ttr_regions_to_data_dev(ttr_engine* e, const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets,
                            ttr_result** out);
int ttr_image_regions_to_data(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const ttr_region* regions, int n, const uint32_t* sets,
                              int n_sets, ttr_result** out);
const int32_t* ttr_result_sets(const ttr_result* r);
int ttr_pack_regions(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const float* quads, int n, uint8_t* crops_out);
int ttr_parseq_logits_sets(ttr_engine* e, const uint8_t* crops, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, float* logits,
                           float* ar_logits, int32_t* ids);
int ttr_logits_confidence_sets(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* ids,
                               float* probs, float* conf);
/* Patterns (DESIGN.md "Patterns"): constrain each word to a regular expression - a date \d{2}/\d{2}/\d{4}, an amount \d+\.\d{2}, a plate
 * [A-Z]{2}\d{2,6} - where each token is chosen: with a pattern in force every returned text (of at most 25 characters, under the character set in
 * force) is a member of the pattern's language, and prob / conf are probabilities over the choices the pattern left open.
 * The syntax is a strict subset of Python's re / POSIX ERE, so re.fullmatch checks a text independently: literals; `\` + a punctuation character as that
 * literal; \d = [0-9]; \w = [A-Za-z0-9_]; `.` = every usable class; [...] with ranges and a leading ^; ( ... ) groups with |; the quantifiers ? * +
 * {m} {m,n} {m,} with 0 <= m <= n <= 25 on an atom or group.  Anchors, back-references, lazy and possessive quantifiers are refused.  The alphabet is the
 * recogniser's classes 1..94 without 88 (which decodes to nothing); a backslash stands for ids 69 and 87; a blank, '~', a non-ASCII byte and a ']' outside
 * its role as the set terminator name no class and are refused by name.  A pattern is compiled under a class mask (ttr_charset_mask's form; NULL = every
 * class): a transition on a blocked class does not exist.  Refused, naming the figure: more than 255 bytes, more than 256 states after minimisation, an
 * empty language, a shortest member of more than 25 characters.
 * ttr_pattern_compile: host only, no engine; *out is freed by ttr_pattern_free.  ttr_pattern_states: states of the minimal automaton (its DONE state not
 * counted); ttr_pattern_min_length: characters of the shortest member; ttr_pattern_table: delta u16 [states + 1][96] (0xFFFF = none; column 0 = the end of
 * the text, which leads from an accepting state to the DONE state; the DONE row holds itself on every class of the mask), mind u8 [states + 1] (characters
 * to acceptance; 255 for DONE), the start state and the DONE state; ttr_pattern_matches: 1 = member, 0 = not, -1 = text names no class somewhere.
 * The choice rule, at character position p (0..25) in state s: class c with t = delta[s][c] may be chosen iff t != 0xFFFF and (c == 0 or mind[t] == 255
 * or p + 1 + mind[t] <= 25); the token is the first maximal index among those classes, then s = t.
 * ttr_engine_set_pattern: the engine's pattern (NULL or "": none), compiled under the engine's character set and recompiled when ttr_engine_set_charset
 * changes it (a set that would leave the pattern an empty language fails and leaves both as they were).  Every page entry point, ttr_parseq_logits and the
 * region calls (each region under its own set) then read every word under it.  It fails, and changes nothing, while streamed batches are in flight, on a
 * bf16 engine, and on an engine with orient, alternatives or a lexicon set; ttr_engine_set_alternatives and ttr_engine_set_lexicon refuse while a pattern
 * is set.  With a communicator attached every rank must be given the same pattern.  Without a pattern no launch, upload or bit differs from before.
 * ttr_regions_to_data_dev_p / ttr_image_regions_to_data_p: the region calls with a pattern per region - region i reads under patterns[pattern_of[i]], -1 =
 * the engine's own pattern (or none); each distinct (pattern, resolved mask) pair is compiled once into one table of at most 1024 states.  They refuse what
 * the region calls refuse, and a pattern index out of range, a bad pattern (naming the region) and a table over 1024 states (naming the total).
 * Stage twins: ttr_parseq_logits_patterns - ttr_parseq_logits_sets with patterns; ttr_logits_decode_patterns - the final decode under patterns alone, row
 * by row: host logits [n][26][95] -> ids, probs [n][26], conf [n] (set_of may be NULL: every row under the engine's set).
 *
 * The decode mode of patterns.  TTR_PATTERN_GREEDY (the default): the text is the one the choice rule above reaches position by position.
 * TTR_PATTERN_BEST: the final decode of every row that has a pattern returns the LIKELIEST member of its language - at most 25 characters, under the row's
 * character set - under the refined per-position distributions.  All fp32: lp[p][c] = (x[p][c] - x[p][id0[p]]) + logf(prob0[p]) for an allowed class, -inf
 * for a blocked one, id0 / prob0 the masked argmax's block on these logits (the lexicon's table, ttr_logits_lexicon); score(w) = the sum in position order
 * from 0.0f of lp[p][w_p], p < L, then + lp[L][0]; the returned w has the largest score by the recurrence V[0][start] = 0, V[p + 1][t] = max over (s, c >= 1,
 * delta[s][c] == t) of V[p][s] + lp[p][c] (ties: lower class, then lower state), the end the maximum over (L <= 25, accepting s) of V[L][s] + lp[L][0]
 * (ties: smaller L, then lower state); -inf and NaN are never chosen.  ids[0 .. L - 1] = w, ids[L] = 0, the positions behind hold the masked argmax; probs[p],
 * p <= L, is expf(x[p][ids[p]] - max_A) / sum_A expf(x - max_A) over the set A the choice rule allows in the path's state - the greedy value 1 / sum where
 * the class is the maximum; conf is the same sequential product (ttr_confidence_from_probs reproduces it).  A row without a pattern, or one in which no
 * member has a finite score, keeps the greedy reading bit for bit.  Where the greedy reading is the likeliest member every bit is greedy mode's; always
 * score(best) >= score(greedy).  The AR loop does not change: its tokens stay the greedy-constrained ones, so a pass's logits are the same bits in both modes
 * and the best path is exact under distributions that were conditioned on the greedy context.
 * ttr_engine_set_pattern_decode: the mode of every page entry point, ttr_parseq_logits and the region calls, fixed for a batch when its recogniser is
 * enqueued; it fails, and changes nothing, for another value, while streamed batches are in flight, and for TTR_PATTERN_BEST on a bf16 engine; without a
 * pattern in force it has no effect, and in greedy mode no launch, allocation, copy or bit differs from before.  ttr_pages_to_data_dev_sharded refuses best
 * mode while a pattern is set.  ttr_result_pattern_logp: [count] floats - score of every item's reading, -inf for an item without a pattern - NULL unless the
 * call ran in best mode with a pattern, and NULL for a result without items (a page on which nothing was found), as the other per-item views are; ttr_results_gather_pattern_logp: the same in ttr_results_gather's item order, -inf for the items of results without
 * the view (logp may be NULL); returns the total.  ttr_logits_decode_patterns_best: ttr_logits_decode_patterns in best mode, whatever the engine's mode, and
 * logp [n].  ttr_pattern_best_from_lp (host only, no engine): the recurrence on a given table lp [26][96] (row p = position p, column 0 = the end of the
 * text, column 95 unused) -> path [26] (the L classes, zeros behind), *len = L, *logp = score; returns 0, 1 when no member has a finite score (path zeros,
 * len -1, logp -inf), -1 for a null argument. */
enum { TTR_PATTERN_GREEDY = 0, TTR_PATTERN_BEST = 1 };
typedef struct ttr_pattern ttr_pattern;
int ttr_pattern_compile(const char* pattern, const uint32_t* mask /* [3] or NULL */, ttr_pattern** out);
void ttr_pattern_free(ttr_pattern* p);
int ttr_pattern_states(const ttr_pattern* p);
int ttr_pattern_min_length(const ttr_pattern* p);
int ttr_pattern_table(const ttr_pattern* p, const uint16_t** delta, const uint8_t** mind, int* start, int* done);
int ttr_pattern_matches(const ttr_pattern* p, const char* text);
int ttr_engine_set_pattern(ttr_engine* e, const char* pattern);
const char* ttr_engine_get_pattern(const ttr_engine* e);
int ttr_regions_to_data_dev_p(ttr_engine* e, const ttr_page* pages, int n_pages, const ttr_region* regions, int n, const uint32_t* sets, int n_sets,
                              const char* const* patterns, int n_patterns, const int32_t* pattern_of, ttr_result** out);
int ttr_image_regions_to_data_p(ttr_engine* e, const uint8_t* hwc_u8, int h, int w, int row_stride, const ttr_region* regions, int n, const uint32_t* sets,
                                int n_sets, const char* const* patterns, int n_patterns, const int32_t* pattern_of, ttr_result** out);
int ttr_parseq_logits_patterns(ttr_engine* e, const uint8_t* crops, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                               const char* const* patterns, int n_patterns, const int32_t* pattern_of, float* logits, float* ar_logits, int32_t* ids);
int ttr_logits_decode_patterns(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                               const char* const* patterns, int n_patterns, const int32_t* pattern_of, int32_t* ids, float* probs, float* conf);
int ttr_engine_set_pattern_decode(ttr_engine* e, int mode);
int ttr_engine_pattern_decode(const ttr_engine* e);
const float* ttr_result_pattern_logp(const ttr_result* r);
int ttr_results_gather_pattern_logp(ttr_result* const* rs, int n, float* logp);
int ttr_logits_decode_patterns_best(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of,
                                    const char* const* patterns, int n_patterns, const int32_t* pattern_of, int32_t* ids, float* probs, float* conf, float* logp);
int ttr_pattern_best_from_lp(const ttr_pattern* p, const float* lp /* [26][96] */, int32_t* path /* [26] */, int32_t* len, float* logp);
/* Character alternatives (DESIGN.md "Character alternatives"): what else each character could have been.  K = alternatives per position, the winner
 * included: 0 (off, the default) or 2..8.  For item i and position p (0..25), under the class mask in force for that crop (the engine's set, or the region's
 * own): alt_ids[p][j], j < K, are the allowed classes in descending order of the refined logit (fp32), ties to the lower class, -1 where fewer than K are
 * allowed; alt_ids[p][0] is ttr_result_ids' id.  alt_probs[p][j] = expf(x[alt_id] - x[id]) * prob[p] in fp32, 0.f in the empty slots; alt_probs[p][0] is
 * ttr_result_prob's value bit for bit.  Every other field of a result is bit for bit that of K = 0; with K = 0 no launch, allocation or copy is added.
 * ttr_engine_set_alternatives: K for every page entry point (the synchronous calls, the list form, the _v forms, streamed batches, the region calls - each
 * region under its own set); with a communicator attached each rank's own results carry them, the gathered payload does not.  It fails, and changes
 * nothing, for K outside {0, 2..8}, while streamed batches are in flight, on a bf16 engine (its kernels take no class mask) and on an engine with
 * orient != 0 (the chosen turn's logits are gone by the time of the choice).  ttr_pages_to_data_dev_sharded refuses an engine with alternatives set.
 * ttr_result_alt_k: K of a result (0 = off).  ttr_result_alt_ids / _probs: item i's [26][K]; the _all views: [count][26][K], NULL when off or empty.
 * ttr_results_gather_alts: ttr_results_gather's item order into ids / probs [total][26][K] (either may be NULL); returns the item count, -1 when the
 * non-empty results differ in K.
 * ttr_logits_alternatives (stage; refuses while batches stream): host logits [n][26][95] through decode_conf_kernel and decode_alts_kernel ->
 * alt_ids / alt_probs [n][26][k], k in 2..8.  sets == NULL: every row under the engine's own set; else row i under sets[set_of[i]] (masks as
 * ttr_charset_mask forms them, bit 0 set), -1 = the engine's own set, as in ttr_logits_confidence_sets.
 * ttr_nbest_from_alts (host, no engine, exact): the m best readings (1 <= m <= 64) of ONE word from its alt_ids / alt_probs [26][k], k in 2..8.  Readings
 * differ from the top reading by substitutions only: one option per character position (the positions before the EOS whose slot-0 id is a character; the
 * options are the slots holding a character - not -1, the EOS or id 88 -, ranked by probability, then slot).  A reading's score is the fp32 product, in
 * position order from 1.0f, of the picked probabilities, times the EOS's slot-0 probability when there is one: reading 0 is the item's (text, conf) bit
 * for bit.  Order: score descending, then rank tuple ascending.  texts receives the readings, each followed by '\n' (written only when cap suffices;
 * *need = the bytes they take), scores [m] their scores (either may be NULL).  Returns the number of readings, or -1 on bad arguments (ttr_last_error). */
int ttr_engine_set_alternatives(ttr_engine* e, int k);
int ttr_engine_alternatives(const ttr_engine* e);
int ttr_result_alt_k(const ttr_result* r);
const int32_t* ttr_result_alt_ids(const ttr_result* r, int i);
const float* ttr_result_alt_probs(const ttr_result* r, int i);
const int32_t* ttr_result_alt_ids_all(const ttr_result* r);
const float* ttr_result_alt_probs_all(const ttr_result* r);
int ttr_results_gather_alts(ttr_result* const* rs, int n, int32_t* ids, float* probs);
int ttr_logits_alternatives(ttr_engine* e, const float* logits, int n, int k, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* alt_ids,
                            float* alt_probs);
int ttr_nbest_from_alts(const int32_t* alt_ids, const float* alt_probs, int k, int m, char* texts, size_t cap, float* scores, size_t* need);
/* Lexicon matching (DESIGN.md "Lexicon matching"): score a caller's word list against each word that is read.  The lexicon holds V words, 1 <= V <= 2^20,
 * each of 1..25 bytes; every byte names exactly one recogniser class in [1, 95) other than 88 - the characters ttr_charset_mask accepts, without ']' and
 * without the backslash (which the table lists twice).  Duplicates are allowed.  M = matches kept per item, 1..8.  For item i, under the class mask in force for
 * that crop (the engine's set, or the region's own), with x the refined logits and id / prob the standard block, all fp32:
 *   lp[p][c] = (x[p][c] - x[p][id[p]]) + logf(prob[p]) for an allowed class, -inf for a blocked one
 *   logp(w)  = the sum, in position order from 0.0f, of lp[p][w_p] for p < L, then + lp[L][0] (the EOS behind the word)
 * lex_idx[j] / lex_logp[j], j < M, are the entries in the total order (logp descending, index ascending); a score that is -inf or NaN is never returned; the
 * slots left over hold -1 / -INFINITY.  An item whose text (1..25 characters, no id 88 before its EOS) is an entry gets that entry in slot 0 (or an equal
 * entry of a lower index), with logp = log(conf) up to rounding.  Every other field of a result is bit for bit that of an engine without a lexicon; with
 * none set no launch, allocation or copy is added.
 * ttr_engine_set_lexicon: the lexicon for every page entry point (the synchronous calls, the list form, the _v forms, streamed batches, the region calls -
 * each region under its own set); words = NULL with n_words = 0 clears it (m is then ignored).  The upload is synchronous; the words are copied.  With a
 * communicator attached each rank's own results carry matches, the gathered payload does not.  It fails, and changes nothing, for a bad word (the message
 * names the first offending word's index), V or M out of range, while streamed batches are in flight, on a bf16 engine (its kernels take no class mask) and
 * on an engine with orient != 0 (the chosen turn's logits are gone by the time of the choice).  ttr_pages_to_data_dev_sharded refuses an engine with a
 * lexicon set.  ttr_engine_lexicon_size / _m: V and M in force (0 = none).  ttr_engine_lexicon_word: entry idx as the engine holds it, NULL out of range;
 * valid until the next ttr_engine_set_lexicon.
 * ttr_result_lex_m: M of a result (0 = none).  ttr_result_lex_idx / _logp: item i's [M]; the _all views: [count][M], NULL when off or empty.
 * ttr_lexicon_encode (host, no engine): the 32-byte device records of n words into records [n][32] - byte 0 the length, bytes 1..L the classes, zeros behind;
 * applies the validation above.  Returns 0, or -1 with the message in ttr_last_error.
 * ttr_logits_lexicon (stage; refuses while batches stream): host logits [n][26][95] through decode_conf_kernel and the scorer under the engine's lexicon ->
 * idx / logp [n][M] (either may be NULL).  sets / n_sets / set_of as in ttr_logits_alternatives. */
int ttr_engine_set_lexicon(ttr_engine* e, const char* const* words, int n_words, int m);
int ttr_engine_lexicon_size(const ttr_engine* e);
int ttr_engine_lexicon_m(const ttr_engine* e);
const char* ttr_engine_lexicon_word(const ttr_engine* e, int idx);
int ttr_result_lex_m(const ttr_result* r);
const int32_t* ttr_result_lex_idx(const ttr_result* r, int i);
const float* ttr_result_lex_logp(const ttr_result* r, int i);
const int32_t* ttr_result_lex_idx_all(const ttr_result* r);
const float* ttr_result_lex_logp_all(const ttr_result* r);
int ttr_lexicon_encode(const char* const* words, int n, uint8_t* records);
int ttr_logits_lexicon(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int32_t* idx, float* logp);
/* Fuzzy alignment (opt-in; DESIGN.md "Lexicon matching", Fuzzy alignment): the rule above indexes - character j of an entry is looked up at position j - so
 * it covers substitutions and nothing else; a reading with one character dropped or doubled shifts every position behind the slip.  With a band B in 0..3 and
 * a gap g (fp32, finite, <= 0: the log-probability charged for one dropped or one extra character) an entry w of L characters is aligned instead.  lp is the
 * table above, unchanged.  A cell D[j][p] stands for "j characters of the entry and p positions of the reading consumed"; it exists for 0 <= j <= L,
 * 0 <= p <= 25, |j - p| <= B, and holds a pair (score fp32, edits int).
 *   D[0][0] = (0.0f, 0); every other cell starts at (-inf, 0)
 *   a candidate replaces the cell's value iff cand.score > cur.score, or cand.score == cur.score and cand.edits < cur.edits (comparisons with NaN are
 *   false: a NaN is never taken up and never spreads)
 *   the candidates of D[j][p], each only from a cell that exists:
 *     match                                                  (D[j-1][p-1].score + lp[p-1][w[j-1]], edits)
 *     extra character in the reading (position p-1 skipped)  (D[j][p-1].score + g, edits + 1)
 *     dropped character (entry character j-1 skipped)        (D[j-1][p].score + g, edits + 1)
 *   the end: over the cells D[L][p] that exist, the candidates (D[L][p].score + lp[p][0], edits) under the same rule from (-inf, 0): the winner is logp(w)
 *   and edits(w)
 * Every operation is one fp32 addition or one comparison, and the order of the additions along a path is the path's own: the result is a function of (table,
 * entry, B, g) alone.  At B = 0 the only path is the diagonal: logp is the rigid rule's value bit for bit, edits 0.  logp never decreases as B grows.
 * Ranking, the empty slots and "never -inf or NaN" are the lexicon's own; lex_edits [count][M] int32 holds each match's edits, -1 in the empty slots.
 * ttr_engine_set_lexicon_fuzzy: the mode for everything that carries a lexicon (the synchronous calls, the list form, the _v forms, streamed batches, the
 * region calls - each region under its own set); band = -1 switches it off (gap is then ignored).  It may be set with no lexicon in place and survives
 * ttr_engine_set_lexicon.  It fails, and changes nothing, for a band outside -1..3, a gap that is not finite or is > 0, and while streamed batches are in
 * flight.  With the mode off no launch, allocation, copy or bit differs from an engine that never heard of it.  The convenience layers default to band 1
 * with g = -6.9077554f (ln 1e-3); neither has been tuned on documents.  ttr_engine_lexicon_fuzzy: the band (-1 = off) and gap in force; either may be NULL.
 * ttr_result_lex_band: the band a result's matches were scored under, -1 when off.  ttr_result_lex_edits: item i's [M]; the _all view: [count][M]; NULL when
 * the mode is off or the result is empty.
 * ttr_lexicon_fuzzy_from_lp (host, no engine): the rule for n records [n][32] (ttr_lexicon_encode's) against one table lp [26][96] -> logp [n], edits [n].
 * Returns 0, or -1 for a null argument, a band outside 0..3, a gap that is not finite or is > 0, or a record whose length byte is outside 1..25 or that holds
 * a class byte >= 96.
 * ttr_logits_lexicon_fuzzy (stage; refuses while batches stream): ttr_logits_lexicon through the fuzzy scorer under (band, gap), whatever the engine's mode
 * -> idx / logp / edits [n][M] (any may be NULL). */
int ttr_engine_set_lexicon_fuzzy(ttr_engine* e, int band, float gap);
int ttr_engine_lexicon_fuzzy(const ttr_engine* e, int* band, float* gap);
int ttr_result_lex_band(const ttr_result* r);
const int32_t* ttr_result_lex_edits(const ttr_result* r, int i);
const int32_t* ttr_result_lex_edits_all(const ttr_result* r);
int ttr_lexicon_fuzzy_from_lp(const float* lp, const uint8_t* records, int n, int band, float gap, float* logp, int32_t* edits);
int ttr_logits_lexicon_fuzzy(ttr_engine* e, const float* logits, int n, const uint32_t* sets, int n_sets, const int32_t* set_of, int band, float gap,
                             int32_t* idx, float* logp, int32_t* edits);
/* ---- wide words (opt-in; DESIGN.md "Wide words") ---------------------------------------------
 * Every recogniser row is one crop stretched to 32 x 128, and the recogniser emits at most 25 characters: a URL, an IBAN or a whole line handed in as one region
 * reaches it with a few columns per character.  With ttr_engine_set_wide(e, max_aspect) a word whose quad is wider than max_aspect times its height is cut into
 * n = min(16, ceil(aspect / max_aspect)) pieces at the gaps between characters, found in the page's own pixels (wide.hip), every piece is read as one more
 * recogniser row of the same pass, and the readings are joined: the item's text is the pieces' texts concatenated (nothing between them), its conf the fp32
 * product of the pieces' conf in order from 1.0f; its ids and prob rows are its first piece's.  bbox, quad, item count and order never change; a word with
 * n = 1 keeps every bit.  Past 16 max_aspect the pieces are simply wider than max_aspect.
 * max_aspect: 0 = off (the default), else a finite value in [2, 64]; anything else fails and changes nothing.  The setter also refuses, naming the reason: while
 * streamed batches are in flight; on an engine whose crop_mode is not TTR_CROP_RECTIFIED; with orient or chars set; with alternatives, a lexicon or a pattern
 * set; with a communicator attached.  The other way round ttr_engine_set_alternatives / _set_lexicon / _set_pattern, ttr_engine_attach_comm, a region call with
 * patterns and ttr_pages_to_data_dev_sharded refuse while wide is on.  Character sets apply: the engine's on page calls, a region's own on each of its pieces.
 * Result views (NULL / 0 with wide off and for an empty result): ttr_result_piece_first [count + 1] - item i owns pieces [first[i], first[i + 1]), an item that
 * is not wide owns one, itself; ttr_result_piece_ids / _piece_probs [P][26]; _piece_confs [P]; _piece_quads [P][8] (tl, tr, br, bl); _piece_cuts [count][17] -
 * c_0 = 0 < ... < c_n = 128 n in columns of the word's frame, -1 beyond n.  ttr_results_gather_pieces: the views of n results back to back - first
 * [sum(count) + n] (each page's offsets from 0), ids / probs / confs / quads by piece, cuts by item; any pointer may be NULL; returns the total piece count, -1
 * for bad arguments.
 * The rule on the host, no engine (each returns 0 or the value named, -1 with the message in ttr_last_error):
 *   ttr_wide_plan             quad [8], max_aspect (in [2, 64]) -> returns n; frame [6] = {X0f, Axf, Bxf, Y0f, Ayf, Byf} in 2^-16 px over 128 n columns x 32 rows
 *   ttr_wide_profile          a host image u8 [h][w][3] (row_stride bytes, 0 = 3 w), frame, n -> q u16 [128 n]
 *   ttr_wide_cuts_from_profile  q [128 n], n -> cuts [17]
 *   ttr_wide_piece_coef       frame, c0, c1 -> the packer row [8] = {1, X0, Ax, Bx, Y0, Ay, By, 0} of the piece over columns [c0, c1)
 *   ttr_wide_piece_quads      quad [8], cuts, n -> quads [n][8]
 * ttr_wide_cuts (stage; refuses while batches stream): a host image and nq quads through wide_cut_kernel, whatever the engine's setting; use_table != 0 reads
 * the page through the device page table as mixed-size batches do.  n_out [nq], cuts [nq][17], profiles [nq][2048] (0 beyond 128 n), coef [nq][16][8] (piece
 * j of quad i at row 16 i + j, zeros beyond n); any output may be NULL. */
int ttr_engine_set_wide(ttr_engine* e, float max_aspect);
float ttr_engine_wide(const ttr_engine* e);
const int32_t* ttr_result_piece_first(const ttr_result* r);
const int32_t* ttr_result_piece_ids(const ttr_result* r);
const float* ttr_result_piece_probs(const ttr_result* r);
const float* ttr_result_piece_confs(const ttr_result* r);
const float* ttr_result_piece_quads(const ttr_result* r);
const int32_t* ttr_result_piece_cuts(const ttr_result* r);
int ttr_results_gather_pieces(ttr_result* const* rs, int n, int32_t* first, int32_t* ids, float* probs, float* confs, float* quads, int32_t* cuts);
int ttr_wide_plan(const float quad[8], float max_aspect, int64_t frame[6]);
int ttr_wide_profile(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], int n, uint16_t* q);
int ttr_wide_cuts_from_profile(const uint16_t* q, int n, int32_t cuts[17]);
int ttr_wide_piece_coef(const int64_t frame[6], int c0, int c1, int64_t row[8]);
int ttr_wide_piece_quads(const float quad[8], const int32_t* cuts, int n, float* quads);
int ttr_wide_cuts(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, float max_aspect, int use_table, int32_t* n_out,
                  int32_t* cuts, uint16_t* profiles, int64_t* coef);
/* ---- curved words (opt-in; DESIGN.md "Curved words") ------------------------------------------
 * A word set on an arc - on a seal, a stamp, a logo - is boxed by a quad far taller than its text, and stretched to 32 x 128 its glyphs ride up and down the crop.
 * With ttr_engine_set_curved(e, 1) every word's spine is sought in the page's own pixels inside its quad (curve.hip, behind the unchanged packer, one launch per
 * batch); a word whose spine bends by at least half its band has its crop made again along the spine, nine knots and eight straight segments, and the recogniser
 * reads that.  The row count of a batch does not change, so a word that is not curved keeps ids, prob, conf and text bit for bit; bbox, quad, item count and
 * order never change.  on: 0 = off (the default) or 1; anything else fails and changes nothing.  The setter also refuses, naming the reason: while streamed
 * batches are in flight; on an engine whose crop_mode is not TTR_CROP_RECTIFIED; with orient or chars set; with wide words on; with a communicator attached.  The
 * other way round ttr_engine_set_wide, ttr_engine_attach_comm and ttr_pages_to_data_dev_sharded refuse while curved is on.  Character sets, alternatives, a
 * lexicon and patterns apply as ever: they act on recogniser rows.
 * Result views (NULL with curved off and for an empty result): ttr_result_curved [count] (1 = straightened); ttr_result_outlines [count][18][2] - the top edge
 * C_j - H_j left to right, then the bottom edge C_j + H_j right to left; for a word that is not curved the quad's long sides at the same nine stations;
 * ttr_result_spine_knots [count][9][4] int64 - {Cx, Cy, Hx, Hy} in 2^-16 px (zeros for a word whose second pass did not run).  ttr_results_gather_curved: the
 * views of n results back to back, any pointer may be NULL; returns the number of curved items, -1 for bad arguments.
 * The rule on the host, no engine (each returns 0 or the value named, -1 with the message in ttr_last_error):
 *   ttr_curve_frame    quad [8] -> frame [6] = {X0, Ax, Bx, Y0, Ay, By} in 2^-16 px over 128 columns x 64 rows
 *   ttr_curve_columns  a host image u8 [h][w][3] (row_stride bytes, 0 = 3 w), frame, knots (NULL = pass 1 over the frame, else pass 2 over the band of that
 *                      table [9][4]) -> stats [4][128] = G | M | first | last
 *   ttr_curve_knots    image, frame -> returns the flag; flag, hb [2], spine [2][9] (1/256 row), knots [9][4], knots1 [9][4] (pass 1's table); any may be NULL
 *   ttr_curve_crop     image, knots [9][4] -> crop u8 [32][128][3]
 *   ttr_curve_outline  quad [8], flag, knots -> outline [18][2]
 * ttr_curve_crops (stage; refuses while batches stream): a host image and nq quads through the kind-1 packer and curve_crop_kernel, whatever the engine's
 * setting; use_table != 0 reads the page through the device page table as mixed-size batches do.  flag [nq], hb [nq][2], spine [nq][2][9], knots [nq][9][4],
 * crops [nq][32][128][3] (the kind-1 crop for a quad that is not curved); any output may be NULL. */
int ttr_engine_set_curved(ttr_engine* e, int on);
int ttr_engine_curved(const ttr_engine* e);
const int32_t* ttr_result_curved(const ttr_result* r);
const float* ttr_result_outlines(const ttr_result* r);
const int64_t* ttr_result_spine_knots(const ttr_result* r);
int ttr_results_gather_curved(ttr_result* const* rs, int n, int32_t* curved, float* outlines, int64_t* knots);
int ttr_curve_frame(const float quad[8], int64_t frame[6]);
int ttr_curve_columns(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], const int64_t* knots, int32_t* stats);
int ttr_curve_knots(const uint8_t* img, int h, int w, int row_stride, const int64_t frame[6], int32_t* flag, int32_t hb[2], int32_t* spine, int64_t* knots, int64_t* knots1);
int ttr_curve_crop(const uint8_t* img, int h, int w, int row_stride, const int64_t* knots, uint8_t* crop);
int ttr_curve_outline(const float quad[8], int flag, const int64_t* knots, float* outline);
int ttr_curve_crops(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, const float* quads, int nq, int use_table, int32_t* flag, int32_t* hb,
                    int32_t* spine, int64_t* knots, uint8_t* crops);
/* ---- tiled pages (opt-in; DESIGN.md "Tiled pages") -----------------------------------------------------------------------------------------------
 * The detector sees a canvas of at most canvas_size pixels on its longer side: a 300 dpi A4 scan is shrunk 3.4 times before it is looked at.  With
 * ttr_engine_set_tiled(e, overlap) a page keeps its own scale (ratio 1, page canvas c32(h) x c32(w), c32 = rounded up to a multiple of 32); one larger than
 * canvas_size is cut into overlapping tiles that share one canvas and run as one detector batch, and their heat maps are stitched into one page map
 * (tile_stitch_kernel, one launch per batch) that everything behind the detector reads as ever.  overlap: 0 = off (the default), else a multiple of 32 in
 * [64, canvas_size / 4].  The setter fails and changes nothing on another value, on an engine whose canvas_size is no multiple of 32 or whose mag_ratio is
 * not 1.0, while streamed batches are in flight and with a communicator attached; ttr_engine_attach_comm and ttr_pages_to_data_dev_sharded refuse while it is
 * on.  A call refuses, naming the figure, a page side above 8192 and a page of more than 16 tiles on an axis or 64 in all.  A page that fits one tile gives
 * the bits of the engine with tiling off; with tiling off nothing differs from before.  The pages of a batch must share the page canvas, which
 * ttr_canvas_geometry reports (ttr_images_to_data buckets by it when mixed_batches is set).  Neither the overlap nor the 16-pixel feather has been tuned on
 * documents.  ttr_result_tiles: the tiles a page's detector ran as, 0 when off.
 * The rule on the host, no engine (each returns 0, or -1 with the message in ttr_last_error):
 *   ttr_tile_plan     one page of h x w under (canvas_size, overlap, mag_ratio): *ny x *nx tiles, origins oy / ox and extents ey / ex (16 ints each, image
 *                     pixels), the tiles' shared canvas *Hc x *Wc, the page map *H2 x *W2.  Any output may be NULL
 *   ttr_stitch_tiles  tiles f32 [pages][ny nx][Hc / 2][Wc / 2][2] (a page's tiles in (ty, tx) order) -> out f32 [pages][H2][W2][2] under the given origins,
 *                     which are checked (multiples of 32, ascending, overlaps of at least 32, the last tile ending at the map's end).  Outside the feather bands
 *                     a copy, inside lerp(a, b, t) = a + t (b - a), x first, then y, every operation rounded on its own
 * Stage calls (refuse while batches stream): ttr_stitch_heat - the same through tile_stitch_kernel, bit for bit; ttr_craft_heatmap_tiled - a host image under
 * `overlap`, whatever the engine's setting -> the page map f32 [*H2][*W2][2] (cap = floats heat_out holds; heat_out NULL: sizes only); ttr_tile_canvases - the
 * tiles' canvases u8 [ny nx][Hc][Wc][3] as the detector gets them (cap = bytes). */
int ttr_engine_set_tiled(ttr_engine* e, int overlap);
int ttr_engine_tiled(const ttr_engine* e);
int ttr_result_tiles(const ttr_result* r);
int ttr_tile_plan(int h, int w, int canvas_size, int overlap, float mag_ratio, int* ny, int* nx, int* oy, int* ox, int* ey, int* ex, int* Hc, int* Wc, int* H2, int* W2);
int ttr_stitch_tiles(const float* tiles, int pages, int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2, float* out);
int ttr_stitch_heat(ttr_engine* e, const float* tiles, int pages, int ny, int nx, const int* oy, const int* ox, int Hc, int Wc, int H2, int W2, float* out);
int ttr_craft_heatmap_tiled(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int overlap, float* heat_out, size_t cap, int* H2, int* W2);
int ttr_tile_canvases(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int overlap, uint8_t* canvases, size_t cap);
/* ---- tables (opt-in; DESIGN.md "Tables") ---------------------------------------------------------
 * With ttr_engine_set_tables(e, min_len, ink) every page call also finds the ruling lines in the page's own pixels (table_ink_kernel, tables.hip: one bit per
 * pixel), groups them into tables, derives each table's grid and merged cells (table_grid_kernel, one workgroup per page) and says for every item which table
 * and cell it lies in.  Items, order, boxes, text, ids, conf and every other layer's outputs keep their bits; with tables off nothing runs.  min_len = 0 is off
 * (the default), else min_len in 16..4096 (the shortest ruling, px) and ink in 1..255 (a pixel is ink iff the mean of its three bytes is below it); the
 * convenience layers use 48 and 128, and neither value has been tuned on documents.  The setter refuses while streamed batches are in flight and with a
 * communicator attached; ttr_engine_attach_comm and ttr_pages_to_data_dev_sharded refuse while tables are on; region calls leave the views empty.
 * Caps (a page beyond one reports mode = -(step of the rule) and nothing else): 8192 runs and 256 rulings per direction, 32 tables, 64 lines per axis and
 * table, 1024 cells.
 * Result views (NULL / 0 with tables off and for an empty result):
 *   ttr_result_table_mode      1, or -2 / -4 / -6 / -7; 0 when off
 *   ttr_result_rulings         [ruling_count][6] int32: dir (0 horizontal, 1 vertical), x0, y0, x1, y1 (inclusive px), table (-1 = loose)
 *   ttr_result_tables          [table_count][8]: x0, y0, x1, y1, rows, cols, first cell, cell count
 *   ttr_result_table_lines     per table its rows + 1 row lines, then its cols + 1 column lines, back to back, in doubled px; *n receives their number
 *   ttr_result_cells           [cell_count][9]: table, row, col, rowspan, colspan, x0, y0, x1, y1
 *   ttr_result_item_table / ttr_result_item_cell   [count]: -1 for an item in no cell
 *   ttr_result_cell_text       the items of cell c through the host line rule, words joined by a space, lines by '\n'; returns the length (without the
 *                              terminator) and writes at most cap bytes, terminator included; -1 for a bad cell
 * ttr_results_gather_tables: item_table / item_cell of n results back to back (-1 where a result has none); returns the number of items in a cell.
 * ttr_tables_from_page: the rule on the host, no engine.  A host image u8 [h][w][3] (row_stride bytes, 0 = 3 w) and nq quads [nq][8] -> mode, counts [6] =
 * {rulings, tables, cells, line values, horizontal runs, vertical runs} (all 0 for a page beyond a cap), rulings [512][6], tables [32][8], lines [32 * 130], cells [1024][9] (capacities; counts says how much is valid),
 * item_table [nq], item_cell [nq]; any output may be NULL.  Returns 0, -1 with the message in ttr_last_error (min_len outside 16..4096, ink outside 1..255, a
 * quad with a coordinate that is not finite or has |x| >= 32768, a page side of 32768 or more).
 * ttr_tables_page (stage; refuses while batches stream): the same through the two kernels, whatever the engine's setting. */
int ttr_engine_set_tables(ttr_engine* e, int min_len, int ink);
int ttr_engine_tables(const ttr_engine* e, int* ink);
int ttr_result_table_mode(const ttr_result* r);
int ttr_result_ruling_count(const ttr_result* r);
const int32_t* ttr_result_rulings(const ttr_result* r);
int ttr_result_table_count(const ttr_result* r);
const int32_t* ttr_result_tables(const ttr_result* r);
const int32_t* ttr_result_table_lines(const ttr_result* r, int* n);
int ttr_result_cell_count(const ttr_result* r);
const int32_t* ttr_result_cells(const ttr_result* r);
const int32_t* ttr_result_item_table(const ttr_result* r);
const int32_t* ttr_result_item_cell(const ttr_result* r);
int ttr_result_cell_text(const ttr_result* r, int c, char* buf, int cap);
int ttr_results_gather_tables(ttr_result* const* rs, int n, int32_t* item_table, int32_t* item_cell);
int ttr_tables_from_page(const uint8_t* img, int h, int w, int row_stride, int min_len, int ink, const float* quads, int nq, int32_t* mode, int32_t* counts,
                         int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell);
int ttr_tables_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_len, int ink, const float* quads, int nq, int32_t* mode,
                    int32_t* counts, int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell);
/* ---- deskew (opt-in; DESIGN.md "Deskew") ---------------------------------------------------------
 * With ttr_engine_set_deskew(e, max_slope, gain, ink) every page of a page call has its skew estimated on the GPU from its own pixels (table_ink_kernel's bitmap,
 * deskew_score_kernel: one workgroup per page and candidate slope) and is resampled upright about its centre, at its own size, into an engine-owned buffer
 * (deskew_rotate_kernel) before the detector reads it.  Everything behind - boxes, quads, text, lines, blocks, characters, tables, wide and curved words - is
 * exactly what the same call returns for that upright page with the layer off, in the upright page's coordinates; ttr_result_to_page maps points back to the
 * caller's page.  A page found straight (slope 0) keeps every byte.  max_slope = 0 is off (the default: nothing runs), else max_slope in 1..128 - candidate
 * slopes are k in -max_slope..max_slope, a text line dropping k px per 512 px to the right, 128 = 14 degrees -, gain in 256..65535 (in 1/256ths: a page is
 * turned only when score[found] * 256 >= score[0] * gain) and ink in 1..255 (as for tables).  The convenience layers use 64, 288 and 128; none of them has been
 * tuned on documents.  The setter refuses while streamed batches are in flight and with a communicator attached; ttr_engine_attach_comm and
 * ttr_pages_to_data_dev_sharded refuse while it is on; a page call refuses a page with a side of 8192 px or more.  Region calls run as before and report slope 0.
 *   ttr_engine_deskew          max_slope in force (0 = off); gain and ink through the pointers (may be NULL)
 *   ttr_result_skew            the page's record (a ttr_result is one page); returns 1, or 0 when the result carries none (the layer was off)
 *   ttr_result_to_page         n points (x, y) of the upright page -> the caller's page: xs = (w-1)/2 + (C (x - (w-1)/2) - S (y - (h-1)/2)) / 65536 and
 *                              ys = (h-1)/2 + (S (x - ..) + C (y - ..)) / 65536, in double, rounded to float; the identity for a result without a record;
 *                              xy_out may be xy_in.  Returns 0, -1 on a null argument
 *   ttr_skew_to_page           the same map from a record alone (C, S, w, h are read): what every binding's map back calls
 *   ttr_results_gather_skew    the records of n results back to back (zeroes where a result has none); returns the number of pages that were resampled
 * ttr_deskew_from_page: the rule on the host, no engine.  A host image u8 [h][w][3] (row_stride bytes, 0 = 3 w; the rule treats the three channels alike, so
 * either channel order gives the same record) -> out_img [h][w][3] tightly packed, rec, scores [2 max_slope + 1] (slope k at k + max_slope); any output may be
 * NULL.  Returns 0, -1 with the message in ttr_last_error (an argument outside its range, a page side of 8192 or more).
 * ttr_deskew_page (stage; refuses while batches stream): the same through the kernels, whatever the engine's setting. */
typedef struct ttr_skew {
  int32_t slope, found;        /* the slope the page was turned by (0: left as it was); the slope of the largest score */
  int32_t C, S;                /* llrint(65536 cos), llrint(65536 sin) of slope */
  int32_t w, h;
  int32_t mode, reserved;      /* 1 resampled, 0 left as it was */
  uint64_t score0, score_found;
} ttr_skew;
int ttr_engine_set_deskew(ttr_engine* e, int max_slope, int gain, int ink);
int ttr_engine_deskew(const ttr_engine* e, int* gain, int* ink);
int ttr_result_skew(const ttr_result* r, ttr_skew* rec);
int ttr_result_to_page(const ttr_result* r, const float* xy_in, int n, float* xy_out);
int ttr_skew_to_page(const ttr_skew* rec, const float* xy_in, int n, float* xy_out);   /* the same map from a record alone (C, S, w, h are read) */
int ttr_results_gather_skew(ttr_result* const* rs, int n, ttr_skew* recs);
int ttr_deskew_from_page(const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int ink, uint8_t* out_img, ttr_skew* rec, uint64_t* scores);
int ttr_deskew_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int ink, uint8_t* out_img, ttr_skew* rec, uint64_t* scores);
/* ---- local ink (opt-in; DESIGN.md "Local ink") --------------------------------------------------
 * Tables and deskew start from one ink bitmap, by default a global threshold (b0 + b1 + b2 < 3 ink): dark ink on light paper only.  With
 * ttr_engine_set_ink(e, radius, drop, polarity) the engine's tables and deskew passes take that bitmap from an adaptive threshold instead: with s = b0 + b1 + b2,
 * n and S the area and the sum of s of the window [x - radius, x + radius] x [y - radius, y + radius] clipped to the page, a pixel is ink iff
 * s n 256 < S (256 - drop) - darker than its neighbourhood's mean by drop 256ths -, in integers (ink_rows_kernel and ink_local_kernel; the layout of the bitmaps
 * and everything behind them is unchanged).  radius = 0 is off (the default: nothing runs, and every launch and bit is as before), else radius in 1..64, drop
 * in 1..255 and polarity 0 (dark ink), 1 (light ink: s becomes 765 - s) or 2 (auto: light iff twice the page's sum of s is below 765 h w; a tie stays dark).
 * The convenience layers use 16, 38 and 2, which nobody has tuned on documents.  On, the `ink` of ttr_engine_set_tables / ttr_engine_set_deskew is not consulted.
 * A blank or all-black page carries no ink; a solid region thicker than the window loses its interior; the bitmap of 255 - page under light ink is that of page
 * under dark ink, bit for bit.  The setter refuses values outside the ranges and while streamed batches are in flight; with neither tables nor deskew on it is
 * accepted and nothing runs.  The stage calls ttr_tables_page / ttr_deskew_page keep the fixed rule, whatever the engine's setting.
 *   ttr_engine_ink             radius in force (0 = off); drop and polarity through the pointers (may be NULL)
 *   ttr_result_ink             the page's record - that of the tables pass when tables ran, else that of the deskew pass; returns 1, or 0 when the result carries none
 *   ttr_results_gather_ink     the records of n results back to back (zeroes where a result has none); returns the number of pages read as light ink
 * ttr_ink_from_page: the rule on the host, no engine.  A host image u8 [h][w][3] (row_stride bytes, 0 = 3 w) -> bits [h][ceil(w / 64)] uint64 (bit x % 64 of word
 * x / 64), bitsT [w][ceil(h / 64)] the same bits along y, rec; any output may be NULL.  Returns 0, -1 with the message in ttr_last_error.
 * ttr_ink_page (stage; refuses while batches stream): the same through the kernels, whatever the engine's setting.
 * ttr_tables_from_page_ink / ttr_deskew_from_page_ink: ttr_tables_from_page / ttr_deskew_from_page with (radius, drop, polarity) in the place of ink. */
typedef struct ttr_ink {
  int32_t radius, drop, polarity, inverted;   /* inverted: 1 = the page was read as light ink on dark paper */
  uint64_t sum;                               /* the page's sum of b0 + b1 + b2 */
  int32_t w, h;
} ttr_ink;
int ttr_engine_set_ink(ttr_engine* e, int radius, int drop, int polarity);
int ttr_engine_ink(const ttr_engine* e, int* drop, int* polarity);
int ttr_result_ink(const ttr_result* r, ttr_ink* rec);
int ttr_results_gather_ink(ttr_result* const* rs, int n, ttr_ink* recs);
int ttr_ink_from_page(const uint8_t* img, int h, int w, int row_stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, ttr_ink* rec);
int ttr_ink_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int radius, int drop, int polarity, uint64_t* bits, uint64_t* bitsT, ttr_ink* rec);
int ttr_tables_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_len, int radius, int drop, int polarity, const float* quads, int nq, int32_t* mode,
                             int32_t* counts, int32_t* rulings, int32_t* tables, int32_t* lines, int32_t* cells, int32_t* item_table, int32_t* item_cell);
int ttr_deskew_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int max_slope, int gain, int radius, int drop, int polarity, uint8_t* out_img, ttr_skew* rec,
                             uint64_t* scores);
/* ---- selection marks (opt-in; DESIGN.md "Selection marks") ----------------------------------------------
 * With ttr_engine_set_marks(e, min_side, max_side, fill, ink) every page call also finds the page's checkboxes - small square frames - on the ink bitmap of
 * the page's own pixels (mark_cand_kernel, marks.hip: pages x row bands), reads each one's state from the ink inside it, and says for every item which mark
 * its centre lies in and for every mark which item stands to its right (mark_page_kernel, one workgroup per page).  Items, order, boxes, text, ids, conf and
 * every other layer's outputs keep their bits; with marks off nothing runs.  min_side = 0 is off (the default), else min_side in 8..64 and max_side in
 * min_side..128 (the frame's sides, px), fill in 1..255 (selected iff 256 inked >= fill area over the interior) and ink in 1..255 (as for tables); the
 * convenience layers use 10, 64, 24 and 128, and none of these values has been tuned on documents.  With tables on under the same ink rule the bitmaps are
 * formed once for both layers; with local ink on they are local ink's.  Unlike tables the layer runs for a page without words.  The setter refuses while
 * streamed batches are in flight and with a communicator attached; ttr_engine_attach_comm and ttr_pages_to_data_dev_sharded refuse while marks are on;
 * region calls leave the views empty.  Under deskew the coordinates are the upright page's.  Cap: 512 marks a page; a page beyond it reports mode -6, no
 * marks and -1 for every item.
 * Result views (NULL / 0 with marks off):
 *   ttr_result_mark_mode       1, or -6; 0 when off
 *   ttr_result_marks           [mark_count][12] int32: x0, y0, x1, y1 (the frame, inclusive px), ix0, iy0, ix1, iy1 (the interior), inked, area, state (1 =
 *                              selected), label (the item the box stands in front of, -1 = none); in (y0, x0) order
 *   ttr_result_item_mark       [count]: the mark an item's centre lies in (the `x` read inside a ticked box), -1 for none
 * ttr_results_gather_marks: item_mark of n results back to back (-1 where a result has none); returns the number of items inside a mark.
 * ttr_marks_from_page: the rule on the host, no engine.  A host image u8 [h][w][3] (row_stride bytes, 0 = 3 w) and nq quads [nq][8] -> mode, counts [3] =
 * {marks, corners examined, candidates kept (beyond 512 on a page of mode -6)}, marks [512][12] (capacity; counts[0] says how much is valid), item_mark [nq];
 * any output may be NULL.  Returns 0, -1 with the message in ttr_last_error (a parameter outside its range, a quad with a coordinate that is not finite or
 * has |x| >= 32768, a page side of 32768 or more).  ttr_marks_from_page_ink: the same with local ink's (radius, drop, polarity) in the place of ink.
 * ttr_marks_page (stage; refuses while batches stream): the same through the kernels under the fixed ink rule, whatever the engine's setting. */
int ttr_engine_set_marks(ttr_engine* e, int min_side, int max_side, int fill, int ink);
int ttr_engine_marks(const ttr_engine* e, int* max_side, int* fill, int* ink);
int ttr_result_mark_mode(const ttr_result* r);
int ttr_result_mark_count(const ttr_result* r);
const int32_t* ttr_result_marks(const ttr_result* r);
const int32_t* ttr_result_item_mark(const ttr_result* r);
int ttr_results_gather_marks(ttr_result* const* rs, int n, int32_t* item_mark);
int ttr_marks_from_page(const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int ink, const float* quads, int nq, int32_t* mode,
                        int32_t* counts, int32_t* marks, int32_t* item_mark);
int ttr_marks_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int radius, int drop, int polarity, const float* quads,
                            int nq, int32_t* mode, int32_t* counts, int32_t* marks, int32_t* item_mark);
int ttr_marks_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_side, int max_side, int fill, int ink, const float* quads, int nq, int32_t* mode,
                   int32_t* counts, int32_t* marks, int32_t* item_mark);
/* ---- barcodes (opt-in; DESIGN.md "Barcodes") --------------------------------------------------------------
 * With ttr_engine_set_barcodes(e, min_lines, ink, symbologies) every page call also reads the page's Code 128 and Code 39 barcodes off single lines of the ink
 * bitmaps of the page's own pixels - every row and every column, forwards and backwards (barcode_scan_kernel, barcodes.hip: pages x bands of lines) -, chains
 * the lines' readings into barcodes and says for every item which barcode its centre lies in, so that the junk words the detector makes of the bars can be
 * dropped (barcode_page_kernel, one workgroup per page).  Items, order, boxes, text, ids, conf and every other layer's outputs keep their bits; with barcodes
 * off nothing runs.  min_lines = 0 is off (the default), else min_lines in 4..256 (the scan lines that must agree), ink in 1..255 (as for tables) and
 * symbologies in 1..3 (bit 0 Code 128, bit 1 Code 39); the convenience layers use 8, 128 and 3, and none of these values has been tuned on documents.  With
 * tables or marks on under the same ink rule the bitmaps are formed once for all; with local ink on they are local ink's.  Like marks the layer runs for a
 * page without words.  The setter refuses while streamed batches are in flight and with a communicator attached; ttr_engine_attach_comm and
 * ttr_pages_to_data_dev_sharded refuse while barcodes are on; region calls leave the views empty.  Under deskew the coordinates are the upright page's.  Cap: 64
 * barcodes a page; a page beyond it reports mode -7, no barcodes and -1 for every item.  Scope: one scan line must cross every bar (turn deskew on for
 * tilted pages); no Code 39 check character, no full-ASCII Code 39; quiet zones of half the standards' width are accepted.
 * Result views (NULL / 0 with barcodes off):
 *   ttr_result_barcode_mode    1, or -7; 0 when off
 *   ttr_result_barcodes        [barcode_count][24] int32: x0, y0, x1, y1 (inclusive px), symbology (1 Code 128, 2 Code 39), dir (0 left to right, 1 top to
 *                              bottom, 2 right to left, 3 bottom to top), lines (the scan lines that agreed), module64 (64 x the mean module or narrow-run
 *                              width), flags (bit 0 GS1: FNC1 first; bit 1 FNC2, bit 2 FNC3, bit 3 FNC4), len, 0, 0, then 48 bytes of text, zero-filled; in
 *                              (y0, x0, dir) order
 *   ttr_result_item_barcode    [count]: the barcode an item's centre lies in, -1 for none
 * ttr_results_gather_barcodes: item_barcode of n results back to back (-1 where a result has none); returns the number of items inside a barcode.
 * ttr_barcodes_from_page: the rule on the host, no engine.  A host image u8 [h][w][3] (row_stride bytes, 0 = 3 w) and nq quads [nq][8] -> mode, counts [6] =
 * {barcodes, candidates examined, start patterns matched, hits kept, hits dropped, chains below min_lines}, barcodes [64][24] (capacity; counts[0] says how
 * much is valid), item_barcode [nq], and the lines' raw hits [(h + w) 2 8][20] and counters [(h + w) 2][4] as ttr_dbg_barcodes describes them; any output may
 * be NULL.  Returns 0, -1 with the message in ttr_last_error (a parameter outside its range, a quad with a coordinate that is not finite or has |x| >= 32768,
 * a page side of 32768 or more).  ttr_barcodes_from_page_ink: the same with local ink's (radius, drop, polarity) in the place of ink.
 * ttr_barcodes_page (stage; refuses while batches stream): the same through the kernels under the fixed ink rule, whatever the engine's setting. */
int ttr_engine_set_barcodes(ttr_engine* e, int min_lines, int ink, int symbologies);
int ttr_engine_barcodes(const ttr_engine* e, int* ink, int* symbologies);
int ttr_result_barcode_mode(const ttr_result* r);
int ttr_result_barcode_count(const ttr_result* r);
const int32_t* ttr_result_barcodes(const ttr_result* r);
const int32_t* ttr_result_item_barcode(const ttr_result* r);
int ttr_results_gather_barcodes(ttr_result* const* rs, int n, int32_t* item_barcode);
int ttr_barcodes_from_page(const uint8_t* img, int h, int w, int row_stride, int min_lines, int ink, int symbologies, const float* quads, int nq, int32_t* mode,
                           int32_t* counts, int32_t* barcodes, int32_t* item_barcode, int32_t* hits, int32_t* line_counts);
int ttr_barcodes_from_page_ink(const uint8_t* img, int h, int w, int row_stride, int min_lines, int symbologies, int radius, int drop, int polarity, const float* quads,
                               int nq, int32_t* mode, int32_t* counts, int32_t* barcodes, int32_t* item_barcode);
int ttr_barcodes_page(ttr_engine* e, const uint8_t* img, int h, int w, int row_stride, int min_lines, int ink, int symbologies, const float* quads, int nq, int32_t* mode,
                      int32_t* counts, int32_t* barcodes, int32_t* item_barcode);
/* Tokenizer::decode + EOS cut (tuatara.cpp:61-78, :497-502) on 26 ids; buf needs >= 27 bytes. */
int ttr_decode_ids(const int32_t* ids, int n, char* buf);

/* Per-engine kernel-selection knobs by name (they change fp32 summation order at most, never a rounding point; tests and
 * tools/ use them to compare kernel generations on the same engine): "mlp_fused" (0 off, 1 = from "mlp_min_rows" rows on (default),
 * 2 = always), "mlp_proj", "qkv_attn" (0 / 1 = from "qkv_attn_min" crops on / 2), "dec_mlp_fused" / "dec_mlp_min_rows" (refinement
 * pass through the fused block kernel), "ln_fuse", "tok_fuse" (decoder LayerNorms / token embedding inside the skinny GEMM),
 * "ar_early_exit" (AR steps return at once when every crop has emitted EOS), "decoder_mode" (0 = one kernel per op, 4 / 8 / 16 = the
 * fused persistent AR kernel, else automatic), "fuse_first" (CRAFT conv1_1 inside conv1_2's loader), "enc_chunk", "dbg_bf16_out".
 * Any other key is handed to the process-wide diagnostics setter of tuatara_hip_debug.h.  Returns 0, or -1 for an unknown key. */
int ttr_engine_set_tuning(ttr_engine* e, const char* key, int value);

/* ---- device memory helpers (so callers need no HIP bindings) -------------------------------- */
void* ttr_dev_alloc(size_t bytes);
void ttr_dev_free(void* p);
int ttr_dev_upload(void* dst, const void* src, size_t bytes);
int ttr_dev_download(void* dst, const void* src, size_t bytes);
int ttr_dev_sync(ttr_engine* e);
/* last batch: milliseconds spent in each stage on the GPU stream (hipEvents): {craft, post, pack, parseq} */
int ttr_last_stage_ms(ttr_engine* e, float ms[4]);
/* per-launch HIP-event timing of the conv / GEMM kernels, accumulated over calls while on (on = 1: the CRAFT convolution launches
 * only, ~100 events per 32-page step; on = 2: every launch, ~1400 events, which costs ~8 % of throughput):
 * index 0 = CRAFT convolutions, 1 = PARSeq encoder (ViT) and batched decoder GEMMs, 2 = the per-step AR decoder GEMMs.  flops = algorithmic 2*M*N*K of the unpadded layers. */
int ttr_set_profiling(ttr_engine* e, int on);
int ttr_get_profile(ttr_engine* e, double ms[3], double flops[3], long long launches[3]);
/* the same records by kernel kind, as JSON text written to buf (at most cap - 1 characters + terminator; returns the full length or -1):
 *   [{"kind": "conv3p_kernel<128,NP=3>", "stage": 0, "launches": n, "ms": t, "alg_flops": a, "exec_flops": x}, ...]
 * alg_flops = 2 x MACs of the layers (the figure a roofline is priced with), exec_flops = what the matrix cores execute for them (x 3 / x 4 in
 * the split-operand precision).  With on = 1 a record spans a run of consecutive launches of one kind (inter-kernel gaps included). */
int ttr_get_profile_kinds(ttr_engine* e, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TUATARA_HIP_H */
