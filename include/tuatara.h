// C++ drop-in for /root/reference/tuatara.h:8-13 on top of the C ABI (tuatara_hip.h).
//
//   struct OutputItem { std::string text; std::vector<float> bbox; };
//   std::vector<OutputItem> image_to_data(cv::Mat image, std::string weights_dir, std::string outputs_dir);
//
// The cv::Mat overload exists only when OpenCV headers are present (the reference's header
// includes them unconditionally, tuatara.h:3-4); the raw-pointer overload is always there and
// is what bindings/python.cpp uses.  Error convention as the reference: message on std::cerr
// and an empty vector (tuatara.cpp:315-323, :337-340, :344-347).  The engine is created on the
// first call for a weights_dir and cached (the reference reloads both models per call).
#ifndef TUATARA_H
#define TUATARA_H
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

struct OutputItem {
  std::string text;
  std::vector<float> bbox;  // x1, y1, x2, y2
};

// image: u8 HWC, 3 channels, `row_stride` bytes per row (0 = tightly packed).  Not modified.
std::vector<OutputItem> image_to_data(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                      std::string outputs_dir);

// The same over a list of images of any sizes: one entry of the result per image, in input order (what a caller of the reference writes as a loop over
// image_to_data; here the list shares one engine, same-sized images travel as batches and the host-to-device copies run beside the GPU's work).
// An error (see above) prints its message and returns an empty list.
struct ImageView { const uint8_t* data; int rows, cols; std::ptrdiff_t row_stride; };   // row_stride 0 = tightly packed
std::vector<std::vector<OutputItem>> images_to_data(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir);

// Rectified crops (opt-in; DESIGN.md "Rectified crops"): the same items as image_to_data - order, text boxes, failures - each with the
// word's quadrilateral; with rectify = true a tilted word is deskewed (up to 45 degrees) before the recogniser reads it, so `text` may
// differ from image_to_data's; with rectify = false the crops are image_to_data's.  OutputItem keeps the reference's layout.
// TUATARA_CROP_MODE=1 in the environment (beside TUATARA_STRICT_CROPS) makes image_to_data / images_to_data use rectified crops too.
// Every OutputItemEx also carries the recogniser's confidence: `conf` for the word and `char_conf` per character (ttr_result_conf / ttr_result_prob).
struct CharBox {                   // one character of an item's text (character boxes; DESIGN.md "Character boxes")
  std::string ch;                  // the character
  std::vector<float> quad;         // 8: tl, tr, br, bl in image pixels, along the word's baseline
  std::vector<float> bbox;         // 4: min x, min y, max x, max y of those corners
};
struct CharAlt {                   // one alternative of one character (character alternatives; DESIGN.md "Character alternatives")
  std::string ch;                  // the character
  float prob = 0.f;                // its softmax probability among the allowed characters
};
struct LexMatch {                  // one entry of the caller's word list matched against an item (lexicon matching; DESIGN.md "Lexicon matching")
  int index = -1;                  // the entry's index in the word list
  std::string word;                // the entry
  float logp = 0.f;                // its log-probability under the item's per-position distributions, the EOS behind it included
  int edits = 0;                   // fuzzy alignment: the dropped and extra characters of the entry's best alignment (0 when the mode is off)
};
struct WordPiece {                 // one piece of a wide word (wide words; DESIGN.md "Wide words")
  std::string text;                // the piece's reading
  float conf = 0.f;                // the recogniser's confidence in it
  std::vector<float> quad;         // 8: tl, tr, br, bl in image pixels
};
struct OutputItemEx {
  std::string text;
  std::vector<float> bbox;  // x1, y1, x2, y2
  std::vector<float> quad;  // tl.x, tl.y, tr.x, tr.y, br.x, br.y, bl.x, bl.y in image pixels; tl -> tr is the baseline
  float conf = 0.f;                // the recogniser's confidence in `text`, a probability in (0, 1] (DESIGN.md "Recognition confidence")
  std::vector<float> char_conf;    // one probability per character of `text`, in order (char_conf.size() == text.size())
  int orient = 0;                  // word orientation: the turn the word was read at, in degrees clockwise (0, 90, 180, 270; DESIGN.md "Word orientation")
  std::vector<CharBox> chars;      // character boxes: one per character of `text`, in text order; empty when chars are off (DESIGN.md "Character boxes")
  int line = -1, word = -1;        // text lines: the item's line of its page, in reading order, and its position inside that line; -1 when lines are off (DESIGN.md "Text lines")
  int region = -1;                 // regions: the index of the caller's region this item reads; -1 for items the detector found (DESIGN.md "Regions and per-row character sets")
  int alt_k = 0;                   // character alternatives: K per position, the winner included; 0 when alternatives are off (DESIGN.md "Character alternatives")
  std::vector<int32_t> alt_ids;    // [26][alt_k]: the K best classes of every position of the recogniser's row (-1 = none), as ttr_result_alt_ids gives them
  std::vector<float> alt_prob;     // [26][alt_k]: their probabilities, as ttr_result_alt_probs gives them
  std::vector<std::vector<CharAlt>> alternatives;   // one list per character of `text`: that position's character options in rank order, the character itself first unless another option ties it
  std::vector<LexMatch> lexicon;   // lexicon matching: the M best entries of the call's word list by (logp descending, index ascending); empty when no lexicon was given (DESIGN.md "Lexicon matching")
  bool has_pattern_logp = false;   // patterns in best mode: the call read under a pattern as the likeliest member of its language (DESIGN.md "Patterns") ...
  float pattern_logp = 0.f;        // ... and this is the log-probability of `text` under the recogniser's per-position distributions (-inf for an item without a pattern)
  std::vector<WordPiece> pieces;   // wide words: the item's pieces in order (one, the item itself, when it is not wide); empty when wide is off (DESIGN.md "Wide words")
  bool curved = false;             // curved words: the item's crop was straightened along a spine found in the page (DESIGN.md "Curved words")
  std::vector<float> outline;      // curved words: 36 = 18 points x, y - the top edge left to right, then the bottom edge right to left; empty when curved is off
  int barcode = -1;                // barcodes: the barcode of its page the item's centre lies in (a junk word the detector made of the bars); -1 for none and when barcodes are off (DESIGN.md "Barcodes")
  int mark = -1;                   // selection marks: the mark of its page the item's centre lies in (the `x` read inside a ticked box); -1 for none and when marks are off (DESIGN.md "Selection marks")
  int table = -1, cell = -1;       // tables: the table of its page and the cell of that page's cell list the item lies in; -1 / -1 in no cell and when tables are off (DESIGN.md "Tables")
  int block = -1, block_line = -1;  // text blocks: the item's block of its page, in reading order, and its line's position inside that block (what a caller sorts by: block, block_line, word); -1 when blocks are off (DESIGN.md "Text blocks")
};
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify);
// Word orientation (opt-in; DESIGN.md "Word orientation"): orient = TTR_ORIENT_FLIP (1) also reads every word turned by 180 degrees,
// TTR_ORIENT_QUARTER (2) by 90, 180 and 270; each item keeps the reading the recogniser is most sure of and says which in `orient`.
// orient_page = true: one turn per page, by a vote of its words.  orient = 0 is the calls above.  TUATARA_ORIENT=flip|quarter in the
// environment makes image_to_data / images_to_data / the calls above read orientations too (per word).  Items, order and boxes do not change.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page);
// Text lines (opt-in; DESIGN.md "Text lines"): lines = true also groups every page's words into lines in reading order; each item says its
// `line` and its `word` position in it (sort the items by (line, word) to read the page; join a line's words by ' ').  lines = false is the
// calls above, unless TUATARA_LINES=1 is set in the environment, which turns lines on for image_to_data / images_to_data / every call above.
// Items, order, boxes and text do not change.  In these two overloads orient = -1 leaves the orientation to TUATARA_ORIENT.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines);
// Character boxes (opt-in; DESIGN.md "Character boxes"): chars = true also gives every item one CharBox per character of its text, cut from the
// detector's region map along the word's baseline.  chars = false is the calls above, unless TUATARA_CHARS=1 is set in the environment, which
// turns them on for image_to_data / images_to_data / every call above.  Items, order, boxes and text do not change.  orient = -1 leaves the
// orientation to TUATARA_ORIENT, lines = false leaves the lines to TUATARA_LINES.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars);
// Text blocks (opt-in; DESIGN.md "Text blocks"): blocks = true also groups every page's text lines into blocks (paragraphs, column pieces) in
// reading order - a column is read to its end before the next begins; each item says its `block` and its line's position `block_line` in it (sort
// the items by (block, block_line, word) to read the page; put a blank line between blocks).  Blocks are made of lines: blocks = true turns lines on.
// blocks = false is the calls above, unless TUATARA_BLOCKS=1 is set in the environment, which turns blocks (and lines) on for image_to_data /
// images_to_data / every call above.  Items, order, boxes and text do not change.  orient = -1, lines = false and chars = false leave those to
// the environment.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks);
// Mixed-size batches (opt-in; DESIGN.md "Mixed-size batches"): the list form batches images of equal size; mixed_batches = true batches images that
// share one detector canvas instead, whatever their sizes - scans of one paper size that differ by a few pixels travel together.  Every result is
// the same either way.  mixed_batches = false is the call above, unless TUATARA_MIXED_BATCHES=1 is set in the environment, which turns it on for
// images_to_data and every images_to_data_ex.  The other arguments as above.
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches);
// Character sets (opt-in; DESIGN.md "Character sets"): allowlist = the characters the recogniser may emit ("" = all), blocklist = characters it may
// not ("" = none) - "this field holds digits", "never emit |".  The set acts where each character is chosen, so the rest of the word is read in its
// light, and conf / char_conf are probabilities over the allowed characters.  It is set on the cached engine for the call and reset afterwards.  A
// character the recogniser has no class for ('~', a blank, non-ASCII bytes), a set that leaves nothing, or a bf16 engine (TUATARA_PRECISION=bf16) with
// a restricting set: the message is printed and the result is empty.  Two empty strings are the calls above, unless TUATARA_ALLOWLIST /
// TUATARA_BLOCKLIST are set in the environment, which then apply to image_to_data / images_to_data / every call above; a non-empty argument
// takes precedence over its variable.  The other arguments as above.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist);

// Regions (DESIGN.md "Regions and per-row character sets"): read quadrilaterals the caller already knows - the fields of a form - with no detector, each
// under its own character set, in one recogniser pass.  A region is a quad tl, tr, br, bl in image pixels (pixel centres at integers, as OutputItemEx::quad
// gives it), or the pixel rectangle [x0, x1) x [y0, y1) through region_from_rect; allowlist / blocklist as above, both empty = the engine's own set
// (TUATARA_ALLOWLIST / TUATARA_BLOCKLIST, else every character).  One item per region, in the caller's order: `region` its index, `quad` the caller's floats,
// `bbox` the corners' extremes, text / conf / char_conf as above.  A bad region or list, or an engine with orientation, lines, character boxes or blocks
// turned on through the environment: the message is printed and the result is empty.
struct RegionSpec {
  std::vector<float> quad;          // 8: tl.x, tl.y, tr.x, tr.y, br.x, br.y, bl.x, bl.y
  std::string allowlist, blocklist;
  std::string pattern;              // the region's own pattern (below); empty = the call's own (TUATARA_PATTERN, else none)
};
RegionSpec region_from_rect(int x0, int y0, int x1, int y1, std::string allowlist = std::string(), std::string blocklist = std::string());
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions);

// Character alternatives (opt-in; DESIGN.md "Character alternatives"): alts = K in 2..8 also gives every item the K best characters of each position with
// their probabilities - what a spell-checker, a "did you mean" or a checksum repair needs beside `conf`.  `alternatives` holds one ranked list per character
// of `text`; nbest() reads the M likeliest whole words out of an item (substitutions only; reading 0 is (text, conf)).  K is set on the cached engine for the
// call and reset afterwards.  alts = 0 is the calls above, unless TUATARA_ALTS=K is set in the environment, which turns them on for every call.  Items,
// order, boxes, text and conf do not change.  Alternatives do not combine with word orientation or a bf16 engine: the message is printed and the result
// is empty.  The other arguments as above.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts);
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts);
// the message of this thread's last call above when it refused its character set or alternatives (it is printed too); empty when the call ran
std::string last_call_error();
struct WordReading { std::string text; float score = 0.f; };
std::vector<WordReading> nbest(const OutputItemEx& item, int m);   // the m best readings (1 <= m <= 64) of an item that carries alternatives; empty otherwise

// Lexicon matching (opt-in; DESIGN.md "Lexicon matching"): every item also gets `lexicon`, the m best entries (1..8) of `words` with their
// log-probabilities under the recogniser's per-position distributions - what matching against a catalogue, a list of names or a form's field values needs.
// Entries are 1..25 characters out of the recogniser's set, without ']' and the backslash; a bad entry prints the message naming its index and the result is
// empty (last_call_error()).  The list is set on the cached engine for the call and cleared afterwards.  Items, order, boxes, text and conf do not change.
// Like the alternatives it does not combine with word orientation or a bf16 engine.  alts = 0 leaves the alternatives off; the other arguments as above.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m);
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, const std::vector<std::string>& words, int m);
// ... with fuzzy alignment (DESIGN.md "Lexicon matching", Fuzzy alignment): band = 0..3 aligns every entry against the reading instead of indexing it, so an
// entry still matches a reading with up to `band` more dropped than extra characters (or the other way round) at any point; gap (finite, <= 0) is the
// log-probability charged for each, and LexMatch::edits says how many the best alignment took.  band = -1 is the calls above.  LexFuzzy{} is band 1 with
// gap = ln 1e-3, which nobody has tuned on documents.  The mode is set on the cached engine for the call and cleared afterwards.
struct LexFuzzy { int band = 1; float gap = -6.9077554f; };
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m, int band, float gap);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m,
                                                         int band, float gap);
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, const std::vector<std::string>& words, int m,
                                           int band, float gap);

// Patterns (opt-in; DESIGN.md "Patterns"): pattern = a regular expression every word must match - "\\d{2}/\\d{2}/\\d{4}" for a date, "[A-Z]{2}\\d{2,6}" for
// a plate; the syntax is the subset of Python's re that include/tuatara_hip.h lists.  The pattern acts where each character is chosen: every returned text is
// a member of its language, and conf / char_conf are probabilities over the choices it left open.  It is set on the cached engine for the call and reset
// afterwards.  An empty string is the call above, unless TUATARA_PATTERN is set in the environment, which then applies to every call here.  A bad pattern, a
// bf16 engine, or an engine with word orientation, alternatives or a lexicon turned on: the message is printed and the result is empty (last_call_error()).
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, std::string pattern);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, std::string pattern);
// ... in best mode: pattern_best = true reads every word as the LIKELIEST member of the pattern's language under the recogniser's refined per-position
// distributions, instead of the member a position-by-position walk reaches, and every item carries pattern_logp (has_pattern_logp set).  The mode is set on
// the cached engine for the call and reset afterwards, also when the call fails.  pattern_best = false is the calls above, unless TUATARA_PATTERN_BEST=1 is
// set in the environment, which turns the mode on for every call here that reads under a pattern.  It needs what a pattern needs.
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, std::string pattern, bool pattern_best);
std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, std::string pattern, bool pattern_best);
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, bool pattern_best);   // (each region under its own pattern)

// Wide words (opt-in; DESIGN.md "Wide words"): a word whose quad is wider than wide.max_aspect times its height - a URL, an IBAN, a serial number - is cut
// into pieces at the gaps between characters, every piece is read as a crop of its own in the same recogniser pass, and the readings are joined: `text` is
// the pieces' texts concatenated, `conf` the product of their conf, `pieces` lists them; char_conf covers the first piece.  Items, order, bbox and quad do not
// change, and a word that is not wide keeps every bit.  The call reads on rectified crops whatever `rectify` says (a piece is a crop of the word's quad).
// wide.max_aspect: a value in [2, 64]; Wide{} is 8, which nobody has tuned on documents.  It is set on the cached engine for the call and reset afterwards;
// TUATARA_WIDE=A (or 1 for the default) in the environment turns it - and with it rectified crops - on for every call here.  With orient or chars, or a value
// out of range: the message is printed and the result is empty (last_call_error()).
struct Wide { float max_aspect = 8.f; };
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, Wide wide);

// Curved words (opt-in; DESIGN.md "Curved words"): a word set on an arc - on a seal, a stamp, a logo - has its crop straightened along a spine found in the
// page's own pixels inside its quad; `curved` says so and `outline` traces the band that was read (for a word that is not curved, its quad's long sides).
// Items, order, bbox and quad do not change, and a word that is not curved keeps every bit.  The call reads on rectified crops whatever `rectify` says.  It
// is set on the cached engine for the call and reset afterwards; TUATARA_CURVED=1 in the environment turns it - and with it rectified crops - on for every call
// here.  With orient or chars: the message is printed and the result is empty (last_call_error()).
struct Curved {};
std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, Curved curved);

// Tiled pages (opt-in; DESIGN.md "Tiled pages"): a page larger than the detector canvas (1024 pixels on its longer side) is read at full size, as overlapping
// tiles whose heat maps are stitched into one page map, instead of being shrunk onto the canvas.  set_tiled(overlap) turns it on for every call of THIS THREAD
// that follows (a multiple of 32 in [64, 256]; 128 is the default of the other layers, which nobody has tuned on documents), set_tiled(0) off again; with it
// off, TUATARA_TILED=O (or 1 for 128) in the environment turns it on for every call here.  It is set on the cached engine for the call and reset afterwards.
// A bad value, a page side above 8192 or more than 64 tiles: the message is printed and the result is empty (last_call_error()).  A page that fits the
// canvas keeps every bit.
void set_tiled(int overlap);
int tiled();

// Tables (opt-in; DESIGN.md "Tables"): ruling lines are found in the page's own pixels, grouped into tables, each table's grid and merged cells derived, and
// every item given its table and cell (OutputItemEx::table, ::cell).  Items, order, boxes and text keep their bits.  set_tables(min_len, ink) turns it on for
// every call of THIS THREAD that follows (min_len 16..4096 px, the shortest ruling; ink 1..255; the other layers use 48 and 128, which nobody has tuned on
// documents), set_tables(0) off again; with it off, TUATARA_TABLES=MIN_LEN (or 1 for 48) in the environment turns it on for every call here.  It is set on the
// cached engine for the call and reset afterwards.  A bad value: the message is printed and the result is empty (last_call_error()).  last_call_tables(): the
// tables of this thread's latest single-image call - rows x cols strings, a merged cell's text at its first base cell, its items joined by the line rule.
struct TableGrid {
  int bbox[4] = {0, 0, 0, 0};       // x0, y0, x1, y1 in image pixels
  int rows = 0, cols = 0;
  std::vector<std::string> text;    // rows x cols, row-major
};
void set_tables(int min_len, int ink = 128);
int tables();
std::vector<TableGrid> last_call_tables();

// Selection marks (opt-in; DESIGN.md "Selection marks"): the page's checkboxes - small square frames - are found on the ink bitmap of the page's own pixels, each
// one's state read from the ink inside it, every item given the mark its centre lies in (OutputItemEx::mark) and every mark the item it stands in front of.
// Items, order, boxes and text keep their bits.  set_marks(min_side, max_side, fill, ink) turns it on for every call of THIS THREAD that follows (min_side 8..64
// and max_side min_side..128 px, fill 1..255 in 1/256ths of the interior, ink 1..255; the other layers use 10, 64, 24 and 128, which nobody has tuned on
// documents), set_marks(0) off again; with it off, TUATARA_MARKS=MIN_SIDE (or 1 for 10) in the environment turns it on for every call here.  It is set on the
// cached engine for the call and reset afterwards.  A bad value: the message is printed and the result is empty (last_call_error()).  last_call_marks(): the
// marks of this thread's latest single-image call, in (y, x) order; a page without words has marks too.
struct SelectionMark {
  int box[4] = {0, 0, 0, 0};        // x0, y0, x1, y1 of the frame in image pixels, inclusive (the upright page's under deskew)
  int interior[4] = {0, 0, 0, 0};   // the pixels inside the frame that were counted
  int inked = 0, area = 0;          // ink pixels of the interior, and its size
  bool selected = false;            // 256 inked >= fill area
  int label = -1;                   // the item the box stands in front of, -1 = none
  std::string text;                 // that item's text
};
void set_marks(int min_side, int max_side = 64, int fill = 24, int ink = 128);
int marks();
std::vector<SelectionMark> last_call_marks();

// Barcodes (opt-in; DESIGN.md "Barcodes"): the page's Code 128 and Code 39 barcodes are read off single lines of the ink bitmap of the page's own pixels, in all
// four directions, and every item is given the barcode its centre lies in (OutputItemEx::barcode), so that the junk words the detector makes of the bars can be
// dropped.  Items, order, boxes and text keep their bits.  set_barcodes(min_lines, ink, symbologies) turns it on for every call of THIS THREAD that follows
// (min_lines 4..256 scan lines that must agree, ink 1..255, symbologies bit 0 Code 128 and bit 1 Code 39; the other layers use 8, 128 and 3, which nobody has
// tuned on documents), set_barcodes(0) off again; with it off, TUATARA_BARCODES=MIN_LINES (or 1 for 8) in the environment turns it on for every call here.  It
// is set on the cached engine for the call and reset afterwards.  A bad value: the message is printed and the result is empty (last_call_error()).
// last_call_barcodes(): the barcodes of this thread's latest single-image call, in (y0, x0, direction) order; a page without words has barcodes too.
struct Barcode {
  int box[4] = {0, 0, 0, 0};        // x0, y0, x1, y1 in image pixels, inclusive (the upright page's under deskew)
  int symbology = 0;                // 1 = Code 128, 2 = Code 39
  int direction = 0;                // 0 left to right, 1 top to bottom, 2 right to left, 3 bottom to top
  int lines = 0;                    // the scan lines that agreed
  double module = 0.0;              // the mean module (Code 128) or narrow-run (Code 39) width in px
  int flags = 0;                    // bit 0 GS1 (FNC1 first), bit 1 FNC2, bit 2 FNC3, bit 3 FNC4
  bool gs1 = false;
  std::string data;                 // the text, at most 48 bytes (Code 128 may hold control characters)
};
void set_barcodes(int min_lines, int ink = 128, int symbologies = 3);
int barcodes();
std::vector<Barcode> last_call_barcodes();

// Deskew (opt-in; DESIGN.md "Deskew"): the page's skew is estimated on the GPU and a page found tilted is read upright; every box and quad of the result is then
// in the upright page's frame.  set_deskew(max_slope, gain, ink) turns it on for every call of THIS THREAD that follows (max_slope 1..128 px per 512 px, gain
// 256..65535 in 1/256ths, ink 1..255; the other layers use 64, 288 and 128, which nobody has tuned on documents), set_deskew(0) off again; with it off,
// TUATARA_DESKEW=MAX_SLOPE (or 1 for 64) in the environment turns it on for every call here.  It is set on the cached engine for the call and reset afterwards.
// A bad value: the message is printed and the result is empty (last_call_error()).  last_call_skew(): the record of this thread's latest single-image call
// (on = false when the layer was off); to_page maps a point of the result to the caller's image.
struct PageSkew {
  bool on = false;
  int slope = 0, found = 0, C = 65536, S = 0, w = 0, h = 0, mode = 0;
  double degrees = 0.0;              // atan(slope / 512)
  void to_page(float x, float y, float* xs, float* ys) const;   // (ttr_skew_to_page; the identity when the layer was off)
};
void set_deskew(int max_slope, int gain = 288, int ink = 128);
int deskew();
PageSkew last_call_skew();

// Local ink (opt-in; DESIGN.md "Local ink"): tables and deskew take their ink bitmap from an adaptive threshold - a pixel darker than its neighbourhood's mean -
// instead of the global one, so shaded, grey or inverted pages keep their rulings and their skew.  set_local_ink(radius, drop, polarity) turns it on for every
// call of THIS THREAD that follows (radius 1..64 px, drop 1..255 in 1/256ths, polarity 0 dark / 1 light / 2 auto; the defaults 16, 38 and 2 are untuned),
// set_local_ink(0) off again; with it off, TUATARA_LOCAL_INK=RADIUS (or 1 for 16) in the environment turns it on for every call here.  It is set on the cached
// engine for the call and reset afterwards; with neither tables nor deskew on nothing runs.  A bad value: the message is printed and the result is empty.
void set_local_ink(int radius, int drop = 38, int polarity = 2);
int local_ink();

#if defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
inline std::vector<OutputItem> image_to_data(cv::Mat image, std::string weights_dir, std::string outputs_dir) {
  if (image.empty() || image.type() != CV_8UC3) return image_to_data(nullptr, 0, 0, 0, weights_dir, outputs_dir);
  return image_to_data(image.data, image.rows, image.cols, (std::ptrdiff_t)image.step, weights_dir, outputs_dir);
}
inline std::vector<std::vector<OutputItem>> images_to_data(const std::vector<cv::Mat>& images, std::string weights_dir, std::string outputs_dir) {
  std::vector<ImageView> v;
  for (const cv::Mat& m : images) v.push_back(m.empty() || m.type() != CV_8UC3 ? ImageView{nullptr, 0, 0, 0} : ImageView{m.data, m.rows, m.cols, (std::ptrdiff_t)m.step});
  return images_to_data(v, weights_dir, outputs_dir);
}
#endif
#endif

#endif  // TUATARA_H
