// image_to_data (tuatara.h:13 / tuatara.cpp:314-512) as a thin C++ shim over the C ABI.
#include "../../include/tuatara.h"

#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>

#include "../../include/tuatara_hip.h"

namespace {
std::mutex g_mu;
std::map<std::string, ttr_engine*> g_engines;  // one engine per (weights_dir, precision); lives for the process

// crop_mode < 0: the process default (TUATARA_CROP_MODE, else TTR_CROP_BOUNDING); orient < 0: the process default (TUATARA_ORIENT=flip|quarter, else off);
// lines < 0: the process default (TUATARA_LINES=1, else off); chars < 0: the process default (TUATARA_CHARS=1, else off); blocks < 0: the process
// default (TUATARA_BLOCKS=1, else off).  Blocks are made of lines: with blocks on, lines are on.  mixed < 0: the process default
// (TUATARA_MIXED_BATCHES=1, else off)
ttr_engine* engine_for(const std::string& weights_dir, int crop_mode = -1, int orient = -1, int orient_page = 0, int lines = -1, int chars = -1, int blocks = -1,
                       int mixed = -1) {
  std::lock_guard<std::mutex> lk(g_mu);
  ttr_config cfg;
  ttr_config_default(&cfg);
  if (const char* p = std::getenv("TUATARA_CROP_MODE")) cfg.crop_mode = std::atoi(p);
  if (std::getenv("TUATARA_WIDE")) cfg.crop_mode = TTR_CROP_RECTIFIED;   // wide words read on rectified crops (DESIGN.md "Wide words")
  if (const char* p = std::getenv("TUATARA_CURVED")) if (std::string(p) == "1") cfg.crop_mode = TTR_CROP_RECTIFIED;   // so do curved words (DESIGN.md "Curved words")
  if (crop_mode >= 0) cfg.crop_mode = crop_mode;
  if (const char* p = std::getenv("TUATARA_ORIENT")) {
    const std::string v(p);
    cfg.orient = v == "flip" ? TTR_ORIENT_FLIP : v == "quarter" ? TTR_ORIENT_QUARTER : TTR_ORIENT_OFF;
  }
  if (orient >= 0) cfg.orient = orient;
  cfg.orient_page = orient_page;
  if (const char* p = std::getenv("TUATARA_LINES")) cfg.lines = std::string(p) == "1" ? 1 : 0;
  if (lines >= 0) cfg.lines = lines;
  if (const char* p = std::getenv("TUATARA_CHARS")) cfg.chars = std::string(p) == "1" ? 1 : 0;
  if (chars >= 0) cfg.chars = chars;
  if (const char* p = std::getenv("TUATARA_BLOCKS")) cfg.blocks = std::string(p) == "1" ? 1 : 0;
  if (blocks >= 0) cfg.blocks = blocks;
  if (cfg.blocks) cfg.lines = 1;
  if (const char* p = std::getenv("TUATARA_MIXED_BATCHES")) cfg.mixed_batches = std::string(p) == "1" ? 1 : 0;
  if (mixed >= 0) cfg.mixed_batches = mixed;
  if (const char* p = std::getenv("TUATARA_PRECISION")) {   // default: TTR_PREC_F16X4 (fp32-equivalent, the reference computes in fp32)
    const std::string v(p);
    cfg.precision = v == "f32" ? TTR_PREC_F32 : v == "bf16" ? TTR_PREC_BF16 : TTR_PREC_F16X4;
  }
  if (const char* p = std::getenv("TUATARA_STRICT_CROPS")) cfg.strict_crops = std::atoi(p);
  if (const char* p = std::getenv("TUATARA_DEVICE")) cfg.device = std::atoi(p);
  std::string key = weights_dir + "#" + std::to_string(cfg.precision) + "#" + std::to_string(cfg.device) + "#" + std::to_string(cfg.crop_mode) + "#" +
                    std::to_string(cfg.orient) + "#" + std::to_string(cfg.orient_page) + "#" + std::to_string(cfg.lines) + "#" + std::to_string(cfg.chars) + "#" +
                    std::to_string(cfg.blocks) + "#" + std::to_string(cfg.mixed_batches);
  auto it = g_engines.find(key);
  if (it != g_engines.end()) return it->second;
  ttr_engine* e = ttr_create(weights_dir.c_str(), &cfg);
  if (e) g_engines[key] = e;
  return e;
}

// A call's character set on the cached engine (DESIGN.md "Character sets"): set when the call begins, reset when it ends, also when it throws.  An empty
// argument falls back on TUATARA_ALLOWLIST / TUATARA_BLOCKLIST.  Calls that share an engine take turns, so that none runs under another's set.
std::map<ttr_engine*, std::unique_ptr<std::mutex>> g_call_mu;
thread_local std::string g_call_error;   // last_call_error()
thread_local int g_call_tiled = 0;       // set_tiled(): the overlap of this thread's calls, 0 = off (then TUATARA_TILED decides)
thread_local int g_call_tables = 0, g_call_tables_ink = 128;   // set_tables(): min_len and ink of this thread's calls, 0 = off (then TUATARA_TABLES decides)
thread_local std::vector<TableGrid> g_call_table_out;          // last_call_tables()
thread_local int g_call_marks = 0, g_call_marks_max = 64, g_call_marks_fill = 24, g_call_marks_ink = 128;   // set_marks(): this thread's calls, 0 = off (then TUATARA_MARKS decides)
thread_local std::vector<SelectionMark> g_call_mark_out;       // last_call_marks()
thread_local int g_call_barcodes = 0, g_call_barcodes_ink = 128, g_call_barcodes_sym = 3;   // set_barcodes(): this thread's calls, 0 = off (then TUATARA_BARCODES decides)
thread_local std::vector<Barcode> g_call_barcode_out;          // last_call_barcodes()
thread_local int g_call_ink = 0, g_call_ink_drop = 38, g_call_ink_polarity = 2;   // set_local_ink(): this thread's calls, 0 = off (then TUATARA_LOCAL_INK decides)
thread_local int g_call_deskew = 0, g_call_deskew_gain = 288, g_call_deskew_ink = 128;   // set_deskew(): this thread's calls, 0 = off (then TUATARA_DESKEW decides)
thread_local PageSkew g_call_skew_out;                         // last_call_skew()
struct CharsetScope {
  ttr_engine* e;
  std::unique_lock<std::mutex> turn;
  bool set = false, ok = true;
  bool alts_set = false, lex_set = false, pattern_set = false, wide_set = false, best_set = false, curved_set = false, fuzzy_set = false, tiled_set = false;
  bool tables_set = false;
  bool marks_set = false;
  bool barcodes_set = false;
  bool deskew_set = false;
  bool ink_set = false;
  CharsetScope(ttr_engine* e_, std::string allow, std::string deny, int alts = 0, const std::vector<std::string>* words = nullptr, int lex_m = 0,
               std::string pattern = std::string(), float wide = 0.f, bool pattern_best = false, bool curved = false, LexFuzzy fuzzy = LexFuzzy{-1, 0.f}) : e(e_) {
    {
      std::lock_guard<std::mutex> lk(g_mu);
      auto& m = g_call_mu[e];
      if (!m) m.reset(new std::mutex);
      turn = std::unique_lock<std::mutex>(*m, std::defer_lock);
    }
    turn.lock();
    g_call_error.clear();
    if (allow.empty()) if (const char* p = std::getenv("TUATARA_ALLOWLIST")) allow = p;
    if (deny.empty()) if (const char* p = std::getenv("TUATARA_BLOCKLIST")) deny = p;
    if (alts <= 0) if (const char* p = std::getenv("TUATARA_ALTS")) alts = std::atoi(p);
    if (alts > 0) {   // character alternatives (DESIGN.md "Character alternatives"): K for the call, like the set
      if (ttr_engine_set_alternatives(e, alts) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      alts_set = true;
    }
    if (words) {      // lexicon matching (DESIGN.md "Lexicon matching"): the word list for the call, like the set
      std::vector<const char*> ptr(words->size());
      for (size_t i = 0; i < words->size(); ++i) ptr[i] = (*words)[i].c_str();
      if (ttr_engine_set_lexicon(e, ptr.empty() ? nullptr : ptr.data(), (int)ptr.size(), lex_m) != 0 || ptr.empty()) {
        g_call_error = ptr.empty() ? "lexicon: the word list is empty" : ttr_last_error();
        std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return;
      }
      lex_set = true;
      if (fuzzy.band >= 0) {   // ... and its fuzzy alignment (DESIGN.md "Lexicon matching", Fuzzy alignment): the band and gap for the call, like the list
        if (ttr_engine_set_lexicon_fuzzy(e, fuzzy.band, fuzzy.gap) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
        fuzzy_set = true;
      }
    }
    if (wide == 0.f) if (const char* p = std::getenv("TUATARA_WIDE")) wide = std::string(p) == "1" ? 8.f : (float)std::atof(p);
    if (wide != 0.f) {   // wide words (DESIGN.md "Wide words"): the largest aspect of a piece for the call, like the set
      if (ttr_engine_set_wide(e, wide) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      wide_set = true;
    }
    int tiled = g_call_tiled;
    if (tiled == 0) if (const char* p = std::getenv("TUATARA_TILED")) tiled = std::string(p) == "1" ? 128 : std::atoi(p);
    if (tiled != 0) {   // tiled pages (DESIGN.md "Tiled pages"): the overlap for the call, like the set
      if (ttr_engine_set_tiled(e, tiled) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      tiled_set = true;
    }
    int tab = g_call_tables;
    if (tab == 0) if (const char* p = std::getenv("TUATARA_TABLES")) tab = std::string(p) == "1" ? 48 : std::atoi(p);
    g_call_table_out.clear();
    if (tab != 0) {   // tables (DESIGN.md "Tables"): min_len and ink for the call, like the set
      if (ttr_engine_set_tables(e, tab, g_call_tables_ink) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      tables_set = true;
    }
    int mk = g_call_marks;
    if (mk == 0) if (const char* p = std::getenv("TUATARA_MARKS")) mk = std::string(p) == "1" ? 10 : std::atoi(p);
    g_call_mark_out.clear();
    if (mk != 0) {   // selection marks (DESIGN.md "Selection marks"): the four parameters for the call, like the set
      if (ttr_engine_set_marks(e, mk, g_call_marks_max, g_call_marks_fill, g_call_marks_ink) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      marks_set = true;
    }
    int bc = g_call_barcodes;
    if (bc == 0) if (const char* p = std::getenv("TUATARA_BARCODES")) bc = std::string(p) == "1" ? 8 : std::atoi(p);
    g_call_barcode_out.clear();
    if (bc != 0) {   // barcodes (DESIGN.md "Barcodes"): the three parameters for the call, like the set
      if (ttr_engine_set_barcodes(e, bc, g_call_barcodes_ink, g_call_barcodes_sym) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      barcodes_set = true;
    }
    int dsk = g_call_deskew;
    if (dsk == 0) if (const char* p = std::getenv("TUATARA_DESKEW")) dsk = std::string(p) == "1" ? 64 : std::atoi(p);
    g_call_skew_out = PageSkew();
    if (dsk != 0) {   // deskew (DESIGN.md "Deskew"): max_slope, gain and ink for the call, like the set
      if (ttr_engine_set_deskew(e, dsk, g_call_deskew_gain, g_call_deskew_ink) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      deskew_set = true;
    }
    int link = g_call_ink;
    if (link == 0) if (const char* p = std::getenv("TUATARA_LOCAL_INK")) link = std::string(p) == "1" ? 16 : std::atoi(p);
    if (link != 0) {   // local ink (DESIGN.md "Local ink"): radius, drop and polarity for the call, like the set
      if (ttr_engine_set_ink(e, link, g_call_ink_drop, g_call_ink_polarity) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      ink_set = true;
    }
    if (!curved) if (const char* p = std::getenv("TUATARA_CURVED")) curved = std::string(p) == "1";
    if (curved) {   // curved words (DESIGN.md "Curved words"): on for the call, like the set
      if (ttr_engine_set_curved(e, 1) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      curved_set = true;
    }
    if (pattern.empty()) if (const char* p = std::getenv("TUATARA_PATTERN")) pattern = p;
    if (!allow.empty() || !deny.empty()) {
      if (ttr_engine_set_charset(e, allow.c_str(), deny.c_str()) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      set = true;
    }
    if (!pattern_best && !pattern.empty()) if (const char* p = std::getenv("TUATARA_PATTERN_BEST")) pattern_best = std::string(p) == "1";   // (the variable reaches only calls that read under a pattern)
    if (pattern_best) {       // the decode mode of patterns (DESIGN.md "Patterns"): the likeliest member, for the call; without a pattern it has no effect
      if (ttr_engine_set_pattern_decode(e, TTR_PATTERN_BEST) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      best_set = true;
    }
    if (!pattern.empty()) {   // the call's pattern (DESIGN.md "Patterns"): behind the set, under which it is compiled
      if (ttr_engine_set_pattern(e, pattern.c_str()) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: " << g_call_error << std::endl; ok = false; return; }
      pattern_set = true;
    }
  }
  ~CharsetScope() {
    if (pattern_set) ttr_engine_set_pattern(e, nullptr);
    if (best_set) ttr_engine_set_pattern_decode(e, TTR_PATTERN_GREEDY);
    if (wide_set) ttr_engine_set_wide(e, 0.f);
    if (curved_set) ttr_engine_set_curved(e, 0);
    if (tiled_set) ttr_engine_set_tiled(e, 0);
    if (tables_set) ttr_engine_set_tables(e, 0, 0);
    if (marks_set) ttr_engine_set_marks(e, 0, 0, 0, 0);
    if (barcodes_set) ttr_engine_set_barcodes(e, 0, 0, 0);
    if (deskew_set) ttr_engine_set_deskew(e, 0, 0, 0);
    if (ink_set) ttr_engine_set_ink(e, 0, 0, 0);
    if (set) ttr_engine_set_charset(e, nullptr, nullptr);
    if (alts_set) ttr_engine_set_alternatives(e, 0);
    if (fuzzy_set) ttr_engine_set_lexicon_fuzzy(e, -1, 0.f);
    if (lex_set) ttr_engine_set_lexicon(e, nullptr, 0, 0);
  }
};

// lexicon matching: the matches' words, read from the engine while the call's list is still set on it (fill() leaves them empty)
inline void name_matches(ttr_engine*, OutputItem&) {}
inline void name_matches(ttr_engine* e, OutputItemEx& o) {
  for (LexMatch& m : o.lexicon) if (const char* w = ttr_engine_lexicon_word(e, m.index)) m.word = w;
}

template <class Item>
void fill(Item& o, const ttr_result* r, int i) {   // text and bbox: OutputItem, and the start of OutputItemEx
  o.text = ttr_result_text(r, i);
  const float* b = ttr_result_bbox(r, i);
  o.bbox.assign(b, b + 4);
}
void fill(OutputItemEx& o, const ttr_result* r, int i) {
  fill<OutputItemEx>(o, r, i);
  const float* q = ttr_result_quad(r, i);
  o.quad.assign(q, q + 8);
  o.conf = ttr_result_conf(r, i);
  float cc[26];
  int nc = 0;
  ttr_confidence_from_probs(ttr_result_ids(r, i), ttr_result_prob(r, i), 26, cc, &nc, nullptr);
  o.char_conf.assign(cc, cc + nc);
  o.orient = 90 * ttr_result_orient(r, i);
  o.region = ttr_result_sets(r) ? i : -1;   // (a region call returns one page's regions in the caller's order)
  const int32_t *ln = ttr_result_lines(r), *wd = ttr_result_words(r);
  o.line = ln ? ln[i] : -1;
  o.word = wd ? wd[i] : -1;
  const int32_t *bk = ttr_result_blocks(r), *lp = ttr_result_line_pos(r);
  o.block = bk ? bk[i] : -1;
  o.block_line = bk && lp && ln ? lp[ln[i]] : -1;
  o.alt_k = ttr_result_alt_k(r);
  o.alt_ids.clear(); o.alt_prob.clear(); o.alternatives.clear();
  if (o.alt_k > 0 && ttr_result_alt_ids_all(r)) {
    const int K = o.alt_k;
    const int32_t* ai = ttr_result_alt_ids(r, i);
    const float* ap = ttr_result_alt_probs(r, i);
    o.alt_ids.assign(ai, ai + 26 * K);
    o.alt_prob.assign(ap, ap + 26 * K);
    auto is_char = [](int id) { return id >= 1 && id < 95 && id != 88; };
    for (int p = 0; p < 26 && ai[p * K] != 0; ++p) {   // the positions of the text's characters (the confidence rule's S)
      if (!is_char(ai[p * K])) continue;
      std::vector<int> slots;
      for (int j = 0; j < K; ++j) if (is_char(ai[p * K + j])) slots.push_back(j);
      std::stable_sort(slots.begin(), slots.end(), [&](int a, int b) { return ap[p * K + a] > ap[p * K + b]; });
      std::vector<CharAlt> alts;
      for (int j : slots) {
        char buf[32];
        ttr_decode_ids(&ai[p * K + j], 1, buf);
        CharAlt a;
        a.ch = buf; a.prob = ap[p * K + j];
        alts.push_back(std::move(a));
      }
      o.alternatives.push_back(std::move(alts));
    }
  }
  o.lexicon.clear();
  if (const int32_t* li = ttr_result_lex_idx(r, i)) {
    const float* ll = ttr_result_lex_logp(r, i);
    const int32_t* le = ttr_result_lex_edits(r, i);   // fuzzy alignment: null when the mode is off
    for (int j = 0, M = ttr_result_lex_m(r); j < M && li[j] >= 0; ++j) {
      LexMatch mt;
      mt.index = li[j]; mt.logp = ll[j]; mt.edits = le ? le[j] : 0;
      o.lexicon.push_back(std::move(mt));
    }
  }
  o.has_pattern_logp = false; o.pattern_logp = 0.f;
  if (const float* pl = ttr_result_pattern_logp(r)) { o.has_pattern_logp = true; o.pattern_logp = pl[i]; }
  o.pieces.clear();
  if (const int32_t* pf = ttr_result_piece_first(r)) {
    const int32_t* pi = ttr_result_piece_ids(r);
    const float *pc = ttr_result_piece_confs(r), *pq = ttr_result_piece_quads(r);
    for (int32_t k = pf[i]; k < pf[i + 1]; ++k) {
      WordPiece p;
      char buf[32];
      ttr_decode_ids(pi + 26 * (size_t)k, 26, buf);
      p.text = buf; p.conf = pc[k];
      p.quad.assign(pq + 8 * (size_t)k, pq + 8 * (size_t)k + 8);
      o.pieces.push_back(std::move(p));
    }
  }
  const int32_t *it = ttr_result_item_table(r), *ic = ttr_result_item_cell(r);
  o.table = it ? it[i] : -1;
  o.cell = ic ? ic[i] : -1;
  const int32_t* im = ttr_result_item_mark(r);
  o.mark = im ? im[i] : -1;
  const int32_t* ib = ttr_result_item_barcode(r);
  o.barcode = ib ? ib[i] : -1;
  o.curved = false; o.outline.clear();
  if (const int32_t* cv = ttr_result_curved(r)) {
    const float* ol = ttr_result_outlines(r);
    o.curved = cv[i] != 0;
    o.outline.assign(ol + 36 * (size_t)i, ol + 36 * (size_t)i + 36);
  }
  o.chars.clear();
  if (const int32_t* cf = ttr_result_char_first(r)) {
    const float *cq = ttr_result_char_quads(r), *cb = ttr_result_char_bboxes(r);
    for (int32_t k = cf[i]; k < cf[i + 1]; ++k) {
      CharBox c;
      const size_t j = (size_t)(k - cf[i]);
      if (j < o.text.size()) c.ch = o.text.substr(j, 1);
      c.quad.assign(cq + 8 * (size_t)k, cq + 8 * (size_t)k + 8);
      c.bbox.assign(cb + 4 * (size_t)k, cb + 4 * (size_t)k + 4);
      o.chars.push_back(std::move(c));
    }
  }
}

// the checks in front of both calls, then the cached engine; null once the reference's message is printed
ttr_engine* open_engine(const std::string& weights_dir, const std::string& outputs_dir, int crop_mode, int orient, int orient_page, int lines, int chars,
                        int blocks, int mixed = -1) {
  if (weights_dir.empty()) { std::cerr << "Please provide a value for weights_dir" << std::endl; return nullptr; }   // tuatara.cpp:315-318
  if (outputs_dir.empty()) { std::cerr << "Please provide a value for outputs_dir" << std::endl; return nullptr; }   // tuatara.cpp:320-323 (never used afterwards, there or here)
  ttr_engine* e = engine_for(weights_dir, crop_mode, orient, orient_page, lines, chars, blocks, mixed);
  if (!e) std::cerr << "error loading craft/parseq model: " << ttr_last_error() << std::endl;                       // tuatara.cpp:337-340, :429-432
  return e;
}

template <class Item>
std::vector<Item> run_one(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, const std::string& weights_dir,
                          const std::string& outputs_dir, int crop_mode, int orient = -1, int orient_page = 0, int lines = -1, int chars = -1,
                                        int blocks = -1, const std::string& allow = std::string(), const std::string& deny = std::string(), int alts = 0,
                                        const std::vector<std::string>* words = nullptr, int lex_m = 0, const std::string& pattern = std::string(), float wide = 0.f,
                                        bool pattern_best = false, bool curved = false, LexFuzzy fuzzy = LexFuzzy{-1, 0.f}) {
  ttr_engine* e = open_engine(weights_dir, outputs_dir, crop_mode, orient, orient_page, lines, chars, blocks);
  if (!e) return {};
  CharsetScope cs(e, allow, deny, alts, words, lex_m, pattern, wide, pattern_best, curved, fuzzy);
  if (!cs.ok) return {};
  if (!image || rows <= 0 || cols <= 0) {  // tuatara.cpp:344-347
    std::cerr << "Error reading image from file";
    return {};
  }
  ttr_result* r = nullptr;
  if (ttr_image_to_data(e, image, rows, cols, row_stride ? (int)row_stride : cols * 3, &r) != 0) {
    std::cerr << "tuatara: " << ttr_last_error() << std::endl;
    if (cs.tiled_set) g_call_error = ttr_last_error();   // tiled pages: a page the tile plan refuses (DESIGN.md "Tiled pages") - the caller can tell it from an empty page
    return {};
  }
  std::vector<Item> out(ttr_result_count(r));
  for (size_t i = 0; i < out.size(); ++i) { fill(out[i], r, (int)i); name_matches(e, out[i]); }
  {   // deskew: the page's record (last_call_skew())
    ttr_skew sk;
    if (ttr_result_skew(r, &sk)) {
      PageSkew& o = g_call_skew_out;
      o.on = true; o.slope = sk.slope; o.found = sk.found; o.C = sk.C; o.S = sk.S; o.w = sk.w; o.h = sk.h; o.mode = sk.mode;
      o.degrees = std::atan((double)sk.slope / 512.0) * 180.0 / 3.14159265358979323846;
    }
  }
  if (const int32_t* mk = ttr_result_marks(r)) {    // selection marks: every mark of the page (last_call_marks())
    for (int m = 0; m < ttr_result_mark_count(r); ++m) {
      const int32_t* q = mk + 12 * (size_t)m;
      SelectionMark s;
      for (int k = 0; k < 4; ++k) { s.box[k] = q[k]; s.interior[k] = q[4 + k]; }
      s.inked = q[8]; s.area = q[9]; s.selected = q[10] != 0; s.label = q[11];
      if (s.label >= 0 && (size_t)s.label < out.size()) s.text = out[(size_t)s.label].text;
      g_call_mark_out.push_back(std::move(s));
    }
  }
  if (const int32_t* bc = ttr_result_barcodes(r)) {   // barcodes: every barcode of the page (last_call_barcodes())
    for (int m = 0; m < ttr_result_barcode_count(r); ++m) {
      const int32_t* q = bc + 24 * (size_t)m;
      Barcode b;
      for (int k = 0; k < 4; ++k) b.box[k] = q[k];
      b.symbology = q[4]; b.direction = q[5]; b.lines = q[6]; b.module = (double)q[7] / 64.0; b.flags = q[8]; b.gs1 = (q[8] & 1) != 0;
      b.data.assign(reinterpret_cast<const char*>(q + 12), (size_t)q[9]);
      g_call_barcode_out.push_back(std::move(b));
    }
  }
  if (const int32_t* tb = ttr_result_tables(r)) {   // tables: every table as rows x cols strings (last_call_tables())
    const int32_t* cl = ttr_result_cells(r);
    for (int t = 0; t < ttr_result_table_count(r); ++t) {
      TableGrid g;
      for (int k = 0; k < 4; ++k) g.bbox[k] = tb[8 * t + k];
      g.rows = tb[8 * t + 4]; g.cols = tb[8 * t + 5];
      g.text.assign((size_t)g.rows * g.cols, std::string());
      for (int c = tb[8 * t + 6]; c < tb[8 * t + 6] + tb[8 * t + 7]; ++c) {
        const int need = ttr_result_cell_text(r, c, nullptr, 0);
        if (need <= 0) continue;
        std::string s((size_t)need + 1, '\0');
        ttr_result_cell_text(r, c, &s[0], need + 1);
        s.resize((size_t)need);
        g.text[(size_t)cl[9 * c + 1] * g.cols + cl[9 * c + 2]] = std::move(s);
      }
      g_call_table_out.push_back(std::move(g));
    }
  }
  ttr_result_free(r);
  return out;
}

template <class Item>
std::vector<std::vector<Item>> run_many(const std::vector<ImageView>& images, const std::string& weights_dir, const std::string& outputs_dir, int crop_mode,
                                        int orient = -1, int orient_page = 0, int lines = -1, int chars = -1,
                                        int blocks = -1, int mixed = -1, const std::string& allow = std::string(), const std::string& deny = std::string(), int alts = 0,
                                        const std::vector<std::string>* words = nullptr, int lex_m = 0, const std::string& pattern = std::string(), bool pattern_best = false,
                                        LexFuzzy fuzzy = LexFuzzy{-1, 0.f}) {
  ttr_engine* e = open_engine(weights_dir, outputs_dir, crop_mode, orient, orient_page, lines, chars, blocks, mixed);
  if (!e) return {};
  CharsetScope cs(e, allow, deny, alts, words, lex_m, pattern, 0.f, pattern_best, false, fuzzy);
  if (!cs.ok) return {};
  const int n = (int)images.size();
  std::vector<const uint8_t*> ptr(n);
  std::vector<int> hs(n), ws(n), st(n);
  for (int i = 0; i < n; ++i) {
    // (an unreadable entry - tuatara.cpp:344-347 - yields an empty list for that image alone: the engine prints the reference's message)
    ptr[i] = images[i].data; hs[i] = images[i].rows; ws[i] = images[i].cols;
    st[i] = images[i].row_stride ? (int)images[i].row_stride : images[i].cols * 3;
  }
  std::vector<ttr_result*> rs(n, nullptr);
  const int rc = n ? ttr_images_to_data(e, ptr.data(), hs.data(), ws.data(), st.data(), n, rs.data()) : 0;
  if (rc < 0) {   // the call could not run at all
    std::cerr << "tuatara: " << ttr_last_error() << std::endl;
    return {};
  }
  if (rc > 0) std::cerr << "tuatara: " << ttr_last_error() << std::endl;   // some images failed: theirs stay empty, the rest are returned (a loop over image_to_data)
  std::vector<std::vector<Item>> out(n);
  for (int i = 0; i < n; ++i) {
    out[i].resize(ttr_result_count(rs[i]));
    for (size_t k = 0; k < out[i].size(); ++k) { fill(out[i][k], rs[i], (int)k); name_matches(e, out[i][k]); }
    ttr_result_free(rs[i]);
  }
  return out;
}
}  // namespace

std::vector<OutputItem> image_to_data(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                      std::string outputs_dir) {
  return run_one<OutputItem>(image, rows, cols, row_stride, weights_dir, outputs_dir, -1);
}

std::vector<std::vector<OutputItem>> images_to_data(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir) {
  return run_many<OutputItem>(images, weights_dir, outputs_dir, -1);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist);
}

RegionSpec region_from_rect(int x0, int y0, int x1, int y1, std::string allowlist, std::string blocklist) {
  RegionSpec r;
  r.quad.assign(8, 0.f);
  if (ttr_region_from_rect(x0, y0, x1, y1, r.quad.data()) != 0) { std::cerr << "tuatara: " << ttr_last_error() << std::endl; r.quad.clear(); }
  r.allowlist = std::move(allowlist); r.blocklist = std::move(blocklist);
  return r;
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions) {
  return image_to_data_ex(image, rows, cols, row_stride, weights_dir, outputs_dir, regions, 0);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, alts);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist, alts);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, alts, &words, m);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist, alts, &words, m);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m, int band, float gap) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, alts, &words, m, std::string(), 0.f, false, false, LexFuzzy{band, gap});
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, int alts, const std::vector<std::string>& words, int m,
                                                         int band, float gap) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist, alts, &words, m, std::string(), false, LexFuzzy{band, gap});
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, std::string pattern) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, pattern);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, std::string pattern) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, pattern);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, std::string pattern, bool pattern_best) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, pattern, 0.f, pattern_best);
}

std::vector<std::vector<OutputItemEx>> images_to_data_ex(const std::vector<ImageView>& images, std::string weights_dir, std::string outputs_dir,
                                                         bool rectify, int orient, bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches,
                                                         std::string allowlist, std::string blocklist, std::string pattern, bool pattern_best) {
  return run_many<OutputItemEx>(images, weights_dir, outputs_dir, rectify ? TTR_CROP_RECTIFIED : -1, orient, orient_page ? 1 : 0, lines ? 1 : -1, chars ? 1 : -1,
                                blocks ? 1 : -1, mixed_batches ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, pattern, pattern_best);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool /*rectify*/, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, Wide wide) {
  if (!(wide.max_aspect >= 2.f && wide.max_aspect <= 64.f)) {   // (before an engine is opened; 0 would read as "off")
    g_call_error = "wide: max_aspect must be a finite value in [2, 64]";
    std::cerr << "tuatara: " << g_call_error << std::endl;
    return {};
  }
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, TTR_CROP_RECTIFIED, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, std::string(), wide.max_aspect);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, bool /*rectify*/, int orient, bool orient_page, bool lines, bool chars, bool blocks,
                                           std::string allowlist, std::string blocklist, Curved) {
  return run_one<OutputItemEx>(image, rows, cols, row_stride, weights_dir, outputs_dir, TTR_CROP_RECTIFIED, orient, orient_page ? 1 : 0, lines ? 1 : -1,
                               chars ? 1 : -1, blocks ? 1 : -1, allowlist, blocklist, 0, nullptr, 0, std::string(), 0.f, false, true);
}

std::string last_call_error() { return g_call_error; }

void set_tiled(int overlap) { g_call_tiled = overlap; }
int tiled() { return g_call_tiled; }
void set_marks(int min_side, int max_side, int fill, int ink) { g_call_marks = min_side; g_call_marks_max = max_side; g_call_marks_fill = fill; g_call_marks_ink = ink; }
int marks() { return g_call_marks; }
std::vector<SelectionMark> last_call_marks() { return g_call_mark_out; }
void set_barcodes(int min_lines, int ink, int symbologies) { g_call_barcodes = min_lines; g_call_barcodes_ink = ink; g_call_barcodes_sym = symbologies; }
int barcodes() { return g_call_barcodes; }
std::vector<Barcode> last_call_barcodes() { return g_call_barcode_out; }
void set_tables(int min_len, int ink) { g_call_tables = min_len; g_call_tables_ink = ink; }
int tables() { return g_call_tables; }
std::vector<TableGrid> last_call_tables() { return g_call_table_out; }
void set_deskew(int max_slope, int gain, int ink) { g_call_deskew = max_slope; g_call_deskew_gain = gain; g_call_deskew_ink = ink; }
int deskew() { return g_call_deskew; }
void set_local_ink(int radius, int drop, int polarity) { g_call_ink = radius; g_call_ink_drop = drop; g_call_ink_polarity = polarity; }
int local_ink() { return g_call_ink; }
PageSkew last_call_skew() { return g_call_skew_out; }
void PageSkew::to_page(float x, float y, float* xs, float* ys) const {
  const float in[2] = {x, y};
  float out[2] = {x, y};
  if (on) { ttr_skew sk{}; sk.slope = slope; sk.found = found; sk.C = C; sk.S = S; sk.w = w; sk.h = h; sk.mode = mode; ttr_skew_to_page(&sk, in, 1, out); }
  *xs = out[0]; *ys = out[1];
}

std::vector<WordReading> nbest(const OutputItemEx& item, int m) {
  std::vector<WordReading> out;
  if (item.alt_k < 2 || item.alt_ids.size() != (size_t)26 * item.alt_k || item.alt_prob.size() != item.alt_ids.size() || m < 1 || m > 64) return out;
  size_t need = 0;
  std::vector<float> scores((size_t)m, 0.f);
  const int n = ttr_nbest_from_alts(item.alt_ids.data(), item.alt_prob.data(), item.alt_k, m, nullptr, 0, nullptr, &need);
  if (n <= 0) return out;
  std::string buf(need, '\0');
  ttr_nbest_from_alts(item.alt_ids.data(), item.alt_prob.data(), item.alt_k, m, &buf[0], need, scores.data(), nullptr);
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    const size_t nl = buf.find('\n', at);
    WordReading w;
    w.text = buf.substr(at, nl - at); w.score = scores[(size_t)i];
    out.push_back(std::move(w));
    at = nl + 1;
  }
  return out;
}

namespace {
std::vector<OutputItemEx> read_regions(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, const std::string& weights_dir,
                                       const std::string& outputs_dir, const std::vector<RegionSpec>& regions, int alts, const std::vector<std::string>* words, int lex_m,
                                       bool pattern_best = false, LexFuzzy fuzzy = LexFuzzy{-1, 0.f}) {
  // every list and quad is checked on the host before an engine is opened
  std::vector<ttr_region> regs(regions.size());
  std::vector<uint32_t> sets;
  std::vector<const char*> pats;            // the regions' own patterns (DESIGN.md "Patterns"), each once
  std::vector<int32_t> pattern_of(regions.size(), -1);
  for (size_t i = 0; i < regions.size(); ++i) {
    const RegionSpec& s = regions[i];
    if (!s.pattern.empty()) {
      ttr_pattern* cp = nullptr;              // (checked on the host, under every class: a pattern that only its region's set empties is refused by the call)
      if (ttr_pattern_compile(s.pattern.c_str(), nullptr, &cp) != 0) { g_call_error = ttr_last_error(); std::cerr << "tuatara: region " << i << ": " << g_call_error << std::endl; return {}; }
      ttr_pattern_free(cp);
      size_t k = 0;
      while (k < pats.size() && s.pattern != pats[k]) ++k;
      if (k == pats.size()) pats.push_back(s.pattern.c_str());
      pattern_of[i] = (int32_t)k;
    }
    if (s.quad.size() != 8) { std::cerr << "tuatara: region " << i << ": a region is 8 floats (tl, tr, br, bl)" << std::endl; return {}; }
    for (int k = 0; k < 8; ++k) regs[i].quad[k] = s.quad[k];
    regs[i].page = 0; regs[i].set = -1;
    if (s.allowlist.empty() && s.blocklist.empty()) continue;
    uint32_t m[3];
    if (ttr_charset_mask(s.allowlist.c_str(), s.blocklist.c_str(), m) < 0) { std::cerr << "tuatara: region " << i << ": " << ttr_last_error() << std::endl; return {}; }
    regs[i].set = (int32_t)(sets.size() / 3);
    sets.insert(sets.end(), m, m + 3);
  }
  ttr_engine* e = open_engine(weights_dir, outputs_dir, -1, -1, 0, -1, -1, -1);
  if (!e) return {};
  if (!pattern_best && !pats.empty()) if (const char* p = std::getenv("TUATARA_PATTERN_BEST")) pattern_best = std::string(p) == "1";   // (regions with patterns of their own)
  CharsetScope cs(e, std::string(), std::string(), alts, words, lex_m, std::string(), 0.f, pattern_best, false, fuzzy);   // (the engine's own set for regions without lists: TUATARA_ALLOWLIST / TUATARA_BLOCKLIST; calls that share the engine take turns)
  if (!cs.ok) return {};
  if (!image || rows <= 0 || cols <= 0) {  // tuatara.cpp:344-347
    std::cerr << "Error reading image from file";
    return {};
  }
  ttr_result* r = nullptr;
  if (ttr_image_regions_to_data_p(e, image, rows, cols, row_stride ? (int)row_stride : cols * 3, regs.data(), (int)regs.size(), sets.empty() ? nullptr : sets.data(),
                                  (int)(sets.size() / 3), pats.empty() ? nullptr : pats.data(), (int)pats.size(), pats.empty() ? nullptr : pattern_of.data(), &r) != 0) {
    g_call_error = ttr_last_error();
    std::cerr << "tuatara: " << g_call_error << std::endl;
    return {};
  }
  std::vector<OutputItemEx> out(ttr_result_count(r));
  for (size_t i = 0; i < out.size(); ++i) { fill(out[i], r, (int)i); name_matches(e, out[i]); }
  ttr_result_free(r);
  return out;
}
}  // namespace

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts) {
  return read_regions(image, rows, cols, row_stride, weights_dir, outputs_dir, regions, alts, nullptr, 0);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, bool pattern_best) {
  return read_regions(image, rows, cols, row_stride, weights_dir, outputs_dir, regions, alts, nullptr, 0, pattern_best);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, const std::vector<std::string>& words, int m) {
  return read_regions(image, rows, cols, row_stride, weights_dir, outputs_dir, regions, alts, &words, m);
}

std::vector<OutputItemEx> image_to_data_ex(const uint8_t* image, int rows, int cols, std::ptrdiff_t row_stride, std::string weights_dir,
                                           std::string outputs_dir, const std::vector<RegionSpec>& regions, int alts, const std::vector<std::string>& words, int m,
                                           int band, float gap) {
  return read_regions(image, rows, cols, row_stride, weights_dir, outputs_dir, regions, alts, &words, m, false, LexFuzzy{band, gap});
}
