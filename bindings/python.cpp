// pybind11 module `pytuatara` — same surface as /root/reference/bindings/python.cpp:43-58:
//   pytuatara.image_to_data(image, weights_dir, outputs_dir) -> list[{"text": str, "bbox": [x1,y1,x2,y2]}]
// plus a keyword-only rectify=False on both calls: rectify=True reads tilted words on deskewed crops (DESIGN.md "Rectified crops") and
// every dict gains "quad": [[x, y] x 4] (tl, tr, br, bl); engines are cached per (weights_dir, rectify).  And a keyword-only conf=False:
// conf=True adds "conf" (the word's confidence, a probability in (0, 1]) and "char_conf" (one probability per character of "text";
// DESIGN.md "Recognition confidence"); it combines with rectify.  And keyword-only orient=None|"flip"|"quarter" and orient_page=False: every
// word is also read turned (by 180 degrees, or by 90, 180 and 270), keeps the reading the recogniser is most sure of, and its dict gains
// "orient" (degrees clockwise; DESIGN.md "Word orientation"); orient_page=True decides once per page.  They combine with rectify and conf;
// engines are cached per (weights_dir, rectify, orient, orient_page, lines).  And a keyword-only lines=False: lines=True groups each page's
// words into text lines in reading order and every dict gains "line" (its line of the page) and "word" (its position in that line; DESIGN.md
// "Text lines"); sort by (line, word) to read the page.  And a keyword-only chars=False: chars=True gives every dict "chars", a list of
// {"char", "quad", "bbox"} with one entry per character of "text" (DESIGN.md "Character boxes").  And a keyword-only blocks=False: blocks=True
// groups each page's text lines into blocks in reading order, a column read to its end before the next (DESIGN.md "Text blocks"); it turns lines
// on, and every dict gains "block" beside "line" and "word".  With all of them off every dict is the reference's {text, bbox}.
// And keyword-only allowlist=None, blocklist=None: the characters the recogniser may / may not emit (DESIGN.md "Character sets"), set on the cached
// engine for the call and reset afterwards, also when the call raises.  A character the recogniser has no class for ('~', a blank, non-ASCII) or a
// set that leaves nothing raises ValueError, naming the character, before anything runs.  The dicts' keys do not change.
// And a keyword-only regions=None on image_to_data: a list of dicts {"quad": 8 floats (or 4 pairs) tl, tr, br, bl | "rect": (x0, y0, x1, y1), optional
// "allowlist" / "blocklist"} reads those regions with no detector, each under its own character set, in one recogniser pass (DESIGN.md "Regions and
// per-row character sets"); a region without lists reads under the call's allowlist / blocklist.  One dict per region, in order: "text", "bbox", "quad" (the
// caller's floats), "region" (its index) and - conf=True - "conf" / "char_conf".  A bad list raises ValueError before anything runs.
// And a keyword-only alts=0 on both calls: alts=K (2..8) gives every dict "alternatives", one list per character of "text" holding (char, prob) tuples
// over that position's K best characters in rank order (DESIGN.md "Character alternatives"); set on the cached engine for the call and reset afterwards.
// It combines with everything above except orient, which raises the engine's message.
// And keyword-only lexicon=None, lexicon_m=1 on both calls: lexicon=[words] gives every dict "lexicon", [(word, prob), ...] over the lexicon_m (1..8) best
// entries of the list for that item, prob = exp(log-probability) in double (DESIGN.md "Lexicon matching"); set on the cached engine for the call and cleared
// afterwards.  A bad entry raises ValueError naming its index (the engine's own message; nothing is read).  It combines with everything above except orient.
// And a keyword-only pattern=None on both calls: a regular expression every word must match (DESIGN.md "Patterns"; the subset of Python's re that
// include/tuatara_hip.h lists), set on the cached engine for the call and reset afterwards, also when the call raises; calls that share the engine take turns.
// "pattern" is also a key of a regions= dict: that region's own.  A bad pattern raises ValueError, naming the offset or the character, before anything runs;
// And keyword-only lexicon_fuzzy=None, lexicon_gap=-6.9077554 (ln 1e-3) on both calls: lexicon_fuzzy=B (0..3) aligns the entries instead of indexing them
// (DESIGN.md "Lexicon matching", Fuzzy alignment) and every dict gains "lexicon_edits", one int per pair of "lexicon"; it needs a lexicon.  Neither default has
// been tuned on documents.
// a pattern with orient, alts or lexicon raises ValueError too.  The dicts' keys do not change.
// And a keyword-only pattern_best=False on both calls: True reads every word that has a pattern as the LIKELIEST member of its language under the
// recogniser's per-position distributions (DESIGN.md "Patterns", best mode) and adds "pattern_logp" to every dict; the mode is set for the call and reset
// afterwards, also when the call raises.  Without a pattern (the call's, a region's or TUATARA_PATTERN) it has no effect.
// And a keyword-only tiled=False on image_to_data: tiled=True (overlap 128) or tiled=O (a multiple of 32 in [64, 256]) reads a page larger than the detector
// canvas at full size, as overlapping tiles whose heat maps are stitched into one page map (DESIGN.md "Tiled pages"); it combines with every keyword but
// regions (no detector runs there: ValueError).  A value out of range raises RuntimeError before anything runs, as does a page the tile plan refuses.
// And a keyword-only wide=False on image_to_data: wide=True (a piece is at most 8 times as wide as high) or wide=A (2..64) reads words wider than that in
// pieces cut at ink gaps and joins the readings (DESIGN.md "Wide words"); every dict gains "pieces", a list of {"text", "conf", "quad"} (one, the item itself,
// for a word that is not wide).  It turns rectify on.  A value out of range raises RuntimeError before anything runs; wide with orient, chars, alts, lexicon,
// pattern or regions raises ValueError.
// And a keyword-only curved=False on image_to_data: True straightens the crops of words set on an arc along a spine found in the page (DESIGN.md "Curved
// words"); every dict gains "curved" (bool) and "outline" (18 [x, y] points: the top edge left to right, then the bottom edge right to left).  It turns
// rectify on.  curved with orient, chars, wide, alts, lexicon, pattern or regions raises ValueError (Engine.set_curved combines with the last four).
// And a keyword-only deskew=False on image_to_data: deskew=True (max_slope 64, gain 288, ink 128) or deskew=(max_slope, gain, ink) estimates the page's skew on the
// GPU and reads the page upright (DESIGN.md "Deskew"); boxes and quads are then the upright page's.  A value out of range raises RuntimeError with the engine's
// message.  last_call_skew() returns the latest call's record (or None), last_call_to_page(points) maps points of its result to the caller's image.
// And a keyword-only local_ink=False on image_to_data: local_ink=True (radius 16, drop 38, polarity 2 = auto) or local_ink=(radius, drop, polarity) makes tables and
// deskew take their ink bitmap from the adaptive threshold (DESIGN.md "Local ink"), so shaded, grey or inverted pages keep their rulings and their skew; with
// neither of the two on nothing runs.  A value out of range raises RuntimeError with the engine's message.
// And a keyword-only marks=False on image_to_data: marks=True (min_side 10, max_side 64, fill 24, ink 128) or marks=(min_side, max_side, fill, ink) finds the page's
// checkboxes and their state (DESIGN.md "Selection marks"); every dict gains "mark" (-1 for an item in no mark), and last_call_marks() returns the marks of the
// latest call as dicts {"box", "interior", "selected", "fill", "label", "text"}.  It does not combine with regions.
// And a keyword-only barcodes=False on image_to_data: barcodes=True (min_lines 8, ink 128, symbologies 3) or barcodes=(min_lines, ink, symbologies) reads the
// page's Code 128 and Code 39 barcodes (DESIGN.md "Barcodes"); every dict gains "barcode" (-1 for an item in no barcode), and last_call_barcodes() returns the
// barcodes of the latest call as dicts {"box", "symbology", "direction", "text", "data", "lines", "module", "gs1"}.  It does not combine with regions.
// And a keyword-only tables=False on image_to_data: tables=True (min_len 48, ink 128) or tables=(min_len, ink) finds ruling lines, tables, grids and merged
// cells in the page's pixels (DESIGN.md "Tables"); every dict gains "table" and "cell" (-1 / -1 for an item in no cell).  It combines with every keyword but
// regions (ValueError); a value out of range raises RuntimeError before anything runs.
// image: uint8 array with 3 dimensions (else RuntimeError("Input array should have 3 dimensions"),
// python.cpp:15-17).  Unlike the reference this copy honours strides and rejects != 3 channels
// instead of silently mis-copying, and the GIL is released while the GPU works.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <cmath>
#include <stdexcept>
#include <tuple>

#include "../include/tuatara.h"
#include "../include/tuatara_hip.h"

namespace py = pybind11;

static py::list quad_pairs(const std::vector<float>& q) {
  py::list l;
  for (int k = 0; k < 4; ++k) l.append(py::make_tuple(q[2 * k], q[2 * k + 1]).cast<py::list>());
  return l;
}

struct Keys { bool quad = false, conf = false, orient = false, lines = false, chars = false, blocks = false, alts = false, lexicon = false, pieces = false, pattern_logp = false, curved = false, lex_edits = false, tables = false, marks = false, barcodes = false; };   // the optional keys of an OutputItemEx's dict

static py::dict item_dict(const OutputItemEx& item, Keys k) {
  py::dict d;
  d["text"] = item.text;
  d["bbox"] = item.bbox;
  if (k.quad) d["quad"] = quad_pairs(item.quad);
  if (k.conf) {
    d["conf"] = item.conf;
    d["char_conf"] = item.char_conf;
  }
  if (k.orient) d["orient"] = item.orient;
  if (k.lines) {
    d["line"] = item.line;
    d["word"] = item.word;
  }
  if (k.blocks) d["block"] = item.block;
  if (k.tables) { d["table"] = item.table; d["cell"] = item.cell; }
  if (k.marks) d["mark"] = item.mark;
  if (k.barcodes) d["barcode"] = item.barcode;
  if (k.curved) {
    d["curved"] = item.curved;
    py::list pts;
    for (size_t j = 0; j + 1 < item.outline.size(); j += 2) pts.append(py::make_tuple(item.outline[j], item.outline[j + 1]).cast<py::list>());
    d["outline"] = pts;
  }
  if (k.chars) {
    py::list cs;
    for (const CharBox& c : item.chars) {
      py::dict cd;
      cd["char"] = c.ch;
      cd["quad"] = quad_pairs(c.quad);
      cd["bbox"] = c.bbox;
      cs.append(cd);
    }
    d["chars"] = cs;
  }
  if (k.alts) {
    py::list per_char;
    for (const std::vector<CharAlt>& opts : item.alternatives) {
      py::list l;
      for (const CharAlt& a : opts) l.append(py::make_tuple(a.ch, a.prob));
      per_char.append(l);
    }
    d["alternatives"] = per_char;
  }
  if (k.pieces) {
    py::list ps;
    for (const WordPiece& p : item.pieces) {
      py::dict pd;
      pd["text"] = p.text;
      pd["conf"] = p.conf;
      pd["quad"] = quad_pairs(p.quad);
      ps.append(pd);
    }
    d["pieces"] = ps;
  }
  if (k.pattern_logp && item.has_pattern_logp) d["pattern_logp"] = item.pattern_logp;
  if (k.lexicon) {
    py::list l;
    for (const LexMatch& m : item.lexicon) l.append(py::make_tuple(m.word, std::exp((double)m.logp)));
    d["lexicon"] = l;
    if (k.lex_edits) {   // fuzzy alignment: each match's edits, beside the (word, prob) pairs
      py::list ed;
      for (const LexMatch& m : item.lexicon) ed.append(m.edits);
      d["lexicon_edits"] = ed;
    }
  }
  return d;
}

// alts=0 | 2..8 -> K; anything else raises ValueError before anything runs
static int alts_arg(int alts) {
  if (alts != 0 && (alts < 2 || alts > 8)) throw std::invalid_argument("alts must be 0 (off) or lie in 2..8");
  return alts;
}

// wide=False | True | a number -> max_aspect (0 = off); a number outside [2, 64] raises RuntimeError, anything else TypeError, before anything runs
static float wide_arg(const py::object& wide) {
  if (wide.is_none()) return 0.f;
  if (py::isinstance<py::bool_>(wide)) return wide.cast<bool>() ? 8.f : 0.f;
  if (!py::isinstance<py::float_>(wide) && !py::isinstance<py::int_>(wide)) throw py::type_error("wide must be False, True or a number in [2, 64]");
  const double a = wide.cast<double>();
  if (!(a >= 2. && a <= 64.)) throw std::runtime_error("wide must be False, True or a number in [2, 64]");
  return (float)a;
}

// lexicon=None | a sequence of str, lexicon_m -> the word list (has = a list was given).  lexicon_m out of range, an empty list and a word with a NUL (which
// would cut it short on the way to the engine) raise ValueError here; the words themselves are checked once, by the engine's setter (raise_refused)
static bool lexicon_args(const py::object& lexicon, int lexicon_m, std::vector<std::string>& words) {
  if (lexicon.is_none()) return false;
  for (py::handle w : lexicon) words.push_back(py::cast<std::string>(w));
  if (lexicon_m < 1 || lexicon_m > 8) throw std::invalid_argument("lexicon_m must lie in 1..8");
  if (words.empty()) throw std::invalid_argument("lexicon: the word list is empty");
  for (size_t i = 0; i < words.size(); ++i)
    if (words[i].find('\0') != std::string::npos) throw std::invalid_argument("lexicon: word " + std::to_string(i) + " holds '\\x00', which names no recogniser class");
  return true;
}

// lexicon_fuzzy=None | a band 0..3, lexicon_gap -> the band (-1 = off).  A band or gap out of range, and a band without a lexicon, raise ValueError.
static int fuzzy_args(const py::object& fuzzy, double gap, bool lex) {
  if (fuzzy.is_none()) return -1;
  const int band = py::cast<int>(fuzzy);
  if (band < 0 || band > 3) throw std::invalid_argument("lexicon_fuzzy must lie in 0..3");
  if (!std::isfinite(gap) || gap > 0.0) throw std::invalid_argument("lexicon_gap must be finite and <= 0");
  if (!lex) throw std::invalid_argument("lexicon_fuzzy needs a lexicon");
  return band;
}

// a call with alts or a lexicon set that came back empty because the engine refused them raises the engine's message: a bad word list (the messages that
// begin "lexicon:") as ValueError, a refusal of the engine's state (orient, a bf16 engine) as RuntimeError
static void raise_refused() {
  const std::string msg = last_call_error();
  if (msg.rfind("lexicon:", 0) == 0) throw std::invalid_argument(msg);
  if (!msg.empty()) throw std::runtime_error(msg);
}

// orient=None|"flip"|"quarter" -> TTR_ORIENT_*
static int orient_mode(const py::object& orient) {
  if (orient.is_none()) return 0;
  const std::string v = py::str(orient);
  if (v == "flip") return 1;
  if (v == "quarter") return 2;
  throw std::invalid_argument("orient must be None, \"flip\" or \"quarter\"");
}

// allowlist / blocklist = None | str -> the string ("" = not given); a bad list raises ValueError with the engine's message (ttr_charset_mask: host only)
static void charset_args(const py::object& allow_kw, const py::object& deny_kw, std::string& allow, std::string& deny) {
  allow = allow_kw.is_none() ? std::string() : allow_kw.cast<std::string>();
  deny = deny_kw.is_none() ? std::string() : deny_kw.cast<std::string>();
  uint32_t mask[3];
  if ((!allow.empty() || !deny.empty()) && ttr_charset_mask(allow.c_str(), deny.c_str(), mask) < 0) throw std::invalid_argument(ttr_last_error());
}

// pattern = None | str -> the string ("" = not given), compiled on the host under the call's lists (ttr_pattern_compile): a bad one raises ValueError
static std::string pattern_arg(const py::object& pattern_kw, const std::string& allow, const std::string& deny, const std::string& at = std::string()) {
  if (pattern_kw.is_none()) return std::string();
  std::string p;
  try { p = pattern_kw.cast<std::string>(); } catch (const py::cast_error&) { throw std::invalid_argument(at + "pattern must be None or a string"); }
  if (p.empty()) return p;
  uint32_t mask[3];
  const bool cset = !allow.empty() || !deny.empty();
  if (cset && ttr_charset_mask(allow.c_str(), deny.c_str(), mask) < 0) throw std::invalid_argument(at + ttr_last_error());
  ttr_pattern* cp = nullptr;
  if (ttr_pattern_compile(p.c_str(), cset ? mask : nullptr, &cp) != 0) throw std::invalid_argument(at + ttr_last_error());
  ttr_pattern_free(cp);
  return p;
}

// regions=[{...}, ...] -> RegionSpecs; every entry is checked here, on the host, so a bad list raises ValueError before anything runs
static std::vector<RegionSpec> region_args(const py::object& regions_kw) {
  std::vector<RegionSpec> out;
  if (!py::isinstance<py::sequence>(regions_kw) || py::isinstance<py::str>(regions_kw)) throw std::invalid_argument("regions must be a list of dicts");
  size_t i = 0;
  for (py::handle h : regions_kw) {
    const std::string at = "regions[" + std::to_string(i++) + "]: ";
    if (!py::isinstance<py::dict>(h)) throw std::invalid_argument(at + "a region is a dict with \"quad\" or \"rect\"");
    py::dict d = py::reinterpret_borrow<py::dict>(h);
    for (auto kv : d) {
      const std::string k = py::str(kv.first);
      if (k != "quad" && k != "rect" && k != "allowlist" && k != "blocklist" && k != "pattern") throw std::invalid_argument(at + "unknown key \"" + k + "\"");
    }
    if (d.contains("quad") == d.contains("rect")) throw std::invalid_argument(at + "give \"quad\" or \"rect\" (one of them)");
    RegionSpec s;
    try {
      if (d.contains("quad")) {
        py::array_t<double, py::array::c_style | py::array::forcecast> q = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(d["quad"]);
        if (!q || q.size() != 8) throw std::invalid_argument("");
        for (int k = 0; k < 8; ++k) s.quad.push_back((float)q.data()[k]);
      } else {
        std::vector<long long> r = d["rect"].cast<std::vector<long long>>();
        if (r.size() != 4) throw std::invalid_argument("");
        s.quad.assign(8, 0.f);
        if (ttr_region_from_rect((int)r[0], (int)r[1], (int)r[2], (int)r[3], s.quad.data()) != 0) throw std::invalid_argument(at + ttr_last_error());
      }
    } catch (const py::cast_error&) {
      throw std::invalid_argument(at + "\"quad\" is 8 floats (tl, tr, br, bl), \"rect\" four integers (x0, y0, x1, y1)");
    } catch (const std::invalid_argument& ex) {
      if (*ex.what()) throw;
      throw std::invalid_argument(at + "\"quad\" is 8 floats (tl, tr, br, bl), \"rect\" four integers (x0, y0, x1, y1)");
    }
    for (int k = 0; k < 8; ++k)
      if (!(s.quad[k] == s.quad[k]) || !(s.quad[k] > -32768.f && s.quad[k] < 32768.f)) throw std::invalid_argument(at + "a coordinate is not finite or has |x| >= 32768");
    try {
      if (d.contains("allowlist") && !d["allowlist"].is_none()) s.allowlist = d["allowlist"].cast<std::string>();
      if (d.contains("blocklist") && !d["blocklist"].is_none()) s.blocklist = d["blocklist"].cast<std::string>();
    } catch (const py::cast_error&) { throw std::invalid_argument(at + "\"allowlist\" / \"blocklist\" are strings"); }
    uint32_t mask[3];
    if ((!s.allowlist.empty() || !s.blocklist.empty()) && ttr_charset_mask(s.allowlist.c_str(), s.blocklist.c_str(), mask) < 0) throw std::invalid_argument(at + ttr_last_error());
    if (d.contains("pattern")) s.pattern = pattern_arg(py::reinterpret_borrow<py::object>(d["pattern"]), s.allowlist, s.blocklist, at);
    out.push_back(std::move(s));
  }
  return out;
}

// The keywords of the page layers that read ink - tables, deskew, local_ink, marks, barcodes: "False | True | tuple of N ints | None" -> the layer's N ints.  None
// and False leave the first 0 (off) and the others at their defaults, True is the defaults, a tuple gives all of them
template <size_t N>
static std::array<int, N> layer_kw(const py::object& kw, const std::array<int, N>& defaults, const char* name, const char* fields) {
  std::array<int, N> v = defaults;
  v[0] = 0;
  if (py::isinstance<py::bool_>(kw)) v[0] = kw.cast<bool>() ? defaults[0] : 0;
  else if (py::isinstance<py::tuple>(kw) && py::len(kw) == N) {
    const py::tuple t = kw.cast<py::tuple>();
    for (size_t i = 0; i < N; ++i) v[i] = t[i].cast<int>();
  } else if (!kw.is_none()) throw py::type_error(std::string(name) + " must be False, True or (" + fields + ")");
  return v;
}
// ... and the layer's setting for one call: the values on entry; off - 0, then the defaults - on exit
template <size_t N, class... A>
struct LayerScope {
  void (*set)(A...);
  std::array<int, N> off;
  LayerScope(void (*set_)(A...), const std::array<int, N>& v, const std::array<int, N>& defaults) : set(set_), off(defaults) { off[0] = 0; std::apply(set, v); }
  ~LayerScope() { std::apply(set, off); }
  LayerScope(const LayerScope&) = delete;
};

static py::list image_to_data_wrapper(py::array_t<unsigned char, py::array::c_style | py::array::forcecast> image, std::string weights_dir,
                                      std::string output_dir, bool rectify, bool conf, py::object orient_kw, bool orient_page, bool lines, bool chars,
                                      bool blocks, py::object allowlist, py::object blocklist, py::object regions_kw, int alts, py::object lexicon, int lexicon_m,
                                      py::object pattern_kw, py::object wide_kw, bool pattern_best, bool curved, py::object lexicon_fuzzy, double lexicon_gap,
                                      py::object tiled_kw, py::object tables_kw, py::object deskew_kw, py::object local_ink_kw, py::object marks_kw, py::object barcodes_kw) {
  // barcodes=False | True (8, 128, 3) | (min_lines, ink, symbologies): barcodes for this call (DESIGN.md "Barcodes")
  const std::array<int, 3> bc_def{8, 128, 3}, bc = layer_kw(barcodes_kw, bc_def, "barcodes", "min_lines, ink, symbologies");
  const int bc_min = bc[0];
  if (bc_min != 0 && !regions_kw.is_none()) throw std::invalid_argument("barcodes does not combine with regions (the views stay empty)");
  if (bc_min != 0 && (bc_min < 4 || bc_min > 256 || bc[1] < 1 || bc[1] > 255 || bc[2] < 1 || bc[2] > 3))
    throw std::runtime_error("barcodes must be False, True or (min_lines, ink, symbologies) with min_lines in 4..256, ink in 1..255 and symbologies in 1..3");
  LayerScope barcodes_scope(set_barcodes, bc, bc_def);
  // marks=False | True (10, 64, 24, 128) | (min_side, max_side, fill, ink): selection marks for this call (DESIGN.md "Selection marks")
  const std::array<int, 4> mk_def{10, 64, 24, 128}, mk = layer_kw(marks_kw, mk_def, "marks", "min_side, max_side, fill, ink");
  const int mk_min = mk[0];
  if (mk_min != 0 && !regions_kw.is_none()) throw std::invalid_argument("marks does not combine with regions (the views stay empty)");
  if (mk_min != 0 && (mk_min < 8 || mk_min > 64 || mk[1] < mk_min || mk[1] > 128 || mk[2] < 1 || mk[2] > 255 || mk[3] < 1 || mk[3] > 255))
    throw std::runtime_error("marks must be False, True or (min_side, max_side, fill, ink) with min_side in 8..64, max_side in min_side..128, fill and ink in 1..255");
  LayerScope marks_scope(set_marks, mk, mk_def);
  // local_ink=False | True (16, 38, 2) | (radius, drop, polarity): the ink rule of tables and deskew for this call (DESIGN.md "Local ink")
  // (the ranges are the engine's to check: ttr_engine_set_ink refuses, the call comes back empty and raise_refused raises its message)
  const std::array<int, 3> ink_def{16, 38, 2}, ink = layer_kw(local_ink_kw, ink_def, "local_ink", "radius, drop, polarity");
  const int ink_r = ink[0];
  LayerScope ink_scope(set_local_ink, ink, ink_def);
  // deskew=False | True (64, 288, 128) | (max_slope, gain, ink): the page is read upright for this call (DESIGN.md "Deskew"); boxes and quads are the upright page's
  // (the ranges are the engine's to check: ttr_engine_set_deskew refuses, the call comes back empty and raise_refused raises its message)
  const std::array<int, 3> dsk_def{64, 288, 128}, dsk = layer_kw(deskew_kw, dsk_def, "deskew", "max_slope, gain, ink");
  const int dsk_m = dsk[0];
  LayerScope deskew_scope(set_deskew, dsk, dsk_def);
  // tables=False | True (48, 128) | (min_len, ink): tables for this call (DESIGN.md "Tables")
  const std::array<int, 2> tab_def{48, 128}, tab = layer_kw(tables_kw, tab_def, "tables", "min_len, ink");
  const int tab_min_len = tab[0];
  if (tab_min_len != 0 && !regions_kw.is_none()) throw std::invalid_argument("tables does not combine with regions (the views stay empty)");
  if (tab_min_len != 0 && (tab_min_len < 16 || tab_min_len > 4096 || tab[1] < 1 || tab[1] > 255))
    throw std::runtime_error("tables must be False, True or (min_len, ink) with min_len in 16..4096 and ink in 1..255");
  LayerScope tables_scope(set_tables, tab, tab_def);
  // tiled=False | True (128) | an overlap: tiled pages for this call (DESIGN.md "Tiled pages"); the engine checks the value, a refusal raises RuntimeError
  struct TiledScope {
    explicit TiledScope(int o) { set_tiled(o); }
    ~TiledScope() { set_tiled(0); }
  };
  int tiled_overlap = 0;
  if (py::isinstance<py::bool_>(tiled_kw)) tiled_overlap = tiled_kw.cast<bool>() ? 128 : 0;
  else if (py::isinstance<py::int_>(tiled_kw)) tiled_overlap = tiled_kw.cast<int>();
  else if (!tiled_kw.is_none()) throw py::type_error("tiled must be False, True or an overlap in pixels");
  if (tiled_overlap != 0 && !regions_kw.is_none()) throw std::invalid_argument("tiled does not combine with regions (no detector runs)");
  if (tiled_overlap != 0 && (tiled_overlap % 32 || tiled_overlap < 64 || tiled_overlap > 256))
    throw std::runtime_error("tiled must be False, True or an overlap that is a multiple of 32 in [64, 256]");
  TiledScope tiled_scope(tiled_overlap);
  const int orient = orient_mode(orient_kw);
  const float wide = wide_arg(wide_kw);
  alts_arg(alts);
  std::vector<std::string> words;
  const bool lex = lexicon_args(lexicon, lexicon_m, words);
  const int band = fuzzy_args(lexicon_fuzzy, lexicon_gap, lex);
  const float gap = (float)lexicon_gap;
  std::string allow, deny;
  charset_args(allowlist, blocklist, allow, deny);
  const std::string pattern = pattern_arg(pattern_kw, allow, deny);
  if (!pattern.empty() && (orient || alts || lex)) throw std::invalid_argument("pattern does not combine with orient, alts or lexicon");
  if (wide != 0.f && (orient || chars || alts || lex || !pattern.empty() || !regions_kw.is_none()))
    throw std::invalid_argument("wide does not combine with orient, chars, alts, lexicon, pattern or regions");
  if (pattern_best && (orient || alts || lex || wide != 0.f)) throw std::invalid_argument("pattern_best does not combine with orient, alts, lexicon or wide");
  if (curved && (orient || chars || wide != 0.f || alts || lex || !pattern.empty() || pattern_best || !regions_kw.is_none()))
    throw std::invalid_argument("curved does not combine with orient, chars, wide, alts, lexicon, pattern or regions");
  const bool cset = !allow.empty() || !deny.empty();
  lines = lines || blocks;   // blocks are made of lines
  if (curved) {   // curved words: rectified crops, the engine's setting for the call
    py::buffer_info wb = image.request();
    if (wb.ndim != 3) throw std::runtime_error("Input array should have 3 dimensions");
    if (wb.shape[2] != 3) throw std::runtime_error("Input array should have 3 channels");
    std::vector<OutputItemEx> got;
    {
      py::gil_scoped_release nogil;
      got = image_to_data_ex(static_cast<const uint8_t*>(wb.ptr), (int)wb.shape[0], (int)wb.shape[1], (std::ptrdiff_t)wb.shape[1] * 3, weights_dir, output_dir, true, -1, orient_page,
                             lines, false, blocks, allow, deny, Curved{});
    }
    if (got.empty()) raise_refused();
    py::list res;
    Keys keys{true, conf, false, lines, false, blocks};
    keys.curved = true;
    keys.tables = tab_min_len != 0;
    keys.marks = mk_min != 0; keys.barcodes = bc_min != 0;
    for (const auto& item : got) res.append(item_dict(item, keys));
    return res;
  }
  if (wide != 0.f) {   // wide words: rectified crops, the engine's setting for the call
    py::buffer_info wb = image.request();
    if (wb.ndim != 3) throw std::runtime_error("Input array should have 3 dimensions");
    if (wb.shape[2] != 3) throw std::runtime_error("Input array should have 3 channels");
    std::vector<OutputItemEx> got;
    {
      py::gil_scoped_release nogil;
      got = image_to_data_ex(static_cast<const uint8_t*>(wb.ptr), (int)wb.shape[0], (int)wb.shape[1], (std::ptrdiff_t)wb.shape[1] * 3, weights_dir, output_dir, true, -1, orient_page,
                             lines, false, blocks, allow, deny, Wide{wide});
    }
    if (got.empty()) raise_refused();
    py::list res;
    Keys wkeys{true, conf, false, lines, false, blocks, false, false, true};
    wkeys.tables = tab_min_len != 0;
    wkeys.marks = mk_min != 0; wkeys.barcodes = bc_min != 0;
    for (const auto& item : got) res.append(item_dict(item, wkeys));
    return res;
  }
  if (!regions_kw.is_none()) {   // regions: no detector; every check before anything runs
    if (rectify || orient || orient_page || lines || chars || blocks) throw std::invalid_argument("regions do not combine with rectify, orient, lines, chars or blocks: a region is read as the quad it is");
    std::vector<RegionSpec> regs = region_args(regions_kw);
    for (RegionSpec& s : regs) if (s.allowlist.empty() && s.blocklist.empty()) { s.allowlist = allow; s.blocklist = deny; }   // the call's own lists where a region has none
    for (RegionSpec& s : regs) {
      if (s.pattern.empty()) s.pattern = pattern;                                                                              // ... and its pattern
      if (!s.pattern.empty() && (alts || lex)) throw std::invalid_argument("pattern does not combine with orient, alts or lexicon");
    }
    bool with_pattern = false;
    for (const RegionSpec& s : regs) with_pattern = with_pattern || !s.pattern.empty();
    py::buffer_info rb = image.request();
    if (rb.ndim != 3) throw std::runtime_error("Input array should have 3 dimensions");
    if (rb.shape[2] != 3) throw std::runtime_error("Input array should have 3 channels");
    std::vector<OutputItemEx> got;
    {
      py::gil_scoped_release nogil;
      got = band >= 0 ? image_to_data_ex(static_cast<const uint8_t*>(rb.ptr), (int)rb.shape[0], (int)rb.shape[1], (std::ptrdiff_t)rb.shape[1] * 3, weights_dir, output_dir, regs, alts, words, lexicon_m, band, gap)
                : lex ? image_to_data_ex(static_cast<const uint8_t*>(rb.ptr), (int)rb.shape[0], (int)rb.shape[1], (std::ptrdiff_t)rb.shape[1] * 3, weights_dir, output_dir, regs, alts, words, lexicon_m)
                : pattern_best ? image_to_data_ex(static_cast<const uint8_t*>(rb.ptr), (int)rb.shape[0], (int)rb.shape[1], (std::ptrdiff_t)rb.shape[1] * 3, weights_dir, output_dir, regs, alts, true)
                : image_to_data_ex(static_cast<const uint8_t*>(rb.ptr), (int)rb.shape[0], (int)rb.shape[1], (std::ptrdiff_t)rb.shape[1] * 3, weights_dir, output_dir, regs, alts);
    }
    if ((alts || lex || with_pattern || dsk_m || ink_r) && got.empty()) raise_refused();
    py::list res;
    for (const auto& item : got) {
      Keys keys{true, conf, false, false, false, false, alts != 0, lex, false, pattern_best};
      keys.lex_edits = band >= 0;
      py::dict d = item_dict(item, keys);
      d["region"] = item.region;
      res.append(d);
    }
    return res;
  }
  py::buffer_info buf = image.request();
  if (buf.ndim != 3) throw std::runtime_error("Input array should have 3 dimensions");
  if (buf.shape[2] != 3) throw std::runtime_error("Input array should have 3 channels");
  const uint8_t* data = static_cast<const uint8_t*>(buf.ptr);
  const int rows = (int)buf.shape[0], cols = (int)buf.shape[1];
  std::vector<OutputItemEx> items;
  {
    py::gil_scoped_release nogil;   // (orient = None: the 7-argument call, which leaves the orientation to TUATARA_ORIENT)
    items = pattern_best     ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny, pattern, true)
            : !pattern.empty() ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny, pattern)
            : band >= 0 ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny, alts, words, lexicon_m, band, gap)
            : lex    ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny, alts, words, lexicon_m)
            : alts   ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny, alts)
            : cset   ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, allow, deny)
            : blocks ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, true, chars, true)
            : chars  ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, true)
            : lines  ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, true)
            : orient ? image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify, orient, orient_page)
                     : image_to_data_ex(data, rows, cols, (std::ptrdiff_t)cols * 3, weights_dir, output_dir, rectify);
  }
  if ((alts || lex || !pattern.empty() || tiled_overlap || dsk_m || ink_r) && items.empty()) raise_refused();
  py::list result;
  Keys keys{rectify, conf, orient != 0, lines, chars, blocks, alts != 0, lex, false, pattern_best};
  keys.lex_edits = band >= 0;
  keys.tables = tab_min_len != 0;
  keys.marks = mk_min != 0; keys.barcodes = bc_min != 0;
  for (const auto& item : items) result.append(item_dict(item, keys));
  return result;
}

// pytuatara.images_to_data(images, weights_dir, outputs_dir) -> list (one entry per image, input order) of the lists image_to_data returns.
// images: a sequence of uint8 arrays [H, W, 3] of any sizes.  What a caller of the reference writes as a loop over image_to_data (bindings/run_ocr.py:92),
// on one cached engine: same-sized images travel as batches, the host-to-device copies run beside the GPU's work, the GIL is released meanwhile.
// Keyword-only mixed_batches=False: True batches images that share one detector canvas, whatever their sizes (DESIGN.md "Mixed-size batches"); same results.
static py::list images_to_data_wrapper(py::sequence images, std::string weights_dir, std::string output_dir, bool rectify, bool conf, py::object orient_kw,
                                       bool orient_page, bool lines, bool chars, bool blocks, bool mixed_batches, py::object allowlist, py::object blocklist, int alts,
                                       py::object lexicon, int lexicon_m, py::object pattern_kw, bool pattern_best, py::object lexicon_fuzzy, double lexicon_gap) {
  const int orient = orient_mode(orient_kw);
  alts_arg(alts);
  std::vector<std::string> words;
  const bool lex = lexicon_args(lexicon, lexicon_m, words);
  const int band = fuzzy_args(lexicon_fuzzy, lexicon_gap, lex);
  const float gap = (float)lexicon_gap;
  std::string allow, deny;
  charset_args(allowlist, blocklist, allow, deny);
  const std::string pattern = pattern_arg(pattern_kw, allow, deny);
  if (!pattern.empty() && (orient || alts || lex)) throw std::invalid_argument("pattern does not combine with orient, alts or lexicon");
  if (pattern_best && (orient || alts || lex)) throw std::invalid_argument("pattern_best does not combine with orient, alts or lexicon");
  const bool cset = !allow.empty() || !deny.empty();
  lines = lines || blocks;   // blocks are made of lines
  std::vector<py::array_t<unsigned char, py::array::c_style | py::array::forcecast>> keep;   // contiguous uint8 views / copies, alive for the call
  std::vector<ImageView> views;
  for (py::handle h : images) {
    auto a = py::array_t<unsigned char, py::array::c_style | py::array::forcecast>::ensure(h);
    if (!a) throw std::runtime_error("images_to_data: every image must convert to a uint8 array");
    py::buffer_info buf = a.request();
    if (buf.ndim != 3) throw std::runtime_error("Input array should have 3 dimensions");
    if (buf.shape[2] != 3) throw std::runtime_error("Input array should have 3 channels");
    views.push_back(ImageView{static_cast<const uint8_t*>(buf.ptr), (int)buf.shape[0], (int)buf.shape[1], (std::ptrdiff_t)buf.shape[1] * 3});
    keep.push_back(std::move(a));
  }
  std::vector<std::vector<OutputItemEx>> pages;
  {
    py::gil_scoped_release nogil;
    pages = pattern_best ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny, pattern, true)
            : !pattern.empty() ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny, pattern)
            : band >= 0 ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny, alts, words, lexicon_m, band, gap)
            : lex ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny, alts, words, lexicon_m)
            : alts ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny, alts)
            : cset ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, mixed_batches, allow, deny)
            : mixed_batches ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, chars, blocks, true)
            : blocks ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, true, chars, true)
            : chars  ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, lines, true)
            : lines  ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient ? orient : -1, orient_page, true)
            : orient ? images_to_data_ex(views, weights_dir, output_dir, rectify, orient, orient_page)
                     : images_to_data_ex(views, weights_dir, output_dir, rectify);
  }
  if ((alts || lex || !pattern.empty()) && pages.empty() && !views.empty()) raise_refused();
  py::list result;
  for (const auto& items : pages) {
    py::list page;
    Keys keys{rectify, conf, orient != 0, lines, chars, blocks, alts != 0, lex, false, pattern_best};
    keys.lex_edits = band >= 0;
    for (const auto& item : items) page.append(item_dict(item, keys));
    result.append(page);
  }
  return result;
}

PYBIND11_MODULE(pytuatara, m) {
  m.doc() = "Tuatara ocr (MI355X-native engine)";
  m.def("image_to_data", &image_to_data_wrapper, py::arg("image"), py::arg("weights_dir"), py::arg("outputs_dir"), py::kw_only(),
        py::arg("rectify") = false, py::arg("conf") = false, py::arg("orient") = py::none(), py::arg("orient_page") = false,
        py::arg("lines") = false, py::arg("chars") = false, py::arg("blocks") = false, py::arg("allowlist") = py::none(), py::arg("blocklist") = py::none(), py::arg("regions") = py::none(), py::arg("alts") = 0, py::arg("lexicon") = py::none(), py::arg("lexicon_m") = 1, py::arg("pattern") = py::none(), py::arg("wide") = false, py::arg("pattern_best") = false, py::arg("curved") = false, py::arg("lexicon_fuzzy") = py::none(), py::arg("lexicon_gap") = -6.9077554, py::arg("tiled") = false, py::arg("tables") = false, py::arg("deskew") = false, py::arg("local_ink") = false, py::arg("marks") = false, py::arg("barcodes") = false, "Extract text and bounding boxes from an image");
  m.def("last_call_marks", []() {
    py::list out;
    for (const SelectionMark& s : last_call_marks()) {
      py::dict d;
      d["box"] = py::make_tuple(s.box[0], s.box[1], s.box[2], s.box[3]);
      d["interior"] = py::make_tuple(s.interior[0], s.interior[1], s.interior[2], s.interior[3]);
      d["selected"] = s.selected; d["fill"] = s.area ? (double)s.inked / (double)s.area : 0.0; d["label"] = s.label; d["text"] = s.text;
      out.append(d);
    }
    return out;
  }, "The selection marks of this thread's latest image_to_data call (DESIGN.md \"Selection marks\"), [] when marks were off");
  m.def("last_call_barcodes", []() {
    py::list out;
    for (const Barcode& b : last_call_barcodes()) {
      py::dict d;
      d["box"] = py::make_tuple(b.box[0], b.box[1], b.box[2], b.box[3]);
      d["symbology"] = b.symbology == 1 ? "code128" : "code39"; d["direction"] = b.direction; d["data"] = py::bytes(b.data);
      d["text"] = py::reinterpret_steal<py::object>(PyUnicode_DecodeLatin1(b.data.data(), (Py_ssize_t)b.data.size(), nullptr));
      d["lines"] = b.lines; d["module"] = b.module; d["gs1"] = b.gs1;
      out.append(d);
    }
    return out;
  }, "The barcodes of this thread's latest image_to_data call (DESIGN.md \"Barcodes\"), [] when barcodes were off");
  m.def("last_call_skew", []() -> py::object {
    const PageSkew s = last_call_skew();
    if (!s.on) return py::none();
    py::dict d;
    d["slope"] = s.slope; d["found"] = s.found; d["C"] = s.C; d["S"] = s.S; d["w"] = s.w; d["h"] = s.h; d["mode"] = s.mode; d["degrees"] = s.degrees;
    return d;
  }, "The skew record of this thread's latest image_to_data call (DESIGN.md \"Deskew\"), or None when deskew was off");
  m.def("last_call_to_page", [](std::vector<std::pair<float, float>> pts) {
    const PageSkew s = last_call_skew();
    for (auto& p : pts) { float x = 0.f, y = 0.f; s.to_page(p.first, p.second, &x, &y); p = {x, y}; }
    return pts;
  }, py::arg("points"), "Points (x, y) of the latest call's result -> the caller's image (the identity when deskew was off)");
  m.def("images_to_data", &images_to_data_wrapper, py::arg("images"), py::arg("weights_dir"), py::arg("outputs_dir"), py::kw_only(),
        py::arg("rectify") = false, py::arg("conf") = false, py::arg("orient") = py::none(), py::arg("orient_page") = false,
        py::arg("lines") = false, py::arg("chars") = false, py::arg("blocks") = false, py::arg("mixed_batches") = false, py::arg("allowlist") = py::none(), py::arg("blocklist") = py::none(), py::arg("alts") = 0, py::arg("lexicon") = py::none(), py::arg("lexicon_m") = 1, py::arg("pattern") = py::none(), py::arg("pattern_best") = false, py::arg("lexicon_fuzzy") = py::none(), py::arg("lexicon_gap") = -6.9077554, "image_to_data over a sequence of images of any sizes: one list of {text, bbox} per image, in input order");
}
