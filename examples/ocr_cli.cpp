// Counterpart of the reference's example CLIs (examples/resume.cpp:7-12, examples/table.cpp:9-10):
//   ocr_cli <image.png> <weights_dir> <outputs_dir>
// reads the image as BGR (what cv::imread(path, cv::IMREAD_COLOR) hands the reference), calls image_to_data and,
// unlike the reference (which discards the result), prints one "x1 y1 x2 y2<TAB>text" line per item.
//   ocr_cli --rectify <image.png> <weights_dir> <outputs_dir>   reads tilted words on deskewed crops (DESIGN.md "Rectified crops") and
// prints "x1 y1 x2 y2<TAB>tl.x tl.y tr.x tr.y br.x br.y bl.x bl.y<TAB>text" per item.
//   ocr_cli --conf <image.png> <weights_dir> <outputs_dir>      prints "x1 y1 x2 y2<TAB>conf<TAB>text" per item, conf being the recogniser's
// confidence in the word, a probability to 6 decimals (DESIGN.md "Recognition confidence").
//   ocr_cli --orient <image.png> <weights_dir> <outputs_dir>    reads every word at the quarter turn the recogniser is most sure of (DESIGN.md
// "Word orientation", TTR_ORIENT_QUARTER, per word) and prints "x1 y1 x2 y2<TAB>degrees<TAB>conf<TAB>text" per item.
//   ocr_cli --lines <image.png> <weights_dir> <outputs_dir>     groups the words into text lines (DESIGN.md "Text lines") and prints the page's text, one line
// of the page per output line, in reading order, the words joined by one space.
//   ocr_cli --chars <image.png> <weights_dir> <outputs_dir>     cuts every word into its characters (DESIGN.md "Character boxes") and prints one line per
// character, "c x1 y1 x2 y2" with the character's bbox as integers, the words in item order.
//   ocr_cli --blocks <image.png> <weights_dir> <outputs_dir>    groups the text lines into blocks (DESIGN.md "Text blocks") and prints the page's text block
// after block in reading order - a column to its end before the next -, one line of the page per output line and an empty line between blocks.
//   ocr_cli --allowlist S --blocklist S ...                      in front of any form above: the characters the recogniser may / may not emit (DESIGN.md
// "Character sets"), e.g. --allowlist 0123456789 for a field of digits.  They reach the call as TUATARA_ALLOWLIST / TUATARA_BLOCKLIST.
//   ocr_cli --pattern P ...                                      in front of any form above: a regular expression every word must match (DESIGN.md "Patterns"),
// e.g. --pattern '\d{2}/\d{2}/\d{4}' for dates.  It reaches the call as TUATARA_PATTERN; a bad pattern fails, naming the offset or the character, before the
// image is read.
//   ocr_cli --pattern P --pattern-best <image.png> <weights_dir> <outputs_dir>   in front of the plain form, with --pattern: reads every word as the LIKELIEST
// member of the pattern's language (DESIGN.md "Patterns", best mode) and prints "x1 y1 x2 y2<TAB>text<TAB>logp" per item, logp being the log-probability of
// the text under the recogniser's per-position distributions, to 6 decimals.
//   ocr_cli --regions FILE <image.png> <weights_dir> <outputs_dir>   reads the regions FILE lists, with no detector, each under its own character set
// (DESIGN.md "Regions and per-row character sets").  One region per line: "x0 y0 x1 y1 [allow [deny]]" - the pixels [x0, x1) x [y0, y1) - or eight floats
// "tl.x tl.y tr.x tr.y br.x br.y bl.x bl.y [allow [deny]]"; '#' starts a comment.  Prints "x1 y1 x2 y2<TAB>conf<TAB>text" per region, in the file's
// order, every number to 9 significant digits (a float read back is the float that was printed).  A malformed file fails, naming the line, before the image is read.
//   ocr_cli --alts K [--nbest M] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: K alternatives per character (2..8; DESIGN.md "Character
// alternatives").  Prints "x1 y1 x2 y2<TAB>conf<TAB>text" per item, then one line per character of the text, "<TAB>c: a=p b=p ..." with that position's
// alternatives in rank order and their probabilities, and - with --nbest M (1..64) - the M likeliest readings of the word, "<TAB>#i score text".
//   ocr_cli --lexicon FILE [--lexicon-m M] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: matches every word that is read against the word
// list in FILE, one word per line (DESIGN.md "Lexicon matching"; empty lines are skipped).  Prints "x1 y1 x2 y2<TAB>conf<TAB>text" per item, then its M best
// entries (1..8, default 1), one line each: "<TAB>=i prob word", prob being exp(log-probability) to 6 decimals.  A bad entry fails, naming its index.
// With --lexicon-fuzzy B [--lexicon-gap G] (B in 0..3; G <= 0, default ln 1e-3 = -6.9077554, not tuned on documents) the entries are aligned against the
// reading instead of indexed (DESIGN.md "Lexicon matching", Fuzzy alignment) and each match's line gains its edits: "<TAB>=i prob word edits".
//   ocr_cli --wide [A] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: reads words wider than A times their height (2..64, default 8) in
// pieces cut at ink gaps, on rectified crops (DESIGN.md "Wide words").  Prints "x1 y1 x2 y2<TAB>conf<TAB>text" per item and, under a wide item, one line per
// piece: "<TAB>|conf text".  A value that is no number in [2, 64] fails before the image is read.
//   ocr_cli --curved <image.png> <weights_dir> <outputs_dir>   in front of the plain form: straightens the crops of words set on an arc along a spine found in
// the page, on rectified crops (DESIGN.md "Curved words").  Prints "x1 y1 x2 y2<TAB>conf<TAB>text" per item and, under a curved item, one line
// "<TAB>~x y x y ..." with the 18 points of its outline.
//   ocr_cli --tiled [O] ...   in front of any form above that runs the detector, options included: a page larger than the detector canvas is read at full size,
// as overlapping tiles whose heat maps are stitched into one page map (DESIGN.md "Tiled pages"); O = the overlap in pixels, a multiple of 32 in [64, 256]
// (default 128, not tuned on documents).  A page of more than 64 tiles or with a side above 8192 fails with the rule's message.
//   ocr_cli --local-ink [R] ...   in front of --tables or --deskew (and of --tiled): the two layers take their ink bitmap from the adaptive threshold - a pixel
// darker than its neighbourhood's mean - so shaded, grey or inverted pages keep their rulings and their skew (DESIGN.md "Local ink"; R = the window's radius in
// px, 1..64, default 16, with drop 38 and automatic polarity, none of them tuned on documents).
//   ocr_cli --deskew [MAX_SLOPE] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: the page's skew is estimated on the GPU and the page read
// upright (DESIGN.md "Deskew"; MAX_SLOPE = the largest slope tried, px per 512 px, 1..128, default 64, not tuned on documents); prints "# page 0 slope S degrees D
// found F" and then the plain form's lines, the boxes in the upright page's frame, each followed by a tab and the box's first corner on the caller's image.
//   ocr_cli --marks [MIN_SIDE] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: finds the page's checkboxes (DESIGN.md "Selection marks";
//                                 sides MIN_SIDE..64 px, default 10) and prints one line per mark - "[x]" or "[ ]", the frame x0 y0 x1 y1, a tab, the text of
//                                 the word it stands in front of - in (y, x) order
//   ocr_cli --barcodes [MIN_LINES] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: reads the page's Code 128 and Code 39 barcodes (DESIGN.md
//                                 "Barcodes"; MIN_LINES = the scan lines that must agree, 4..256, default 8) and prints one line per barcode - "code128" or
//                                 "code39", the direction 0..3, the box x0 y0 x1 y1, a tab, the text (bytes outside 32..126 as \xHH) - in (y0, x0) order
//   ocr_cli --tables [MIN_LEN] <image.png> <weights_dir> <outputs_dir>   in front of the plain form: finds ruling lines, tables, grids and merged cells in the
// page's pixels (DESIGN.md "Tables"; MIN_LEN = the shortest ruling in px, 16..4096, default 48, not tuned on documents) and prints each table as "# table T x0 y0
// x1 y1 rows cols" followed by its rows, the cells' texts separated by tabs (a merged cell's text at its first base cell; a line break inside a cell as " / ").
//   ocr_cli --decode-only <image.png> <out.raw>   writes the decoded BGR bytes (tests of the PNG reader; no GPU).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../include/tuatara.h"
#include "../include/tuatara_hip.h"
#include "png_decode.h"

// --regions FILE: one RegionSpec per line (see the top of the file); throws, naming the line, on anything else
static std::vector<RegionSpec> read_regions(const char* path) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error(std::string("cannot read regions file ") + path);
  std::vector<RegionSpec> out;
  std::string line;
  for (int ln = 1; std::getline(f, line); ++ln) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    const std::string at = std::string(path) + ":" + std::to_string(ln) + ": ";
    const size_t nnum = tok.size() >= 8 ? 8 : 4;
    if (tok.size() < 4 || tok.size() > nnum + 2) throw std::runtime_error(at + "a region is \"x0 y0 x1 y1 [allow [deny]]\" or eight floats \"tl tr br bl [allow [deny]]\"");
    double v[8];
    for (size_t k = 0; k < nnum; ++k) {
      char* end = nullptr;
      v[k] = std::strtod(tok[k].c_str(), &end);
      if (end == tok[k].c_str() || *end || !std::isfinite(v[k]) || std::fabs(v[k]) >= 32768.) throw std::runtime_error(at + "\"" + tok[k] + "\" is not a coordinate");
    }
    RegionSpec r;
    if (nnum == 4) {
      for (int k = 0; k < 4; ++k) if (v[k] != std::floor(v[k])) throw std::runtime_error(at + "a rectangle's corners are integers");
      if (v[2] <= v[0] || v[3] <= v[1]) throw std::runtime_error(at + "the rectangle is empty");
      r = region_from_rect((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
    } else {
      for (int k = 0; k < 8; ++k) r.quad.push_back((float)v[k]);
    }
    if (tok.size() > nnum) r.allowlist = tok[nnum];
    if (tok.size() > nnum + 1) r.blocklist = tok[nnum + 1];
    out.push_back(std::move(r));
  }
  return out;
}

int main(int argc, const char** argv) {
  try {
    if (argc >= 2 && std::string(argv[1]) == "--local-ink") {   // a leading option of the forms that read the page's ink (--tables, --deskew): the radius for the calls that follow
      int radius = 16, used = 1;
      if (argc >= 3 && argv[2][0] != '-' && std::string(argv[2]).find_first_not_of("0123456789") == std::string::npos && std::strlen(argv[2]) <= 4) {
        radius = std::atoi(argv[2]); used = 2;
        if (radius < 1 || radius > 64) throw std::runtime_error("--local-ink takes a radius in 1..64 px (default 16)");
      }
      set_local_ink(radius);
      argv[used] = argv[0]; argv += used; argc -= used;
    }
    if (argc >= 2 && std::string(argv[1]) == "--tiled") {   // a leading option of every form that runs the detector: the overlap for the calls that follow
      int overlap = 128, used = 1;
      if (argc >= 3 && argv[2][0] >= '0' && argv[2][0] <= '9' && std::string(argv[2]).find_first_not_of("0123456789") == std::string::npos && std::strlen(argv[2]) <= 4) {
        overlap = std::atoi(argv[2]); used = 2;
      }
      if (overlap % 32 || overlap < 64 || overlap > 256) throw std::runtime_error("--tiled takes an overlap that is a multiple of 32 in [64, 256] (default 128)");
      set_tiled(overlap);
      argv[used] = argv[0]; argv += used; argc -= used;
    }
    while (argc >= 3 && (std::string(argv[1]) == "--allowlist" || std::string(argv[1]) == "--blocklist" || std::string(argv[1]) == "--pattern")) {   // leading options, any order
      const std::string opt = argv[1];
      if (opt == "--pattern") {   // checked here, on the host, under every class: the engine compiles it again under the set in force
        ttr_pattern* p = nullptr;
        if (ttr_pattern_compile(argv[2], nullptr, &p) != 0) throw std::runtime_error(std::string("--pattern: ") + ttr_last_error());
        ttr_pattern_free(p);
      }
      setenv(opt == "--allowlist" ? "TUATARA_ALLOWLIST" : opt == "--blocklist" ? "TUATARA_BLOCKLIST" : "TUATARA_PATTERN", argv[2], 1);
      argv[2] = argv[0]; argv += 2; argc -= 2;
    }
    if (argc >= 2 && std::string(argv[1]) == "--pattern-best") {
      if (argc != 5) throw std::runtime_error("--pattern-best goes in front of <image.png> <weights_dir> <outputs_dir>");
      if (!std::getenv("TUATARA_PATTERN")) throw std::runtime_error("--pattern-best needs --pattern P in front of it");
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false, -1, false, false,
                                                         false, false, std::string(), std::string(), std::string(), true);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const OutputItemEx& it : items) printf("%g %g %g %g\t%s\t%.6f\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.text.c_str(), it.has_pattern_logp ? it.pattern_logp : -INFINITY);
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--wide") {
      float a = 8.f;
      if (argc == 6) {
        char* end = nullptr;
        const double v = std::strtod(argv[2], &end);
        if (end == argv[2] || *end || !(v >= 2. && v <= 64.)) throw std::runtime_error("--wide takes an aspect in [2, 64] (default 8)");
        a = (float)v;
      }
      if (argc != 5 && argc != 6) throw std::runtime_error("--wide [A] goes in front of <image.png> <weights_dir> <outputs_dir>");
      const char* const* rest = argv + (argc - 3);                      // <image.png> <weights_dir> <outputs_dir>
      pngdec::Image img = pngdec::read(rest[0]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, rest[1], rest[2], true, -1, false, false,
                                                         false, false, std::string(), std::string(), Wide{a});
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const OutputItemEx& it : items) {
        printf("%g %g %g %g\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
        if (it.pieces.size() > 1)
          for (const WordPiece& p : it.pieces) printf("\t|%.6f %s\n", p.conf, p.text.c_str());
      }
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--deskew") {
      int max_slope = 64, used = 1;
      if (argc == 6) {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (!end || *end || v < 1 || v > 128) throw std::runtime_error("--deskew takes a largest slope in 1..128 px per 512 px (default 64)");
        max_slope = (int)v; used = 2;
      }
      if (argc - used != 4) throw std::runtime_error("--deskew [MAX_SLOPE] goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[used + 1]);
      set_deskew(max_slope);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[used + 2], argv[used + 3], false);
      set_deskew(0);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      const PageSkew sk = last_call_skew();
      printf("# page 0 slope %d degrees %.4f found %d\n", sk.slope, sk.degrees, sk.found);
      for (const OutputItemEx& it : items) {
        float px = 0.f, py = 0.f;
        sk.to_page(it.bbox[0], it.bbox[1], &px, &py);
        printf("%g %g %g %g\t%s\t%.9g %.9g\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.text.c_str(), px, py);
      }
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--barcodes") {
      int min_lines = 8, used = 1;
      if (argc == 6) {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (!end || *end || v < 4 || v > 256) throw std::runtime_error("--barcodes takes the scan lines that must agree, 4..256 (default 8)");
        min_lines = (int)v; used = 2;
      }
      if (argc - used != 4) throw std::runtime_error("--barcodes [MIN_LINES] goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[used + 1]);
      set_barcodes(min_lines);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[used + 2], argv[used + 3], false);
      set_barcodes(0);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const Barcode& b : last_call_barcodes()) {                   // one line per barcode: its symbology, direction and box, then its text
        printf("%s %d %d %d %d %d\t", b.symbology == 1 ? "code128" : "code39", b.direction, b.box[0], b.box[1], b.box[2], b.box[3]);
        for (unsigned char c : b.data) { if (c >= 32 && c < 127 && c != '\\') putchar(c); else printf("\\x%02X", c); }
        putchar('\n');
      }
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--marks") {
      int min_side = 10, used = 1;
      if (argc == 6) {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (!end || *end || v < 8 || v > 64) throw std::runtime_error("--marks takes a smallest side in 8..64 px (default 10)");
        min_side = (int)v; used = 2;
      }
      if (argc - used != 4) throw std::runtime_error("--marks [MIN_SIDE] goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[used + 1]);
      set_marks(min_side);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[used + 2], argv[used + 3], false);
      set_marks(0);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const SelectionMark& m : last_call_marks())                  // one line per mark: its state, its frame, the word it stands in front of
        printf("%s %d %d %d %d\t%s\n", m.selected ? "[x]" : "[ ]", m.box[0], m.box[1], m.box[2], m.box[3], m.text.c_str());
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--tables") {
      int min_len = 48, used = 1;
      if (argc == 6) {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (!end || *end || v < 16 || v > 4096) throw std::runtime_error("--tables takes a shortest ruling in 16..4096 px (default 48)");
        min_len = (int)v; used = 2;
      }
      if (argc - used != 4) throw std::runtime_error("--tables [MIN_LEN] goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[used + 1]);
      set_tables(min_len);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[used + 2], argv[used + 3], false);
      set_tables(0);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      const std::vector<TableGrid> tabs = last_call_tables();
      for (size_t t = 0; t < tabs.size(); ++t) {
        const TableGrid& g = tabs[t];
        printf("# table %zu %d %d %d %d %d %d\n", t, g.bbox[0], g.bbox[1], g.bbox[2], g.bbox[3], g.rows, g.cols);
        for (int i = 0; i < g.rows; ++i) {
          for (int j = 0; j < g.cols; ++j) {
            std::string s = g.text[(size_t)i * g.cols + j];
            for (size_t p = 0; (p = s.find('\n', p)) != std::string::npos;) s.replace(p, 1, " / ");
            printf("%s%s", j ? "\t" : "", s.c_str());
          }
          printf("\n");
        }
      }
      return 0;
    }
    if (argc >= 2 && std::string(argv[1]) == "--curved") {
      if (argc != 5) throw std::runtime_error("--curved goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], true, -1, false, false,
                                                         false, false, std::string(), std::string(), Curved{});
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const OutputItemEx& it : items) {
        printf("%g %g %g %g\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
        if (it.curved) {
          printf("\t~");
          for (size_t k = 0; k < it.outline.size(); ++k) printf("%s%.9g", k ? " " : "", it.outline[k]);
          printf("\n");
        }
      }
      return 0;
    }
    int alts = 0, nbest_m = 0;
    while (argc >= 3 && (std::string(argv[1]) == "--alts" || std::string(argv[1]) == "--nbest")) {
      char* end = nullptr;
      const long v = std::strtol(argv[2], &end, 10);
      const bool is_alts = std::string(argv[1]) == "--alts";
      if (end == argv[2] || *end || (is_alts ? (v < 2 || v > 8) : (v < 1 || v > 64))) throw std::runtime_error(is_alts ? "--alts takes K in 2..8" : "--nbest takes M in 1..64");
      (is_alts ? alts : nbest_m) = (int)v;
      argv[2] = argv[0]; argv += 2; argc -= 2;
    }
    if (nbest_m && !alts) throw std::runtime_error("--nbest needs --alts K");
    if (alts) {
      if (argc != 4) throw std::runtime_error("--alts K [--nbest M] goes in front of <image.png> <weights_dir> <outputs_dir>");
      pngdec::Image img = pngdec::read(argv[1]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[2], argv[3], false, -1, false, false,
                                                         false, false, std::string(), std::string(), alts);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const OutputItemEx& it : items) {
        printf("%g %g %g %g\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
        for (size_t c = 0; c < it.alternatives.size(); ++c) {
          printf("\t%c:", c < it.text.size() ? it.text[c] : '?');
          for (const CharAlt& a : it.alternatives[c]) printf(" %s=%.6f", a.ch.c_str(), a.prob);
          printf("\n");
        }
        if (nbest_m) {
          const std::vector<WordReading> rd = nbest(it, nbest_m);
          for (size_t i = 0; i < rd.size(); ++i) printf("\t#%zu %.6f %s\n", i, rd[i].score, rd[i].text.c_str());
        }
      }
      return 0;
    }
    std::string lex_file;
    int lex_m = 0, lex_band = -1;
    float lex_gap = LexFuzzy{}.gap;
    bool lex_gap_set = false;
    while (argc >= 3 && (std::string(argv[1]) == "--lexicon" || std::string(argv[1]) == "--lexicon-m" || std::string(argv[1]) == "--lexicon-fuzzy" ||
                         std::string(argv[1]) == "--lexicon-gap")) {
      if (std::string(argv[1]) == "--lexicon") lex_file = argv[2];
      else if (std::string(argv[1]) == "--lexicon-fuzzy") {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (end == argv[2] || *end || v < 0 || v > 3) throw std::runtime_error("--lexicon-fuzzy takes a band B in 0..3");
        lex_band = (int)v;
      } else if (std::string(argv[1]) == "--lexicon-gap") {
        char* end = nullptr;
        const double v = std::strtod(argv[2], &end);
        if (end == argv[2] || *end || !std::isfinite(v) || v > 0.0) throw std::runtime_error("--lexicon-gap takes a finite log-probability G <= 0");
        lex_gap = (float)v; lex_gap_set = true;
      } else {
        char* end = nullptr;
        const long v = std::strtol(argv[2], &end, 10);
        if (end == argv[2] || *end || v < 1 || v > 8) throw std::runtime_error("--lexicon-m takes M in 1..8");
        lex_m = (int)v;
      }
      argv[2] = argv[0]; argv += 2; argc -= 2;
    }
    if (lex_m && lex_file.empty()) throw std::runtime_error("--lexicon-m needs --lexicon FILE");
    if (lex_band >= 0 && lex_file.empty()) throw std::runtime_error("--lexicon-fuzzy needs --lexicon FILE");
    if (lex_gap_set && lex_band < 0) throw std::runtime_error("--lexicon-gap needs --lexicon-fuzzy B");
    if (!lex_file.empty()) {
      if (argc != 4) throw std::runtime_error("--lexicon FILE [--lexicon-m M] [--lexicon-fuzzy B [--lexicon-gap G]] goes in front of <image.png> <weights_dir> <outputs_dir>");
      std::ifstream f(lex_file);
      if (!f) throw std::runtime_error("cannot read lexicon file " + lex_file);
      std::vector<std::string> words;
      for (std::string line; std::getline(f, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty()) words.push_back(line);
      }
      if (words.empty()) throw std::runtime_error("the lexicon file " + lex_file + " holds no word");
      pngdec::Image img = pngdec::read(argv[1]);
      std::vector<OutputItemEx> items =
          lex_band >= 0 ? image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[2], argv[3], false, -1, false, false, false, false,
                                           std::string(), std::string(), 0, words, lex_m ? lex_m : 1, lex_band, lex_gap)
                        : image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[2], argv[3], false, -1, false, false,
                                           false, false, std::string(), std::string(), 0, words, lex_m ? lex_m : 1);
      if (!last_call_error().empty()) return 1;                         // (the message is on stderr)
      for (const OutputItemEx& it : items) {
        printf("%g %g %g %g\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
        for (const LexMatch& m : it.lexicon) {
          if (lex_band >= 0) printf("\t=%d %.6f %s %d\n", m.index, std::exp((double)m.logp), m.word.c_str(), m.edits);
          else printf("\t=%d %.6f %s\n", m.index, std::exp((double)m.logp), m.word.c_str());
        }
      }
      return 0;
    }
    if (argc == 4 && std::string(argv[1]) == "--decode-only") {
      pngdec::Image img = pngdec::read(argv[2]);
      FILE* f = fopen(argv[3], "wb");
      if (!f) throw std::runtime_error("cannot write output");
      fwrite(img.bgr.data(), 1, img.bgr.size(), f);
      fclose(f);
      printf("%d %d\n", img.rows, img.cols);
      return 0;
    }
    if (argc == 6 && std::string(argv[1]) == "--regions") {
      const std::vector<RegionSpec> regions = read_regions(argv[2]);   // (before the image and the engine: a malformed file costs nothing)
      pngdec::Image img = pngdec::read(argv[3]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[4], argv[5], regions);
      if (items.size() != regions.size()) return 1;                    // (the message is on stderr)
      for (const OutputItemEx& it : items) printf("%.9g %.9g %.9g %.9g\t%.9g\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--rectify") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], true);
      for (const OutputItemEx& it : items) {
        const std::vector<float>& q = it.quad;
        printf("%g %g %g %g\t%g %g %g %g %g %g %g %g\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7],
               it.text.c_str());
      }
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--conf") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false);
      for (const OutputItemEx& it : items) printf("%g %g %g %g\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.conf, it.text.c_str());
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--orient") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false, 2, false);
      for (const OutputItemEx& it : items)
        printf("%g %g %g %g\t%d\t%.6f\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.orient, it.conf, it.text.c_str());
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--lines") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false, -1, false, true);
      std::vector<size_t> at(items.size());
      for (size_t i = 0; i < at.size(); ++i) at[i] = i;
      std::sort(at.begin(), at.end(), [&](size_t a, size_t b) { return items[a].line != items[b].line ? items[a].line < items[b].line : items[a].word < items[b].word; });
      for (size_t k = 0; k < at.size(); ++k) {
        if (k) fputc(items[at[k]].line != items[at[k - 1]].line ? '\n' : ' ', stdout);
        fputs(items[at[k]].text.c_str(), stdout);
      }
      if (!at.empty()) fputc('\n', stdout);
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--blocks") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false, -1, false, true, false, true);
      std::vector<size_t> at(items.size());
      for (size_t i = 0; i < at.size(); ++i) at[i] = i;
      std::sort(at.begin(), at.end(), [&](size_t a, size_t b) {
        const OutputItemEx &x = items[a], &y = items[b];
        return x.block != y.block ? x.block < y.block : x.block_line != y.block_line ? x.block_line < y.block_line : x.word < y.word;
      });
      for (size_t k = 0; k < at.size(); ++k) {
        const OutputItemEx &it = items[at[k]];
        if (k) fputs(it.block != items[at[k - 1]].block ? "\n\n" : it.block_line != items[at[k - 1]].block_line ? "\n" : " ", stdout);
        fputs(it.text.c_str(), stdout);
      }
      if (!at.empty()) fputc('\n', stdout);
      return 0;
    }
    if (argc == 5 && std::string(argv[1]) == "--chars") {
      pngdec::Image img = pngdec::read(argv[2]);
      std::vector<OutputItemEx> items = image_to_data_ex(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[3], argv[4], false, -1, false, false, true);
      for (const auto& it : items)
        for (const CharBox& c : it.chars)
          printf("%s %d %d %d %d\n", c.ch.c_str(), (int)std::lround(c.bbox[0]), (int)std::lround(c.bbox[1]), (int)std::lround(c.bbox[2]), (int)std::lround(c.bbox[3]));
      return 0;
    }
    if (argc != 4) {
      std::cerr << "usage: ocr_cli --barcodes [MIN_LINES] <image.png> <weights_dir> <outputs_dir> | ocr_cli --marks [MIN_SIDE] <image.png> <weights_dir> <outputs_dir> | ocr_cli --deskew [MAX_SLOPE] <image.png> <weights_dir> <outputs_dir> | ocr_cli --tables [MIN_LEN] <image.png> <weights_dir> <outputs_dir> | ocr_cli [--tiled [O]] [--allowlist S] [--blocklist S] [--pattern P [--pattern-best]] [--wide [A] | --curved | --alts K [--nbest M] | --lexicon FILE [--lexicon-m M] [--lexicon-fuzzy B [--lexicon-gap G]] | --rectify | --conf | --orient | --lines | --chars | --blocks | --regions FILE] <image.png> <weights_dir> <outputs_dir>" << std::endl;
      return 2;
    }
    pngdec::Image img = pngdec::read(argv[1]);
    std::vector<OutputItem> items = image_to_data(img.bgr.data(), img.rows, img.cols, (std::ptrdiff_t)img.cols * 3, argv[2], argv[3]);
    if (tiled() && !last_call_error().empty()) return 1;              // (--tiled refused: the message is on stderr)
    for (const OutputItem& it : items) printf("%g %g %g %g\t%s\n", it.bbox[0], it.bbox[1], it.bbox[2], it.bbox[3], it.text.c_str());
    return 0;
  } catch (const std::exception& ex) {
    std::cerr << "ocr_cli: " << ex.what() << std::endl;
    return 1;
  }
}
