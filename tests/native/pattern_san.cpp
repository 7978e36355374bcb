// The pattern compiler (tuatara_amd/csrc/pattern.cpp; DESIGN.md "Patterns") under sanitizers: a stand-alone program, host code only.
//   pattern_san <corpus>    one pattern per line, hex-encoded (any bytes but NUL).  Every pattern is compiled with and without a class mask: it must compile
//                           or be refused with a C++ exception; a compiled one is walked (every table entry in range, the budget invariant), matched against
//                           a few texts and appended to a call table until that refuses.  Prints "compiled C refused R".
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../tuatara_amd/csrc/pattern.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

static std::string unhex(const std::string& h) {
  std::string s;
  for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return s;
}

// every entry inside the table, and the budget invariant over every reachable (state, position)
static bool walk(const Pattern& p) {
  const int rows = p.rows();
  if ((int)p.delta.size() != rows * kPatCols || (int)p.mind.size() != rows || p.done != rows - 1 || p.mind[p.done] != kPatFree) return false;
  for (int s = 0; s < rows; ++s) for (int c = 0; c < kPatCols; ++c) { const int t = p.delta[(size_t)s * kPatCols + c]; if (t != kPatNone && t >= rows) return false; }
  std::set<std::pair<int, int>> seen{{p.start, 0}};
  std::vector<std::pair<int, int>> todo{{p.start, 0}};
  while (!todo.empty()) {
    const std::pair<int, int> sp = todo.back(); todo.pop_back();
    int n = 0;
    for (int c = 0; c < 95; ++c) {
      if (!pattern_allows(p.delta.data(), p.mind.data(), sp.first, sp.second, c)) continue;
      ++n;
      if (sp.second == kPatMaxChars && sp.first != p.done && c != 0) return false;
      const std::pair<int, int> nx{p.delta[(size_t)sp.first * kPatCols + c], sp.second + 1};
      if (sp.second < kPatMaxChars && seen.insert(nx).second) todo.push_back(nx);
    }
    if (!n) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: pattern_san <corpus>");
  std::ifstream f(argv[1]);
  if (!f) return fail("cannot read the corpus");
  const Tokenizer tok;
  uint32_t digits_capitals[3];
  charset_mask(tok, "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ", nullptr, digits_capitals);
  const char* texts[] = {"", "12.34", "AB1234", "Hello", "\\\\", "a b", "0000000000000000000000000", "abababab"};
  int compiled = 0, refused = 0;
  PatternTable table;
  bool table_full = false;
  std::string line;
  while (std::getline(f, line)) {
    const std::string src = unhex(line);
    for (const uint32_t* mask : {(const uint32_t*)nullptr, (const uint32_t*)digits_capitals}) {
      try {
        const Pattern p = pattern_compile(tok, src.c_str(), mask);
        ++compiled;
        if (!walk(p)) return fail("a bad table for " + line);
        for (const char* t : texts) { const int m = pattern_matches(tok, p, t); if (m < -1 || m > 1) return fail("pattern_matches"); }
        if (!table_full) { try { table.add(p, "pattern_san"); } catch (const std::runtime_error&) { table_full = true; } }
      } catch (const std::runtime_error& e) {
        if (std::string(e.what()).rfind("pattern: ", 0) != 0) return fail(std::string("an unexpected refusal: ") + e.what());
        ++refused;
      }
    }
  }
  const Pattern none = pattern_none(digits_capitals);
  if (!walk(none)) return fail("pattern_none");
  if (table.rows() > kPatMaxTable) return fail("the table grew past its limit");
  std::cout << "compiled " << compiled << " refused " << refused << std::endl;
  return 0;
}
