// The host rule of the best decode of patterns (tuatara_amd/csrc/pattern.cpp: pattern_best_from_lp; DESIGN.md "Patterns") under sanitizers: a stand-alone
// program, host code only.
//   pattern_best_san <seed> <tables>    every pattern of the list, with and without a class mask, against <tables> seeded tables of four kinds - random,
//                                       peaked, all equal, laden with -inf and NaN.  A returned path must be a member of at most 25 characters whose score,
//                                       summed again in order, has the returned bits; outputs may be null.  Prints "found F none N".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/pattern.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: pattern_best_san <seed> <tables>");
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int tables = std::atoi(argv[2]);
  const Tokenizer tok;
  uint32_t digits_capitals[3];
  charset_mask(tok, "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ./", nullptr, digits_capitals);
  const char* patterns[] = {"(USD|EUR|GBP)\\d{2}", "\\d{2}/\\d{2}", "[A-C]{1,3}x?", "\\d+\\.\\d{2}", "\\d*", ".{0,25}", "[ab]*a[ab]{7}", "\\d{25}", "[A-Z]{2}\\d{2,6}"};
  std::mt19937 rng(seed);
  std::normal_distribution<float> normal(0.f, 3.f);
  std::uniform_real_distribution<float> unit(0.f, 1.f);
  int found = 0, none = 0;
  for (const char* src : patterns) {
    for (int masked = 0; masked < 2; ++masked) {
      Pattern p;
      try { p = pattern_compile(tok, src, masked ? digits_capitals : nullptr); }
      catch (const std::runtime_error&) { continue; }   // (the mask empties some languages)
      for (int t = 0; t < tables; ++t) {
        const int kind = t & 3;
        std::vector<float> lp((size_t)26 * kPatCols, -INFINITY);
        for (int r = 0; r < 26; ++r) {
          const float row = normal(rng);
          const int peak = (int)(unit(rng) * 94.99f);
          for (int c = 0; c < 95; ++c) {
            float v = kind == 2 ? row : -std::fabs(normal(rng));
            if (kind == 1 && c != peak) v -= 30.f;
            if (kind == 3 && unit(rng) < 0.35f) v = -INFINITY;
            if (kind == 3 && unit(rng) < 0.01f) v = std::numeric_limits<float>::quiet_NaN();
            lp[(size_t)r * kPatCols + c] = v;
          }
        }
        int32_t path[26], len = 99;
        float logp = 1.f;
        const int rc = pattern_best_from_lp(p, lp.data(), path, &len, &logp);
        if (pattern_best_from_lp(p, lp.data(), nullptr, nullptr, nullptr) != rc) return fail("the outputs change the answer");
        if (rc == 1) {
          ++none;
          if (len != -1 || logp != -INFINITY) return fail("no member, but a length or a score");
          continue;
        }
        if (rc != 0 || len < 0 || len > kPatMaxChars) return fail(std::string("bad length for ") + src);
        ++found;
        int s = p.start;
        float sum = 0.0f;
        for (int i = 0; i < len; ++i) {
          if (path[i] < 1 || path[i] > 94) return fail("a class out of range");
          const int next = p.delta[(size_t)s * kPatCols + path[i]];
          if (next == kPatNone) return fail("the path leaves the automaton");
          sum += lp[(size_t)i * kPatCols + path[i]];
          s = next;
        }
        if (p.delta[(size_t)s * kPatCols] == kPatNone) return fail("the path does not end in an accepting state");
        sum += lp[(size_t)len * kPatCols];
        if (std::memcmp(&sum, &logp, 4) != 0 || !(logp > -INFINITY)) return fail("the score is not the path's sum");
        for (int i = len; i < 26; ++i) if (path[i] != 0) return fail("the path is not zero behind its end");
      }
    }
  }
  std::cout << "found " << found << " none " << none << std::endl;
  return 0;
}
