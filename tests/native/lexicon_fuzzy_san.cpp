// The host rule of the fuzzy alignment of lexicon entries (tuatara_amd/csrc/geometry.cpp: lexicon_fuzzy_from_lp; DESIGN.md "Lexicon matching", Fuzzy
// alignment) under sanitizers: a stand-alone program, host code only.
//   lexicon_fuzzy_san <seed> <tables>   <tables> seeded tables of six kinds - random, peaked, spreads of 1e30, all equal, with blocked classes (-inf), laden
//                                       with NaN - each in a heap block of exactly 26 x 96 floats, against records of every length 1..25 in a block of
//                                       exactly n x 32 bytes, at every band 0..3 and three gaps.  A score is never NaN, band 0 has no edits and equals the
//                                       sequential sum where that is finite, a score never falls as the band grows; every refusal returns -1 and writes
//                                       nothing.  Prints "scored S finite F".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../tuatara_amd/csrc/geometry.h"

using namespace ttr;

static int fail(const std::string& what) { std::cerr << "FAILED: " << what << std::endl; return 1; }

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: lexicon_fuzzy_san <seed> <tables>");
  const unsigned seed = (unsigned)std::atoi(argv[1]);
  const int tables = std::atoi(argv[2]);
  std::mt19937 rng(seed);
  std::normal_distribution<float> normal(0.f, 3.f);
  std::uniform_real_distribution<float> unit(0.f, 1.f);
  const float ninf = -std::numeric_limits<float>::infinity();
  const float gaps[3] = {0.f, -6.9077554f, -50.f};
  long scored = 0, finite = 0;
  for (int t = 0; t < tables; ++t) {
    const int kind = t % 6;
    std::vector<float> x(26 * 95);
    for (float& v : x) v = normal(rng);
    if (kind == 1) for (int p = 0; p < 26; ++p) x[p * 95 + (int)(unit(rng) * 94.99f)] += 20.f;
    if (kind == 2) for (float& v : x) { const float u = unit(rng); if (u < 0.3f) v = 1e30f; else if (u < 0.6f) v = -1e30f; }
    if (kind == 3) for (float& v : x) v = 1.25f;
    float* lp = new float[26 * 96];                           // exactly the table: a read past either end is a report
    for (int p = 0; p < 26; ++p) {
      float mx = ninf, sum = 0.f;
      for (int c = 0; c < 95; ++c) mx = std::max(mx, x[p * 95 + c]);
      for (int c = 0; c < 95; ++c) sum += std::exp(x[p * 95 + c] - mx);
      const float lprob = std::log(1.f / sum);
      for (int c = 0; c < 95; ++c) lp[p * 96 + c] = (x[p * 95 + c] - mx) + lprob;
      lp[p * 96 + 95] = ninf;
      if (kind == 4) for (int c = 1; c < 95; c += 3) lp[p * 96 + c] = ninf;
      if (kind == 5) for (int c = 0; c < 95; ++c) if (unit(rng) < 0.05f) lp[p * 96 + c] = std::nanf("");
    }
    const int n = 50;                                          // two records of every length
    uint8_t* rec = new uint8_t[(size_t)n * kLexRecord];
    memset(rec, 0, (size_t)n * kLexRecord);
    for (int i = 0; i < n; ++i) {
      const int L = 1 + i % 25;
      rec[i * kLexRecord] = (uint8_t)L;
      for (int k = 1; k <= L; ++k) rec[i * kLexRecord + k] = (uint8_t)(1 + (int)(unit(rng) * 93.99f));
    }
    float* logp = new float[4 * n];
    int32_t* edits = new int32_t[4 * n];
    for (float gap : gaps) {
      for (int band = 0; band <= 3; ++band)
        if (lexicon_fuzzy_from_lp(lp, rec, n, band, gap, logp + band * n, edits + band * n) != 0) return fail("a good call was refused");
      for (int i = 0; i < n; ++i) {
        float s = 0.f;                                         // the rigid scorer's chain
        for (int p = 0; p <= rec[i * kLexRecord]; ++p) s += lp[p * 96 + rec[i * kLexRecord + 1 + p]];
        if (std::isnan(s)) s = ninf;
        if (memcmp(&s, &logp[i], 4) != 0 || edits[i] != 0) return fail("band 0 is not the rigid sum");
        for (int band = 0; band <= 3; ++band) {
          const float v = logp[band * n + i];
          if (std::isnan(v)) return fail("a NaN was taken up");
          if (edits[band * n + i] < 0 || edits[band * n + i] > 2 * kLexMaxLen + 1) return fail("edits out of range");
          if (band && v < logp[(band - 1) * n + i]) return fail("logp fell as the band grew");
          ++scored;
          finite += std::isfinite(v);
        }
      }
    }
    // the refusals: nothing is written
    logp[0] = 123.f; edits[0] = 77;
    const float nan = std::nanf("");
    bool refused = lexicon_fuzzy_from_lp(nullptr, rec, n, 1, -1.f, logp, edits) == -1 && lexicon_fuzzy_from_lp(lp, nullptr, n, 1, -1.f, logp, edits) == -1 &&
                   lexicon_fuzzy_from_lp(lp, rec, n, 1, -1.f, nullptr, edits) == -1 && lexicon_fuzzy_from_lp(lp, rec, n, 1, -1.f, logp, nullptr) == -1 &&
                   lexicon_fuzzy_from_lp(lp, rec, n, -1, -1.f, logp, edits) == -1 && lexicon_fuzzy_from_lp(lp, rec, n, 4, -1.f, logp, edits) == -1 &&
                   lexicon_fuzzy_from_lp(lp, rec, n, 1, 1e-6f, logp, edits) == -1 && lexicon_fuzzy_from_lp(lp, rec, n, 1, ninf, logp, edits) == -1 &&
                   lexicon_fuzzy_from_lp(lp, rec, n, 1, nan, logp, edits) == -1;
    rec[(n - 1) * kLexRecord] = 26;                            // the last record's length: checked before the first is scored
    refused = refused && lexicon_fuzzy_from_lp(lp, rec, n, 1, -1.f, logp, edits) == -1;
    rec[(n - 1) * kLexRecord] = 0;
    refused = refused && lexicon_fuzzy_from_lp(lp, rec, n, 1, -1.f, logp, edits) == -1;
    if (!refused || logp[0] != 123.f || edits[0] != 77) return fail("a refusal");
    delete[] lp; delete[] rec; delete[] logp; delete[] edits;
  }
  printf("scored %ld finite %ld\n", scored, finite);
  return 0;
}
