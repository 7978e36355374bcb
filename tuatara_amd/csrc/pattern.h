// Patterns (DESIGN.md "Patterns"): a word constrained to a regular expression.  Host only, no HIP: the pattern language, its automaton and the table the
// two kernels of pattern.hip walk.  Compiles with plain g++, like geometry.cpp.
//
// The language is a strict subset of Python's `re` / POSIX ERE over the recogniser's characters: literals, `\` + punctuation, \d, \w, `.`, [...] sets with
// ranges and a leading ^, ( ... ) groups with | alternation, and the quantifiers ? * + {m} {m,n} {m,} (0 <= m <= n <= 25) on an atom or group.  The alphabet
// is the recogniser's class ids through Tokenizer::itos: the usable classes are 1..94 except 88 (Tokenizer::decode stops at id 88); a backslash stands for
// ids 69 and 87 (the charset rule).  The automaton is compiled under a class mask (charset_mask's form): a transition on a blocked class does
// not exist.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "geometry.h"

namespace ttr {

constexpr int kPatCols = 96;             // columns of a table row: 0 = EOS, 1..94 the characters, 95 padding
constexpr int kPatNone = 0xFFFF;         // no transition
constexpr int kPatFree = 255;            // mind of a DONE state: it constrains nothing
constexpr int kPatMaxChars = 25;         // characters the recogniser can return
constexpr int kPatMaxStates = 256;       // states of one minimised automaton (its DONE state not counted)
constexpr int kPatMaxTable = 1024;       // states of one call's concatenated table
constexpr int kPatMaxBytes = 255;        // bytes of a pattern

// One compiled automaton: rows 0 .. states - 1 are the minimal DFA (start = 0, numbered breadth first), row `states` is its DONE state.
//   delta [states + 1][96]  delta[s][0] = done iff s accepts; delta[s][c], 1 <= c <= 94, the successor on class c; 0xFFFF = none.  The DONE row holds
//                           itself on every class of the mask (EOS included)
//   mind  [states + 1]      least number of characters from s to acceptance (at most 254); 255 for DONE
struct Pattern {
  std::string src;
  uint32_t mask[3] = {0xffffffffu, 0xffffffffu, 0x7fffffffu};
  int states = 0, start = 0, done = 0;
  std::vector<uint16_t> delta;
  std::vector<uint8_t> mind;
  int rows() const { return states + 1; }
};

// pattern under mask (null = every class).  Throws std::runtime_error: a syntax error names its byte offset, a character that names no usable class is
// named in charset_mask's words, an automaton of more than 256 states, an empty language and a shortest member over 25 characters name the figure.
Pattern pattern_compile(const Tokenizer& tok, const char* pattern, const uint32_t* mask);
// the automaton of a row without a pattern: a DONE state alone under the mask - a plain masked argmax
Pattern pattern_none(const uint32_t* mask);
// 1 = text is a member of the language, 0 = it is not, -1 = text holds a byte that names no usable class.  The budget of 25 characters is not applied.
int pattern_matches(const Tokenizer& tok, const Pattern& p, const char* text);
// the choice rule: may class c be chosen at character position pos (0..25) in state s?  (`delta`, `mind`: any table in the format above)
inline bool pattern_allows(const uint16_t* delta, const uint8_t* mind, int s, int pos, int c) {
  const int t = delta[(size_t)s * kPatCols + c];
  return t != kPatNone && (c == 0 || mind[t] == kPatFree || pos + 1 + mind[t] <= kPatMaxChars);
}

// The likeliest member (DESIGN.md "Patterns", the best decode): the member w of p's language with at most 25 characters and the largest
//   score(w) = the sum, in position order from 0.0f, of lp[i][w_i] for i < L, then + lp[L][0]     (lp: [26][96] fp32, row i = character position i, column 0 = EOS)
// by the Viterbi recurrence over (position, state): V[0][start] = 0, V[i + 1][t] = max over (s, c >= 1, delta[s][c] == t) of V[i][s] + lp[i][c]; ties to the
// lower class, then the lower state; the result the maximum over (L, accepting s) of V[L][s] + lp[L][0], ties to the smaller L, then the lower state.  fp32
// addition is monotone, so each maximum is the maximum of the sequentially rounded sums.  A value of -inf or NaN is never chosen.
// path [26]: the classes w_0 .. w_(L-1), zeros behind; *len = L; *logp = score(w).  Returns 0, or 1 when no member has a finite score (path zeros, len -1, logp -inf).
int pattern_best_from_lp(const Pattern& p, const float* lp, int32_t* path, int32_t* len, float* logp);

// A call's table: automata appended into one state space.  add() returns the start state of the appended automaton (its rows are shifted by the rows
// before it); throws, naming the total, beyond 1024 states.
struct PatternTable {
  std::vector<uint16_t> delta;
  std::vector<uint8_t> mind;
  int rows() const { return (int)mind.size(); }
  int add(const Pattern& p, const char* what);
};

}  // namespace ttr
