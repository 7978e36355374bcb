// Patterns (DESIGN.md "Patterns"): the pattern language -> Thompson NFA -> subset construction -> trim -> Moore minimisation -> the table of pattern.h.
// Host only, no HIP.
#include "pattern.h"

#include <algorithm>
#include <bitset>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>

namespace ttr {

namespace {

typedef std::bitset<kPatCols> ClassSet;
constexpr int kMaxNfa = 20000;      // NFA states a pattern may expand to (nested counted repeats multiply)
constexpr int kMaxSubset = 8192;    // DFA states before minimisation

bool usable(int c) { return c >= 1 && c <= 94 && c != 88; }

std::string quote(unsigned char ch) {           // charset_mask's form: ASCII as itself, anything else as \xNN
  char b[16];
  if (ch >= 0x20 && ch < 0x7f) snprintf(b, sizeof b, "'%c'", ch); else snprintf(b, sizeof b, "'\\x%02x'", ch);
  return std::string(b);
}

[[noreturn]] void syntax(size_t at, const std::string& what) { throw std::runtime_error("pattern: offset " + std::to_string(at) + ": " + what); }

// the usable classes a byte names (a backslash: ids 69 and 87); empty = it names none
ClassSet classes_of(const Tokenizer& tok, unsigned char ch) {
  ClassSet s;
  for (int i = 1; i <= 94; ++i) if (usable(i) && (unsigned char)tok.itos[i] == ch) s.set(i);
  return s;
}

ClassSet named(const Tokenizer& tok, unsigned char ch, size_t at) {
  const ClassSet s = classes_of(tok, ch);
  if (s.none()) throw std::runtime_error("pattern: offset " + std::to_string(at) + " holds " + quote(ch) + ", which names no recogniser class");
  return s;
}

struct Node {
  enum Kind { kSet, kCat, kAlt, kRep, kEmpty } kind = kEmpty;
  ClassSet set;
  std::vector<std::unique_ptr<Node>> kids;
  int lo = 0, hi = 0;   // kRep: hi < 0 = unbounded
};
typedef std::unique_ptr<Node> NodeP;

struct Parser {
  const Tokenizer& tok;
  const std::string& s;
  size_t i = 0;
  int depth = 0;
  ClassSet all, digits, word;

  Parser(const Tokenizer& t, const std::string& src) : tok(t), s(src) {
    for (int c = 1; c <= 94; ++c) if (usable(c)) all.set(c);
    for (int c = 1; c <= 94; ++c) {
      if (!usable(c)) continue;
      const unsigned char ch = (unsigned char)tok.itos[c];
      if (ch >= '0' && ch <= '9') { digits.set(c); word.set(c); }
      if ((ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || ch == '_') word.set(c);
    }
  }
  bool more() const { return i < s.size(); }
  static bool is_quant(char c) { return c == '?' || c == '*' || c == '+' || c == '{'; }

  // `\` + what follows, at s[i] == '\\': a class escape or an escaped punctuation character
  ClassSet escape() {
    const size_t at = i++;
    if (!more()) syntax(at, "a backslash at the end of the pattern");
    const unsigned char ch = (unsigned char)s[i++];
    if (ch == 'd') return digits;
    if (ch == 'w') return word;
    if ((ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z'))
      syntax(at, std::string("the escape \\") + (char)ch + " is not part of the pattern language (\\d, \\w and \\ + punctuation are)");
    return named(tok, ch, at + 1);   // (a blank, '~', ']' or a non-ASCII byte: refused by name)
  }

  NodeP set_atom() {   // at s[i] == '['
    const size_t open = i++;
    bool neg = false;
    if (more() && s[i] == '^') { neg = true; ++i; }
    ClassSet m;
    bool first = true;
    for (;;) {
      if (!more()) syntax(open, "'[' without its ']'");
      if (s[i] == ']') {
        if (first) syntax(i, "an empty set (']' itself names no recogniser class)");
        ++i;
        break;
      }
      first = false;
      const size_t at = i;
      unsigned char lo = (unsigned char)s[i];
      ClassSet one;
      bool single = true;   // a plain byte, which may start a range
      if (lo == '\\') {
        one = escape();
        single = i >= 2 && s[i - 1] != 'd' && s[i - 1] != 'w';
        lo = (unsigned char)s[i - 1];
      } else { one = named(tok, lo, at); ++i; }
      if (single && i + 1 < s.size() && s[i] == '-' && s[i + 1] != ']') {   // a range lo-hi, by byte value
        const size_t hat = i + 1;
        unsigned char hi = (unsigned char)s[hat];
        i = hat;
        if (hi == '\\') {
          const ClassSet h = escape();
          hi = (unsigned char)s[i - 1];
          if (hi == 'd' || hi == 'w') syntax(hat, "a class escape cannot end a range");
          (void)h;
        } else { named(tok, hi, hat); ++i; }
        if (hi < lo) syntax(at, std::string("the range ") + (char)lo + "-" + (char)hi + " runs backwards");
        for (int ch = lo; ch <= hi; ++ch) m |= named(tok, (unsigned char)ch, at);
      } else m |= one;
    }
    NodeP n(new Node);
    n->kind = Node::kSet;
    n->set = neg ? (all & ~m) : m;
    return n;
  }

  int number() {   // digits at s[i]; -1 when there are none
    if (!more() || s[i] < '0' || s[i] > '9') return -1;
    int v = 0;
    while (more() && s[i] >= '0' && s[i] <= '9') { v = std::min(v * 10 + (s[i] - '0'), 100000); ++i; }
    return v;
  }

  NodeP atom() {
    const size_t at = i;
    const unsigned char ch = (unsigned char)s[i];
    if (is_quant((char)ch)) syntax(at, std::string("the quantifier '") + (char)ch + "' has nothing before it");
    if (ch == '(') {
      if (++depth > 64) syntax(at, "groups nest deeper than 64");
      ++i;
      if (more() && s[i] == '?') syntax(i, "group extensions (?...) are not part of the pattern language");
      NodeP n = alternation();
      if (!more() || s[i] != ')') syntax(at, "'(' without its ')'");
      ++i; --depth;
      return n;
    }
    NodeP n(new Node);
    n->kind = Node::kSet;
    if (ch == '[') return set_atom();
    if (ch == '.') { n->set = all; ++i; return n; }
    if (ch == '\\') { n->set = escape(); return n; }
    if (ch == '^' || ch == '$') syntax(at, std::string("the anchor '") + (char)ch + "' is not part of the pattern language: a pattern always matches the whole word (write \\" + (char)ch + " for the character)");
    n->set = named(tok, ch, at);   // (']' names no usable class: refused here)
    ++i;
    return n;
  }

  NodeP quantified() {
    NodeP a = atom();
    if (!more() || !is_quant(s[i])) return a;
    const size_t at = i;
    int lo = 0, hi = -1;
    const char q = s[i++];
    if (q == '?') { lo = 0; hi = 1; }
    else if (q == '*') { lo = 0; hi = -1; }
    else if (q == '+') { lo = 1; hi = -1; }
    else {
      lo = number();
      if (lo < 0) syntax(at, "'{' opens a quantifier {m}, {m,n} or {m,}: write \\{ for the character");
      hi = lo;
      if (more() && s[i] == ',') { ++i; hi = number(); }
      if (!more() || s[i] != '}') syntax(at, "'{' opens a quantifier {m}, {m,n} or {m,}: write \\{ for the character");
      ++i;
      if (lo > kPatMaxChars || hi > kPatMaxChars || (hi >= 0 && hi < lo))
        syntax(at, "the quantifier " + s.substr(at, i - at) + " is out of range: 0 <= m <= n <= 25");
    }
    if (more() && is_quant(s[i])) syntax(i, std::string("the quantifier '") + s[i] + "' has nothing before it (lazy, possessive and stacked quantifiers are not part of the pattern language)");
    NodeP r(new Node);
    r->kind = Node::kRep; r->lo = lo; r->hi = hi;
    r->kids.push_back(std::move(a));
    return r;
  }

  NodeP concatenation() {
    NodeP n(new Node);
    n->kind = Node::kCat;
    while (more() && s[i] != '|' && s[i] != ')') n->kids.push_back(quantified());
    if (n->kids.empty()) n->kind = Node::kEmpty;
    return n;
  }

  NodeP alternation() {
    NodeP n(new Node);
    n->kind = Node::kAlt;
    n->kids.push_back(concatenation());
    while (more() && s[i] == '|') { ++i; n->kids.push_back(concatenation()); }
    if (n->kids.size() == 1) return std::move(n->kids[0]);
    return n;
  }

  NodeP parse() {
    NodeP n = alternation();
    if (more()) syntax(i, "')' without its '('");   // (alternation stops at nothing else)
    return n;
  }
};

struct Nfa {
  struct Edge { ClassSet on; int to; };
  std::vector<std::vector<Edge>> edge;
  std::vector<std::vector<int>> eps;
  int fresh() {
    if ((int)edge.size() >= kMaxNfa) throw std::runtime_error("pattern: it expands to more than " + std::to_string(kMaxNfa) + " NFA states: nested counted repeats multiply");
    edge.emplace_back(); eps.emplace_back();
    return (int)edge.size() - 1;
  }
  // the fragment of n from state `from`; returns its end state
  int build(const Node& n, int from) {
    switch (n.kind) {
      case Node::kEmpty: return from;
      case Node::kSet: { const int to = fresh(); edge[from].push_back({n.set, to}); return to; }
      case Node::kCat: { int at = from; for (const NodeP& k : n.kids) at = build(*k, at); return at; }
      case Node::kAlt: {
        const int end = fresh();
        for (const NodeP& k : n.kids) { const int b = fresh(); eps[from].push_back(b); eps[build(*k, b)].push_back(end); }
        return end;
      }
      case Node::kRep: {
        int at = from;
        for (int r = 0; r < n.lo; ++r) at = build(*n.kids[0], at);
        if (n.hi < 0) {              // star: at -> in -> body -> in; in -> out
          const int in = fresh(), out = fresh();
          eps[at].push_back(in); eps[in].push_back(out);
          eps[build(*n.kids[0], in)].push_back(in);
          return out;
        }
        const int end = fresh();     // hi - lo optional copies, each may be skipped to the end
        for (int r = n.lo; r < n.hi; ++r) { eps[at].push_back(end); at = build(*n.kids[0], at); }
        eps[at].push_back(end);
        return end;
      }
    }
    return from;
  }
  void close(std::vector<int>& set) const {   // epsilon closure, sorted and unique
    std::vector<char> in(edge.size(), 0);
    std::vector<int> stack;
    for (int s : set) if (!in[s]) { in[s] = 1; stack.push_back(s); }
    set.clear();
    while (!stack.empty()) {
      const int s = stack.back(); stack.pop_back();
      set.push_back(s);
      for (int t : eps[s]) if (!in[t]) { in[t] = 1; stack.push_back(t); }
    }
    std::sort(set.begin(), set.end());
  }
};

ClassSet mask_set(const uint32_t* mask) {
  ClassSet m;
  for (int c = 0; c < 95; ++c) if (!mask || ((mask[c >> 5] >> (c & 31)) & 1u)) m.set(c);
  return m;
}

void fill_done(Pattern& p, const ClassSet& m) {   // the DONE row: itself on every class of the mask, EOS included
  const int d = p.done;
  for (int c = 0; c < 95; ++c) if (c == 0 || m.test(c)) p.delta[(size_t)d * kPatCols + c] = (uint16_t)d;
  p.mind[d] = kPatFree;
}

}  // namespace

Pattern pattern_none(const uint32_t* mask) {
  Pattern p;
  const ClassSet m = mask_set(mask);
  for (int i = 0; i < 3; ++i) p.mask[i] = mask ? mask[i] : p.mask[i];
  p.states = 0; p.start = 0; p.done = 0;
  p.delta.assign(kPatCols, (uint16_t)kPatNone);
  p.mind.assign(1, 0);
  fill_done(p, m);
  return p;
}

Pattern pattern_compile(const Tokenizer& tok, const char* pattern, const uint32_t* mask) {
  if (!pattern || !*pattern) syntax(0, "the pattern is empty");
  const std::string src(pattern);
  if (src.size() > (size_t)kPatMaxBytes) syntax(kPatMaxBytes, "the pattern has " + std::to_string(src.size()) + " bytes: at most 255");
  Parser ps(tok, src);
  const NodeP ast = ps.parse();
  Nfa nfa;
  const int n0 = nfa.fresh();
  const int nend = nfa.build(*ast, n0);
  const ClassSet allowed = mask_set(mask) & ps.all;

  // subset construction, over the classes the mask allows
  std::map<std::vector<int>, int> index;
  std::vector<std::vector<int>> sets;
  std::vector<std::vector<int>> dt;   // [state][96], -1 = none
  std::vector<char> acc;
  auto intern = [&](std::vector<int>& set) {
    auto it = index.find(set);
    if (it != index.end()) return it->second;
    if ((int)sets.size() >= kMaxSubset) throw std::runtime_error("pattern: its automaton has more than " + std::to_string(kMaxSubset) + " states before minimisation: at most 256 after it");
    const int id = (int)sets.size();
    index.emplace(set, id);
    acc.push_back(std::binary_search(set.begin(), set.end(), nend) ? 1 : 0);
    sets.push_back(set);
    dt.emplace_back(kPatCols, -1);
    return id;
  };
  {
    std::vector<int> s0{n0};
    nfa.close(s0);
    intern(s0);
  }
  for (size_t d = 0; d < sets.size(); ++d) {
    ClassSet any;
    for (int s : sets[d]) for (const Nfa::Edge& e : nfa.edge[s]) any |= e.on;
    any &= allowed;
    // classes with the same set of edges go the same way: group them by the edges that carry them
    std::map<std::vector<int>, int> by_targets;
    const std::vector<int> cur = sets[d];   // (a copy: intern grows `sets`)
    for (int c = 1; c <= 94; ++c) {
      if (!any.test(c)) continue;
      std::vector<int> to;
      for (int s : cur) for (const Nfa::Edge& e : nfa.edge[s]) if (e.on.test(c)) to.push_back(e.to);
      std::sort(to.begin(), to.end());
      to.erase(std::unique(to.begin(), to.end()), to.end());
      auto it = by_targets.find(to);
      if (it == by_targets.end()) {
        std::vector<int> closed = to;
        nfa.close(closed);
        it = by_targets.emplace(to, intern(closed)).first;
      }
      dt[d][c] = it->second;
    }
  }
  const int nd = (int)sets.size();

  // trim: every state is reachable by construction; keep those from which an accepting state is reachable
  std::vector<char> live(nd, 0);
  {
    std::vector<std::vector<int>> back(nd);
    for (int s = 0; s < nd; ++s) for (int c = 1; c <= 94; ++c) if (dt[s][c] >= 0) back[dt[s][c]].push_back(s);
    std::vector<int> stack;
    for (int s = 0; s < nd; ++s) if (acc[s]) { live[s] = 1; stack.push_back(s); }
    while (!stack.empty()) {
      const int s = stack.back(); stack.pop_back();
      for (int r : back[s]) if (!live[r]) { live[r] = 1; stack.push_back(r); }
    }
  }
  if (!live[0]) throw std::runtime_error(std::string("pattern: the language of \"") + src + "\" is empty" + (mask ? " under the character set in force" : "") + ": 0 texts match");
  for (int s = 0; s < nd; ++s) for (int c = 1; c <= 94; ++c) if (dt[s][c] >= 0 && !live[dt[s][c]]) dt[s][c] = -1;

  // Moore: refine {accepting, not} by the blocks of the successors until nothing splits (a missing transition is block -1)
  std::vector<int> block(nd, -1);
  int nb = 0;
  {
    int ba = -1, bn = -1;
    for (int s = 0; s < nd; ++s) if (live[s]) block[s] = acc[s] ? (ba < 0 ? (ba = nb++) : ba) : (bn < 0 ? (bn = nb++) : bn);
  }
  for (;;) {
    std::map<std::vector<int>, int> sig;
    std::vector<int> next(nd, -1);
    for (int s = 0; s < nd; ++s) {
      if (!live[s]) continue;
      std::vector<int> k(kPatCols);
      k[0] = block[s];
      for (int c = 1; c <= 94; ++c) k[c] = dt[s][c] >= 0 ? block[dt[s][c]] : -1;
      k[95] = 0;
      auto it = sig.find(k);
      if (it == sig.end()) it = sig.emplace(std::move(k), (int)sig.size()).first;
      next[s] = it->second;
    }
    const int n2 = (int)sig.size();
    block.swap(next);
    if (n2 == nb) break;
    nb = n2;
  }
  if (nb > kPatMaxStates) throw std::runtime_error("pattern: its minimal automaton has " + std::to_string(nb) + " states: at most 256");

  // number the blocks breadth first from the start, in class order
  std::vector<int> rep(nb, -1), order(nb, -1);
  for (int s = 0; s < nd; ++s) if (live[s] && rep[block[s]] < 0) rep[block[s]] = s;
  std::vector<int> queue{block[0]};
  order[block[0]] = 0;
  for (size_t q = 0; q < queue.size(); ++q) {
    const int s = rep[queue[q]];
    for (int c = 1; c <= 94; ++c) {
      if (dt[s][c] < 0) continue;
      const int b = block[dt[s][c]];
      if (order[b] < 0) { order[b] = (int)queue.size(); queue.push_back(b); }
    }
  }

  Pattern p;
  p.src = src;
  if (mask) for (int i = 0; i < 3; ++i) p.mask[i] = mask[i];
  p.states = nb; p.start = 0; p.done = nb;
  p.delta.assign((size_t)(nb + 1) * kPatCols, (uint16_t)kPatNone);
  p.mind.assign(nb + 1, 0);
  for (int b = 0; b < nb; ++b) {
    const int s = rep[b], r = order[b];
    if (acc[s]) p.delta[(size_t)r * kPatCols] = (uint16_t)p.done;
    for (int c = 1; c <= 94; ++c) if (dt[s][c] >= 0) p.delta[(size_t)r * kPatCols + c] = (uint16_t)order[block[dt[s][c]]];
  }
  // mind: breadth first backwards from the accepting states
  {
    std::vector<int> dist(nb, -1);
    std::vector<std::vector<int>> back(nb);
    for (int r = 0; r < nb; ++r) for (int c = 1; c <= 94; ++c) { const int t = p.delta[(size_t)r * kPatCols + c]; if (t != kPatNone) back[t].push_back(r); }
    std::vector<int> q;
    for (int r = 0; r < nb; ++r) if (p.delta[(size_t)r * kPatCols] != kPatNone) { dist[r] = 0; q.push_back(r); }
    for (size_t k = 0; k < q.size(); ++k) for (int r : back[q[k]]) if (dist[r] < 0) { dist[r] = dist[q[k]] + 1; q.push_back(r); }
    for (int r = 0; r < nb; ++r) p.mind[r] = (uint8_t)std::min(dist[r], 254);
  }
  fill_done(p, mask_set(mask));
  if (p.mind[p.start] > kPatMaxChars)
    throw std::runtime_error(std::string("pattern: the shortest text that matches \"") + src + "\" has " + std::to_string((int)p.mind[p.start]) + " characters: the recogniser returns at most 25");
  return p;
}

int pattern_matches(const Tokenizer& tok, const Pattern& p, const char* text) {
  if (!text) return -1;
  // a byte may name two classes (the backslash): follow every state they lead to
  std::vector<int> cur{p.start};
  bool dead = false;
  for (const char* q = text; *q; ++q) {
    const ClassSet cs = classes_of(tok, (unsigned char)*q);
    if (cs.none()) return -1;
    if (dead) continue;
    std::vector<int> next;
    for (int s : cur) {
      if (s == p.done) continue;
      for (int c = 1; c <= 94; ++c) {
        if (!cs.test(c)) continue;
        const int t = p.delta[(size_t)s * kPatCols + c];
        if (t != kPatNone && std::find(next.begin(), next.end(), t) == next.end()) next.push_back(t);
      }
    }
    cur.swap(next);
    dead = cur.empty();
  }
  if (dead) return 0;
  for (int s : cur) if (s != p.done && p.delta[(size_t)s * kPatCols] != kPatNone) return 1;
  return 0;
}

int pattern_best_from_lp(const Pattern& p, const float* lp, int32_t* path, int32_t* len, float* logp) {
  constexpr int kLevels = kPatMaxChars + 1;   // V[L]: the best score of L characters that end in a state
  const int S = p.states;
  if (path) std::fill(path, path + kLevels, 0);
  if (len) *len = -1;
  if (logp) *logp = -INFINITY;
  if (S <= 0) return 1;                        // a DONE state alone: no language to choose from
  std::vector<float> V((size_t)kLevels * S, -INFINITY);
  std::vector<uint16_t> bc((size_t)kLevels * S, 0), bs((size_t)kLevels * S, 0);
  V[(size_t)p.start] = 0.0f;
  float best = -INFINITY; int best_l = -1, best_s = -1;
  for (int l = 0; l < kLevels; ++l) {
    const float* row = lp + (size_t)l * kPatCols;
    for (int s = 0; s < S; ++s) {
      const float vs = V[(size_t)l * S + s];
      if (!(vs > -INFINITY)) continue;         // (never reached; a NaN is never chosen below, so none is stored)
      if (p.delta[(size_t)s * kPatCols] != kPatNone) {   // s accepts: the word of l characters that ends here, and the EOS behind it
        const float f = (vs + row[0]) + 0.0f;    // (+ 0.0f: -0.0f becomes +0.0f, as in pattern_best_kernel, whose keys tell the two apart)
        if (f > best) { best = f; best_l = l; best_s = s; }   // (l, then s ascending: an equal score later never replaces)
      }
      if (l == kPatMaxChars) continue;
      for (int c = 1; c <= 94; ++c) {
        const int t = p.delta[(size_t)s * kPatCols + c];
        if (t == kPatNone) continue;
        const float v = (vs + row[c]) + 0.0f;
        if (!(v > -INFINITY)) continue;        // -inf and NaN are never chosen
        const size_t o = (size_t)(l + 1) * S + t;
        if (v > V[o] || (v == V[o] && (c < bc[o] || (c == bc[o] && s < bs[o])))) { V[o] = v; bc[o] = (uint16_t)c; bs[o] = (uint16_t)s; }
      }
    }
  }
  if (best_l < 0) return 1;
  if (len) *len = best_l;
  if (logp) *logp = best;
  if (path)
    for (int l = best_l, s = best_s; l > 0; --l) {
      const size_t o = (size_t)l * S + s;
      path[l - 1] = bc[o];
      s = bs[o];
    }
  return 0;
}

int PatternTable::add(const Pattern& p, const char* what) {
  const int base = rows(), total = base + p.rows();
  if (total > kPatMaxTable) throw std::runtime_error(std::string(what) + ": the call's patterns need " + std::to_string(total) + " automaton states in all: at most 1024 fit one table");
  delta.resize((size_t)total * kPatCols);
  mind.resize(total);
  for (int r = 0; r < p.rows(); ++r) {
    mind[base + r] = p.mind[r];
    for (int c = 0; c < kPatCols; ++c) {
      const int t = p.delta[(size_t)r * kPatCols + c];
      delta[(size_t)(base + r) * kPatCols + c] = (uint16_t)(t == kPatNone ? kPatNone : t + base);
    }
  }
  return base + p.start;
}

}  // namespace ttr
