"""Reference for patterns (DESIGN.md "Patterns"), written independently of the engine: the pattern language to a minimal DFA and `mind` by Brzozowski
derivatives (the engine goes through a Thompson NFA and the subset construction), the choice rule, the float64 sequential decode under it, and the oracle's
PARSeq forward restated with the sequential choice in its AR loop (it imports oracle.models through the caller's model and does not edit it)."""
from __future__ import annotations

import numpy as np

from tests import charset_ref as CR

N_CLS = 95
NONE = 0xFFFF
FREE = 255
MAX_CHARS = 25
USABLE = [c for c in range(1, 95) if c != 88]


# --------------------------------------------------------------------------------------------------------------- the language
def _classes(itos, ch):
    return frozenset(c for c in USABLE if itos[c] == ch)


class _Parser:
    """pattern -> a term: ("nil",) the empty language, ("eps",), ("set", frozenset), ("cat", a, b), ("alt", frozenset), ("star", a), ("rep", a, lo, hi)"""

    def __init__(self, itos, s):
        self.itos, self.s, self.i = itos, s, 0
        self.dot = frozenset(USABLE)
        self.digit = frozenset(c for c in USABLE if itos[c].isdigit() and itos[c].isascii())
        self.word = frozenset(c for c in USABLE if (itos[c].isalnum() and itos[c].isascii()) or itos[c] == "_")

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else None

    def lit(self, ch):
        cs = _classes(self.itos, ch)
        if not cs:
            raise ValueError(f"{ch!r} names no class")
        return cs

    def esc(self):
        self.i += 1
        ch = self.peek()
        if ch is None:
            raise ValueError("dangling backslash")
        self.i += 1
        if ch == "d":
            return self.digit, True
        if ch == "w":
            return self.word, True
        if ch.isalnum():
            raise ValueError(f"unknown escape \\{ch}")
        return self.lit(ch), False

    def alt(self):
        parts = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            parts.append(self.cat())
        return mk_alt(parts)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.quant())
        t = ("eps",)
        for it in reversed(items):
            t = mk_cat(it, t)
        return t

    def quant(self):
        a = self.atom()
        ch = self.peek()
        if ch is None or ch not in "?*+{":
            return a
        self.i += 1
        if ch == "?":
            t = mk_rep(a, 0, 1)
        elif ch == "*":
            t = mk_star(a)
        elif ch == "+":
            t = mk_cat(a, mk_star(a))
        else:
            j = self.s.index("}", self.i)
            body = self.s[self.i:j]
            self.i = j + 1
            if "," in body:
                lo, hi = body.split(",")
                lo, hi = int(lo), (int(hi) if hi else None)
            else:
                lo = hi = int(body)
            if lo > MAX_CHARS or (hi is not None and not lo <= hi <= MAX_CHARS):
                raise ValueError("quantifier out of range")
            t = mk_cat(mk_rep(a, lo, lo), mk_star(a)) if hi is None else mk_rep(a, lo, hi)
        if self.peek() is not None and self.peek() in "?*+{":
            raise ValueError("stacked quantifier")
        return t

    def atom(self):
        ch = self.peek()
        if ch in "?*+{":
            raise ValueError("nothing to repeat")
        if ch == "(":
            self.i += 1
            t = self.alt()
            if self.peek() != ")":
                raise ValueError("unbalanced (")
            self.i += 1
            return t
        if ch == "[":
            return self.cset()
        if ch == ".":
            self.i += 1
            return ("set", self.dot)
        if ch == "\\":
            return ("set", self.esc()[0])
        if ch in "^$":
            raise ValueError("anchor")
        self.i += 1
        return ("set", self.lit(ch))

    def cset(self):
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        members, first = set(), True
        while True:
            ch = self.peek()
            if ch is None:
                raise ValueError("unbalanced [")
            if ch == "]":
                if first:
                    raise ValueError("empty set")
                self.i += 1
                break
            first = False
            if ch == "\\":
                cs, is_class = self.esc()
                lo = None if is_class else self.s[self.i - 1]
            else:
                cs, lo = self.lit(ch), ch
                self.i += 1
            if lo is not None and self.peek() == "-" and self.i + 1 < len(self.s) and self.s[self.i + 1] != "]":
                self.i += 1
                hi = self.peek()
                if hi == "\\":
                    _, is_class = self.esc()
                    if is_class:
                        raise ValueError("class escape in a range")
                    hi = self.s[self.i - 1]
                else:
                    self.i += 1
                if ord(hi) < ord(lo):
                    raise ValueError("range runs backwards")
                for o in range(ord(lo), ord(hi) + 1):
                    members |= self.lit(chr(o))
            else:
                members |= cs
        return ("set", self.dot - members if neg else frozenset(members))


def mk_cat(a, b):
    if a == ("nil",) or b == ("nil",):
        return ("nil",)
    if a == ("eps",):
        return b
    if b == ("eps",):
        return a
    if a[0] == "cat":                                  # right-nested, so that equal languages meet in equal terms more often
        return mk_cat(a[1], mk_cat(a[2], b))
    return ("cat", a, b)


def mk_alt(parts):
    flat = set()
    for p in parts:
        if p[0] == "alt":
            flat |= p[1]
        elif p != ("nil",):
            flat.add(p)
    if not flat:
        return ("nil",)
    if len(flat) == 1:
        return next(iter(flat))
    return ("alt", frozenset(flat))


def mk_star(a):
    if a in (("nil",), ("eps",)):
        return ("eps",)
    if a[0] == "star":
        return a
    return ("star", a)


def mk_rep(a, lo, hi):
    if hi == 0 or a == ("eps",):
        return ("eps",)
    if a == ("nil",):
        return ("eps",) if lo == 0 else ("nil",)
    if lo == 1 and hi == 1:
        return a
    return ("rep", a, lo, hi)


def nullable(t):
    k = t[0]
    if k in ("eps", "star"):
        return True
    if k in ("nil", "set"):
        return False
    if k == "cat":
        return nullable(t[1]) and nullable(t[2])
    if k == "alt":
        return any(nullable(p) for p in t[1])
    return t[2] == 0 or nullable(t[1])                 # rep


def deriv(t, c, memo):
    key = (t, c)
    if key in memo:
        return memo[key]
    k = t[0]
    if k in ("nil", "eps"):
        r = ("nil",)
    elif k == "set":
        r = ("eps",) if c in t[1] else ("nil",)
    elif k == "cat":
        r = mk_cat(deriv(t[1], c, memo), t[2])
        if nullable(t[1]):
            r = mk_alt([r, deriv(t[2], c, memo)])
    elif k == "alt":
        r = mk_alt([deriv(p, c, memo) for p in t[1]])
    elif k == "star":
        r = mk_cat(deriv(t[1], c, memo), t)
    else:
        r = mk_cat(deriv(t[1], c, memo), mk_rep(t[1], max(t[2] - 1, 0), t[3] - 1))
    memo[key] = r
    return r


class Dfa:
    """delta uint16 [states + 1, 96] and mind uint8 [states + 1] in the engine's table format (row `states` = DONE), built on this file's own route"""

    def __init__(self, delta, mind, start, done, mask):
        self.delta, self.mind, self.start, self.done, self.mask = delta, mind, start, done, mask
        self.states = done


def compile_pattern(itos, pattern, mask=None, limit=20000) -> Dfa:
    """ValueError for a pattern outside the language, an empty language, or a shortest member over 25 characters"""
    if not pattern:
        raise ValueError("empty pattern")
    allowed = CR.allowed(CR.FULL if mask is None else mask)
    classes = [c for c in USABLE if allowed[c]]
    ps = _Parser(itos, pattern)
    term = ps.alt()
    if ps.i != len(pattern):
        raise ValueError("unbalanced )")
    memo = {}
    index, order, trans = {term: 0}, [term], []
    q = 0
    while q < len(order):                               # the derivative automaton: a state is a term
        row = {}
        for c in classes:
            d = deriv(order[q], c, memo)
            if d == ("nil",):
                continue
            if d not in index:
                if len(order) >= limit:
                    raise ValueError("too many states")
                index[d] = len(order)
                order.append(d)
            row[c] = index[d]
        trans.append(row)
        q += 1
    n = len(order)
    acc = [nullable(t) for t in order]
    # co-reachable states only
    live = set(i for i in range(n) if acc[i])
    grew = True
    while grew:
        grew = False
        for s in range(n):
            if s not in live and any(t in live for t in trans[s].values()):
                live.add(s)
                grew = True
    if 0 not in live:
        raise ValueError("empty language")
    trans = [{c: t for c, t in row.items() if t in live} for row in trans]
    # Moore's refinement
    block = {s: int(acc[s]) for s in live}
    while True:
        sig = {}
        nxt = {}
        for s in sorted(live):
            k = (block[s], tuple(sorted((c, block[t]) for c, t in trans[s].items())))
            nxt[s] = sig.setdefault(k, len(sig))
        done = len(sig) == len(set(block.values()))
        block = nxt
        if done:
            break
    # number the blocks breadth first from the start
    rep = {}
    for s in sorted(live):
        rep.setdefault(block[s], s)
    num, queue = {block[0]: 0}, [block[0]]
    for b in queue:
        for c in sorted(trans[rep[b]]):
            t = block[trans[rep[b]][c]]
            if t not in num:
                num[t] = len(queue)
                queue.append(t)
    S = len(queue)
    delta = np.full((S + 1, 96), NONE, np.uint16)
    for b in queue:
        if acc[rep[b]]:
            delta[num[b], 0] = S
        for c, t in trans[rep[b]].items():
            delta[num[b], c] = num[block[t]]
    mind = np.full(S + 1, 254, np.int64)
    mind[[s for s in range(S) if delta[s, 0] != NONE]] = 0
    for _ in range(S):
        for s in range(S):
            ts = delta[s, 1:95]
            ts = ts[ts != NONE]
            if len(ts):
                mind[s] = min(mind[s], 1 + mind[ts].min())
    mind = np.minimum(mind, 254)
    delta[S, 0] = S
    for c in range(1, 95):
        if allowed[c]:
            delta[S, c] = S
    mind[S] = FREE
    if mind[0] > MAX_CHARS:
        raise ValueError(f"the shortest member has {int(mind[0])} characters")
    return Dfa(delta, mind.astype(np.uint8), 0, S, CR.FULL.copy() if mask is None else np.asarray(mask, np.uint32))


def none_pattern(mask=None) -> Dfa:
    """a row without a pattern: a DONE state alone under the mask"""
    allowed = CR.allowed(CR.FULL if mask is None else mask)
    delta = np.full((1, 96), NONE, np.uint16)
    delta[0, :95][allowed] = 0
    return Dfa(delta, np.array([FREE], np.uint8), 0, 0, CR.FULL.copy() if mask is None else np.asarray(mask, np.uint32))


def matches(itos, dfa: Dfa, text) -> bool:
    cur = {dfa.start}
    for ch in text:
        cs = _classes(itos, ch)
        cur = {int(dfa.delta[s, c]) for s in cur if s != dfa.done for c in cs if dfa.delta[s, c] != NONE}
    return any(s != dfa.done and dfa.delta[s, 0] != NONE for s in cur)


# --------------------------------------------------------------------------------------------------------------- the choice rule
def allowed_at(delta, mind, s, p) -> np.ndarray:
    """bool [95]: the classes that may be chosen at character position p in state s"""
    t = delta[s, :95].astype(np.int64)
    ok = t != NONE
    m = np.where(ok, mind[np.where(ok, t, 0)], 0).astype(np.int64)
    budget = (m == FREE) | (p + 1 + m <= MAX_CHARS)
    budget[0] = True
    return ok & budget


def sequential_decode(logits, dfas):
    """float64: logits [n, 26, 95], dfas: one Dfa per row -> ids [n, 26], prob [n, 26], conf [n], and the states walked [n, 27]"""
    x = np.asarray(logits).astype(np.float64).reshape(-1, 26, N_CLS)
    n = len(x)
    ids, prob, states = np.zeros((n, 26), np.int64), np.zeros((n, 26)), np.zeros((n, 27), np.int64)
    for i in range(n):
        d = dfas[i]
        s = d.start
        states[i, 0] = s
        for p in range(26):
            a = allowed_at(d.delta, d.mind, s, p)
            xm = np.where(a, x[i, p], -np.inf)
            c = int(xm.argmax())
            ids[i, p] = c
            prob[i, p] = 1.0 / np.exp(xm - xm[c]).sum()
            s = int(d.delta[s, c])
            states[i, p + 1] = s
    conf = np.array([CR.confidence64(a, b) for a, b in zip(ids, prob)])
    return ids, prob, conf, states


def gap_sequential(logits, dfas, states) -> np.ndarray:
    """[n, 26] float64: the gap between the two best allowed classes at each position, in the given states (inf where one class alone is allowed)"""
    x = np.asarray(logits).astype(np.float64).reshape(-1, 26, N_CLS)
    g = np.full(x.shape[:2], np.inf)
    for i in range(len(x)):
        for p in range(26):
            a = allowed_at(dfas[i].delta, dfas[i].mind, int(states[i, p]), p)
            v = np.sort(x[i, p][a])
            if len(v) > 1:
                g[i, p] = v[-1] - v[-2]
    return g


# --------------------------------------------------------------------------------------------------------------- the oracle under a pattern
def pattern_forward(parseq, images, dfa: Dfa):
    """charset_ref.masked_forward with the sequential choice in the AR loop: the token of step i is the first maximal index among the classes the rule
    allows at position i in the crop's state, which then moves; the refinement pass reads the AR tokens.  Returns (refined logits, AR logits, AR tokens
    [N, 25], AR states [N, 26]); the logits themselves are untouched by the pattern."""
    import torch

    with torch.no_grad():
        bs = images.shape[0]
        num_steps = parseq.max_label_length + 1
        memory = parseq.encode(images)
        pos_queries = parseq.pos_queries[:, :num_steps].expand(bs, -1, -1)
        tgt_mask = query_mask = torch.triu(torch.full((num_steps, num_steps), float("-inf")), 1)
        tgt_in = torch.full((bs, num_steps), parseq.PAD, dtype=torch.long)
        tgt_in[:, 0] = parseq.BOS
        state = np.full(bs, dfa.start, np.int64)
        states = np.zeros((bs, num_steps), np.int64)
        logits = []
        for i in range(num_steps):
            j = i + 1
            tgt_out = parseq.decode(tgt_in[:, :j], memory, tgt_mask[:j, :j], tgt_query=pos_queries[:, i:j], tgt_query_mask=query_mask[i:j, :j])
            p_i = parseq.head(tgt_out)
            logits.append(p_i)
            states[:, i] = state
            if j < num_steps:
                row = p_i.squeeze(1)
                for b in range(bs):
                    a = torch.from_numpy(~allowed_at(dfa.delta, dfa.mind, int(state[b]), i))
                    c = int(row[b].masked_fill(a, float("-inf")).argmax(-1))
                    tgt_in[b, j] = c
                    state[b] = int(dfa.delta[state[b], c])
        logits = torch.cat(logits, dim=1)
        ar_logits = logits
        ar_tokens = tgt_in[:, 1:].clone()
        query_mask = query_mask.clone()
        query_mask[torch.triu(torch.ones(num_steps, num_steps, dtype=torch.bool), 2)] = 0
        tgt_padding_mask = (tgt_in == parseq.EOS).int().cumsum(-1) > 0       # the refinement pass's input: the AR tokens
        tgt_out = parseq.decode(tgt_in, memory, tgt_mask[: tgt_in.shape[1], : tgt_in.shape[1]], tgt_padding_mask,
                                tgt_query=pos_queries, tgt_query_mask=query_mask[:, : tgt_in.shape[1]])
        return parseq.head(tgt_out), ar_logits, ar_tokens.numpy(), states


_memo = {}


def pattern_oracle(parseq, crops, dfa: Dfa, key):
    """(refined, AR, AR tokens, AR states) of pattern_forward on the whole batch, memoised per (model, crops, key)"""
    import hashlib
    k = (id(parseq), crops.shape, hashlib.sha1(np.ascontiguousarray(crops).tobytes()).hexdigest(), key)
    if k not in _memo:
        r, a, t, s = pattern_forward(parseq, CR.crops_to_images(crops), dfa)
        _memo[k] = (r.numpy(), a.numpy(), t, s)
    r, a, t, s = _memo[k]
    return r.copy(), a.copy(), t.copy(), s.copy()


def left_out(ref, ref_ar, ar_tokens, ar_states, dfa: Dfa, tau: float = 2e-3) -> np.ndarray:
    """bool [N]: the oracle's gap between its two best allowed classes is below tau at any refined position (walking the oracle's own refined states), or
    at any AR position up to the AR EOS (in the oracle's own AR states)"""
    n = len(ref)
    dfas = [dfa] * n
    _, _, _, rf_states = sequential_decode(ref, dfas)
    near_rf = (gap_sequential(ref, dfas, rf_states) < tau).any(1)
    g_ar = gap_sequential(ref_ar, dfas, ar_states)[:, :25]                  # the 25 choices the AR loop makes
    near_ar = ((g_ar < tau) & CR.upto_first_eos(ar_tokens)).any(1)
    return near_rf | near_ar
