"""Reference for the best decode of patterns (DESIGN.md "Patterns", the likeliest member), numpy only and independent of the C++: the list-Viterbi in
float64 over tests/pattern_ref.py's own DFA (the two best distinct members, so that the runner-up is known), the fp32 restatement of the rule with its
tie order, the forced-path prob / conf in float64, and an enumerator of a finite language's members.

A table lp is [26, >= 95]: row p = character position p, column 0 = the end of the text, column c = class c.  A member is a tuple of class ids."""
import numpy as np

from tests import charset_ref as CR
from tests import pattern_ref as PR

N_POS, MAX_CHARS = 26, PR.MAX_CHARS


def edges(dfa):
    """the character transitions of the automaton (its DONE state left out): int64 arrays (src, cls, dst), sorted by (src, cls); and bool [states] accepting"""
    S = dfa.states
    d = dfa.delta[:S, :95].astype(np.int64)
    src, cls = np.nonzero(d[:, 1:] != PR.NONE)
    cls = cls + 1
    return src, cls, d[src, cls], d[:, 0] != PR.NONE


def score64(lp, w) -> float:
    """rule 2 in float64: the sum over p < L of lp[p][w_p], then + lp[L][0]; -inf where a term is -inf or NaN"""
    s = sum(float(lp[p][c]) for p, c in enumerate(w)) + float(lp[len(w)][0])
    return s if np.isfinite(s) else -np.inf


def list_viterbi64(lp, dfa):
    """float64 table -> [(score, member), ...]: the best member and the best member distinct from it (fewer when the language has fewer members of finite
    score), best first.  Per (position, state) the two best distinct prefixes are kept; the automaton is deterministic, so distinct paths are distinct texts."""
    lp = np.asarray(lp, dtype=np.float64)
    S = dfa.states
    if S == 0:
        return []
    src, cls, dst, acc = edges(dfa)
    V = np.full((N_POS, S, 2), -np.inf)
    back = np.full((N_POS, S, 2, 3), -1, np.int64)             # (source state, its rank, class)
    V[0, dfa.start, 0] = 0.0
    ends = []                                                  # (score, L, state, rank)
    for L in range(N_POS):
        with np.errstate(all="ignore"):
            f = V[L] + lp[L][0]
        for s in np.nonzero(acc)[0]:
            for r in range(2):
                if np.isfinite(f[s, r]):
                    ends.append((float(f[s, r]), L, int(s), r))
        if L == MAX_CHARS or not len(src):
            continue
        with np.errstate(all="ignore"):
            cand = (V[L][src] + lp[L][cls][:, None]).ravel()  # [E, 2] -> candidate e * 2 + r
        cand[~np.isfinite(cand)] = -np.inf
        d2 = np.repeat(dst, 2)
        order = np.lexsort((-cand, d2))                        # by target, best first
        first = np.r_[True, d2[order][1:] != d2[order][:-1]]
        pos = np.arange(len(order)) - np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))
        for j in np.nonzero((pos < 2) & np.isfinite(cand[order]))[0]:
            k, r = int(order[j]), int(pos[j])
            t = int(d2[k])
            V[L + 1, t, r] = cand[k]
            back[L + 1, t, r] = (src[k // 2], k % 2, cls[k // 2])
    ends.sort(key=lambda e: (-e[0], e[1], e[2], e[3]))
    out = []
    for sc, L, s, r in ends[:2]:
        w = []
        for l in range(L, 0, -1):
            s, r, c = (int(v) for v in back[l, s, r])
            w.append(c)
        out.append((sc, tuple(reversed(w))))
    return out


def viterbi32(lp, dfa):
    """The rule's fp32 restatement: V[0][start] = 0, V[p + 1][t] = max over (s, c >= 1, delta[s][c] == t) of V[p][s] + lp[p][c] in float32, ties to the
    lower class, then the lower state; the end the maximum over (L <= 25, accepting s) of V[L][s] + lp[L][0], ties to the smaller L, then the lower state;
    -inf and NaN are never chosen.  -> (member, float32 score), or None when no member has a finite score."""
    lp = np.asarray(lp, dtype=np.float32)
    S = dfa.states
    if S == 0:
        return None
    src, cls, dst, acc = edges(dfa)
    V = np.full((N_POS, S), -np.inf, np.float32)
    back = np.full((N_POS, S, 2), -1, np.int64)
    V[0, dfa.start] = np.float32(0.0)
    best = None                                                # (score, L, state)
    for L in range(N_POS):
        with np.errstate(all="ignore"):
            f = (V[L] + lp[L][0]).astype(np.float32)
        for s in np.nonzero(acc)[0]:
            if V[L, s] > -np.inf and f[s] > -np.inf and (best is None or f[s] > best[0]):
                best = (f[s], L, int(s))
        if L == MAX_CHARS or not len(src):
            continue
        with np.errstate(all="ignore"):
            cand = (V[L][src] + lp[L][cls]).astype(np.float32)
        ok = (V[L][src] > -np.inf) & (cand > -np.inf)          # (false for NaN)
        e = np.nonzero(ok)[0]
        order = e[np.lexsort((src[e], cls[e], -cand[e].astype(np.float64), dst[e]))]
        first = np.r_[True, dst[order][1:] != dst[order][:-1]] if len(order) else np.zeros(0, bool)
        for k in order[first]:
            V[L + 1, dst[k]] = cand[k]
            back[L + 1, dst[k]] = (src[k], cls[k])
    if best is None:
        return None
    sc, L, s = best
    w = []
    for l in range(L, 0, -1):
        s, c = (int(v) for v in back[l, s])
        w.append(c)
    return tuple(reversed(w)), np.float32(sc)


def forced_decode64(x, dfa, w):
    """float64: one row's logits [26, 95] read along member w - ids [26], prob [26], conf, as the rule's outputs define them: positions 0..L in the states of
    the path (prob = exp(x[id] - max_A) / sum over A of exp(x - max_A), A the classes the choice rule allows), the positions behind L the masked argmax."""
    x = np.asarray(x).astype(np.float64).reshape(N_POS, PR.N_CLS)
    ids, prob = np.zeros(N_POS, np.int64), np.zeros(N_POS)
    s = dfa.start
    forced = list(w) + [0]
    for p in range(N_POS):
        a = PR.allowed_at(dfa.delta, dfa.mind, s, p)
        xm = np.where(a, x[p], -np.inf)
        c = forced[p] if p < len(forced) else int(xm.argmax())
        assert a[c], (p, c)
        ids[p] = c
        prob[p] = np.exp(x[p, c] - xm.max()) / np.exp(xm - xm.max()).sum()
        s = int(dfa.delta[s, c])
    return ids, prob, CR.confidence64(ids, prob)


def members(dfa, limit=200000):
    """every member of the language of at most 25 characters, as tuples of class ids, shortest first; ValueError beyond `limit` members"""
    out, level = [], [((), dfa.start)]
    for L in range(MAX_CHARS + 1):
        out += [w for w, s in level if dfa.delta[s, 0] != PR.NONE]
        if len(out) > limit:
            raise ValueError("the language has too many members to enumerate")
        if L == MAX_CHARS:
            break
        nxt = []
        for w, s in level:
            for c in np.nonzero(dfa.delta[s, 1:95] != PR.NONE)[0] + 1:
                t = int(dfa.delta[s, c])
                if L + 1 + int(dfa.mind[t]) <= MAX_CHARS:
                    nxt.append((w + (int(c),), t))
        if len(nxt) > limit:
            raise ValueError("the language has too many members to enumerate")
        level = nxt
    return out


def greedy32(lp, dfa):
    """the greedy walk on a table (the choice rule on lp itself, first maximal index): the member it reaches - what greedy mode reads when the logits' order
    within every allowed set is the table's"""
    lp = np.asarray(lp, dtype=np.float32)
    s, w = dfa.start, []
    for p in range(N_POS):
        a = PR.allowed_at(dfa.delta, dfa.mind, s, p)
        c = int(np.where(a, lp[p][:95], -np.inf).argmax())
        if c == 0:
            return tuple(w)
        w.append(c)
        s = int(dfa.delta[s, c])
    return tuple(w)
