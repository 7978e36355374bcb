"""numpy restatement of the fuzzy alignment of lexicon entries (DESIGN.md "Lexicon matching", Fuzzy alignment): the rule cell by cell with np.float32
scalars - every operation one fp32 addition or one comparison, as the library's - and the same recurrence in float64 with the rounding bound of the path
it chooses.  Pure numpy; the tests compare the library against it."""
import numpy as np

N_POS, MAX_LEN = 26, 25
GAP = np.float32(-6.9077554)          # ln 1e-3, the convenience layers' default


def _take(cur, cand):
    """the replacement rule: a greater score, or an equal one with fewer edits (a comparison with NaN is false)"""
    return cand if cand[0] > cur[0] or (cand[0] == cur[0] and cand[1] < cur[1]) else cur


def align(lp, record, band, gap, dtype=np.float32, mag=None):
    """One record u8 [32] against one table lp [26, >= 95] -> (score, edits, terms, magsum): the winner of the end rule; terms = table entries on the winning
    path (the EOS included), magsum = the sum of mag over them (0 without mag).  dtype: np.float32 (the rule itself) or np.float64."""
    f = dtype
    L = int(record[0])
    assert 1 <= L <= MAX_LEN and 0 <= band <= 3
    w = [int(c) for c in record[1:1 + L]]
    g, ag = f(gap), abs(float(gap))
    none = (f(-np.inf), 0, 0, 0.0)
    m = (lambda p, c: float(mag[p, c])) if mag is not None else (lambda p, c: 0.0)
    D = {}
    with np.errstate(all="ignore"):
        for j in range(L + 1):
            for p in range(N_POS):
                if abs(j - p) > band:
                    continue
                if j == 0 and p == 0:
                    D[0, 0] = (f(0.0), 0, 0, 0.0)
                    continue
                cur = none
                c = D.get((j - 1, p - 1))
                if c is not None:                                  # match
                    cur = _take(cur, (c[0] + f(lp[p - 1, w[j - 1]]), c[1], c[2] + 1, c[3] + m(p - 1, w[j - 1])))
                c = D.get((j, p - 1))
                if c is not None:                                  # extra character in the reading
                    cur = _take(cur, (c[0] + g, c[1] + 1, c[2], c[3]))
                c = D.get((j - 1, p))
                if c is not None:                                  # dropped character
                    cur = _take(cur, (c[0] + g, c[1] + 1, c[2], c[3]))
                D[j, p] = cur
        best = none
        for p in range(N_POS):
            c = D.get((L, p))
            if c is not None:
                best = _take(best, (c[0] + f(lp[p, 0]), c[1], c[2] + 1, c[3] + m(p, 0)))
    return best


def scores32(lp, records, band, gap):
    """records u8 [n, 32] against one f32 table -> (logp f32 [n], edits i32 [n]), the rule itself"""
    lp = np.asarray(lp, dtype=np.float32)
    out = [align(lp, r, band, gap) for r in np.asarray(records, dtype=np.uint8)]
    return np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.int32)


def scores64(lp64, mag, records, band, gap):
    """the same recurrence in float64 -> (score f64 [n], edits [n], tol f64 [n]): tol = lexicon_ref.scores' path bound on the path float64 chooses - 2.5e-6
    per table entry + 2^-19 * the entries' magnitudes - plus 2^-19 |g| per edit (one rounding of an addition of g against the running sum)."""
    out = [align(lp64, r, band, gap, np.float64, mag) for r in np.asarray(records, dtype=np.uint8)]
    s = np.array([o[0] for o in out], np.float64)
    e = np.array([o[1] for o in out], np.int64)
    tol = np.array([o[2] * 2.5e-6 + 2.0 ** -19 * o[3] + o[1] * 2.0 ** -19 * abs(float(gap)) for o in out])
    return s, e, tol


def rigid32(lp, record):
    """the rigid scorer's chain: the sum in position order from 0.0f of lp[p][w_p], p < L, then + lp[L][0]"""
    lp = np.asarray(lp, dtype=np.float32)
    s = np.float32(0.0)
    with np.errstate(all="ignore"):
        for p in range(int(record[0]) + 1):
            s = s + lp[p, int(record[1 + p])]
    return s
