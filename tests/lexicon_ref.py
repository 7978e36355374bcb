"""numpy float64 restatement of lexicon matching (DESIGN.md "Lexicon matching"): the records' encoding, the score of every word under a class mask, its
rounding bound, and the ranking.  Pure numpy; the tests compare the library against it."""
import numpy as np

N_POS, N_CLS, MAX_LEN, RECORD = 26, 95, 25, 32


def class_of(itos) -> dict:
    """character -> its one class in [1, 95) other than 88; a character the table lists twice (the backslash: ids 69 and 87) names none"""
    seen = {}
    for i in range(1, N_CLS):
        if i != 88:
            seen.setdefault(itos[i], []).append(i)
    return {ch: v[0] for ch, v in seen.items() if len(v) == 1 and ch != "]"}


def encode(words, itos) -> np.ndarray:
    """u8 [n, 32]: byte 0 the length, bytes 1..L the classes, zeros behind"""
    cls = class_of(itos)
    rec = np.zeros((len(words), RECORD), np.uint8)
    for i, w in enumerate(words):
        assert 1 <= len(w) <= MAX_LEN
        rec[i, 0] = len(w)
        rec[i, 1:1 + len(w)] = [cls[ch] for ch in w]
    return rec


def allowed(mask=None) -> np.ndarray:
    """uint32 [3] mask (class c = bit c & 31 of word c >> 5; None = every class) -> bool [95]"""
    if mask is None:
        return np.ones(N_CLS, bool)
    m = [int(v) for v in np.asarray(mask).ravel()[:3]]
    return np.array([bool((m[c >> 5] >> (c & 31)) & 1) for c in range(N_CLS)])


def tables(logits, masks=None):
    """logits f32 [n, 26, 95]; masks None, one uint32 [3] mask, or uint32 [n, 3] -> (lp f64 [n, 26, 95], mag f64 [n, 26, 95]): lp[p][c] = (x[c] - x[id]) +
    log(prob) for an allowed class (id the first maximum among the allowed, prob = 1 / sum over the allowed of exp(x - x[id])), -inf for a blocked one;
    mag = |x[c] - x[id]| + |log prob|, what the rounding bound weighs (inf where lp is -inf or NaN)."""
    x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, N_POS, N_CLS).astype(np.float64)
    n = len(x)
    masks = None if masks is None else np.asarray(masks, dtype=np.uint32)
    lp = np.full((n, N_POS, N_CLS), -np.inf)
    mag = np.full((n, N_POS, N_CLS), np.inf)
    with np.errstate(all="ignore"):
        for i in range(n):
            ok = allowed(None if masks is None else (masks if masks.ndim == 1 else masks[i]))
            for p in range(N_POS):
                row = np.where(ok, x[i, p], -np.inf)
                xid = row[int(np.argmax(row))]
                d = row - xid
                logprob = -np.log(np.exp(d[ok]).sum())
                lp[i, p, ok] = d[ok] + logprob
                mag[i, p, ok] = np.abs(d[ok]) + abs(logprob)
    bad = ~np.isfinite(lp)
    lp[bad] = -np.inf
    mag[bad] = np.inf
    return lp, mag


def scores(records, lp, mag):
    """records u8 [V, 32], lp / mag [n, 26, 95] -> (score f64 [n, V], tol f64 [n, V]): score = sum over p < L of lp[p][w_p], + lp[L][0];
    tol = (L + 1) * 2.5e-6 + 2^-19 * the same sum over mag - the fp32 path's distance from float64 (prob within 2e-6 relative, logf within two ulp, one
    rounding per subtraction and per addition against the running magnitude)."""
    rec = np.asarray(records, dtype=np.uint8)
    L = rec[:, 0].astype(np.int64)
    cls = rec[:, 1:1 + N_POS].astype(np.int64)                          # [V, 26]: the padding reads as class 0, the EOS
    use = np.arange(N_POS)[None, :] <= L[:, None]                       # positions 0..L
    n = len(lp)
    s = np.zeros((n, len(rec)))
    t = np.zeros((n, len(rec)))
    with np.errstate(all="ignore"):
        for p in range(N_POS):
            u = use[:, p]
            s[:, u] += lp[:, p, cls[u, p]]
            t[:, u] += mag[:, p, cls[u, p]]
    s[~np.isfinite(s)] = -np.inf
    tol = (L + 1)[None, :] * 2.5e-6 + 2.0 ** -19 * t
    return s, tol


def rank(score_row, m: int):
    """one crop's scores f64 [V] -> the indices of its m best words by (score descending, index ascending), words of score -inf left out"""
    order = np.lexsort((np.arange(len(score_row)), -score_row))
    order = order[np.isfinite(score_row[order])]
    return order[:m]
