"""numpy restatement of the character alternatives (DESIGN.md "Character alternatives"): the top-k rule on logits, and the n-best rule on one word's
alternatives in two forms - brute force over every rank tuple, and the best-first walk.  Pure numpy; the tests compare the library against it."""
import heapq
import itertools

import numpy as np

N_POS, N_CLS = 26, 95


def allowed_classes(mask=None) -> np.ndarray:
    """uint32 [3] mask (class c = bit c & 31 of word c >> 5; None = every class) -> the allowed classes, ascending"""
    if mask is None:
        return np.arange(N_CLS)
    m = [int(v) for v in np.asarray(mask).ravel()[:3]]
    return np.array([c for c in range(N_CLS) if (m[c >> 5] >> (c & 31)) & 1], dtype=np.int64)


def topk(logits, k: int, masks=None):
    """logits f32 [n, 26, 95]; masks None, one uint32 [3] mask, or uint32 [n, 3] (one per crop) -> (alt_ids i64 [n, 26, k], alt_prob f64 [n, 26, k], d f64
    [n, 26, k] = x[alt_id] - x[id]).  Ids: the allowed classes by np.argsort(-x, kind="stable") - descending fp32 logit, ties to the lower class -, -1 where
    fewer than k are allowed.  Probabilities in float64: exp(x[c] - x[id]) / sum over the allowed classes of exp(x - x[id]); 0 in the empty slots."""
    x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, N_POS, N_CLS)
    n = len(x)
    ids = np.full((n, N_POS, k), -1, np.int64)
    prob = np.zeros((n, N_POS, k), np.float64)
    d = np.zeros((n, N_POS, k), np.float64)
    masks = None if masks is None else np.asarray(masks, dtype=np.uint32)
    for i in range(n):
        cls = allowed_classes(None if masks is None else (masks if masks.ndim == 1 else masks[i]))
        for p in range(N_POS):
            row = x[i, p, cls]
            order = np.argsort(-row, kind="stable")[:k]
            r64 = row.astype(np.float64)
            s = np.exp(r64 - r64[order[0]]).sum()
            m = len(order)
            ids[i, p, :m] = cls[order]
            d[i, p, :m] = r64[order] - r64[order[0]]
            prob[i, p, :m] = np.exp(d[i, p, :m]) / s
    return ids, prob, d


def is_char(c: int) -> bool:
    return 1 <= c < 95 and c != 88


def _word(alt_ids, alt_prob):
    """-> (S, options per position of S as slot lists in rank order, e or None); probabilities stay float32"""
    ids = np.asarray(alt_ids)
    pr = np.asarray(alt_prob, dtype=np.float32)
    assert ids.shape == pr.shape and ids.shape[0] == N_POS
    eos = np.nonzero(ids[:, 0] == 0)[0]
    e = int(eos[0]) if len(eos) else None
    S = [p for p in range(N_POS if e is None else e) if is_char(int(ids[p, 0]))]
    opts = []
    for p in S:
        slots = [j for j in range(ids.shape[1]) if is_char(int(ids[p, j]))]
        slots.sort(key=lambda j: -float(pr[p, j]))           # stable: (prob descending, slot ascending)
        opts.append(slots)
    return S, opts, e


def _reading(ids, pr, S, opts, e, ranks, itos):
    c = np.float32(1.0)
    for p, o, r in zip(S, opts, ranks):
        c = np.float32(c * pr[p, o[r]])                      # the fp32 product, in position order from 1.0f
    if e is not None:
        c = np.float32(c * pr[e, 0])
    return "".join(itos[int(ids[p, o[r]])] for p, o, r in zip(S, opts, ranks)), c


def nbest_brute(alt_ids, alt_prob, m: int, itos):
    """every rank tuple, sorted by (score descending, tuple ascending) -> [(text, score f32, ranks)] (small words only: prod(len(options)) tuples)"""
    ids, pr = np.asarray(alt_ids), np.asarray(alt_prob, dtype=np.float32)
    S, opts, e = _word(ids, pr)
    out = []
    for ranks in itertools.product(*[range(len(o)) for o in opts]):
        t, c = _reading(ids, pr, S, opts, e, ranks, itos)
        out.append((t, c, tuple(ranks)))
    out.sort(key=lambda r: (-float(r[1]), r[2]))
    return out[:m]


def nbest_walk(alt_ids, alt_prob, m: int, itos):
    """the best-first walk over "raise one position's rank by one" -> (the same list, the number of tuples pushed)"""
    ids, pr = np.asarray(alt_ids), np.asarray(alt_prob, dtype=np.float32)
    S, opts, e = _word(ids, pr)
    zero = (0,) * len(S)
    heap = [(-float(_reading(ids, pr, S, opts, e, zero, itos)[1]), zero)]
    seen, out, pushed = {zero}, [], 1
    while heap and len(out) < m:
        _, ranks = heapq.heappop(heap)
        t, c = _reading(ids, pr, S, opts, e, ranks, itos)
        out.append((t, c, ranks))
        for i in range(len(S)):
            if ranks[i] + 1 < len(opts[i]):
                nx = ranks[:i] + (ranks[i] + 1,) + ranks[i + 1:]
                if nx not in seen:
                    seen.add(nx)
                    heapq.heappush(heap, (-float(_reading(ids, pr, S, opts, e, nx, itos)[1]), nx))
                    pushed += 1
    return out, pushed


def char_options(alt_ids, alt_prob, itos):
    """one list per character of the text: [(char, prob f32), ...] over that position's character options in rank order"""
    ids, pr = np.asarray(alt_ids), np.asarray(alt_prob, dtype=np.float32)
    S, opts, _ = _word(ids, pr)
    return [[(itos[int(ids[p, j])], float(pr[p, j])) for j in o] for p, o in zip(S, opts)]
