"""Reference for character sets (DESIGN.md "Character sets"), written independently of the engine: the mask rule against an itos table, the
masked decode in float64, and the oracle's PARSeq forward restated with the masked argmax in its two places (it imports oracle.models and does
not edit it)."""
from __future__ import annotations

import numpy as np

N_CLS = 95
FULL = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0x7FFFFFFF], np.uint32)


def mask_rule(itos, allow=None, deny=None) -> np.ndarray:
    """uint32 [3]: bit 0 (EOS) always; bit i (1 <= i <= 94) iff itos[i] occurs in allow (None / "" = every character) and not in deny (None / "" = none).
    ValueError, naming the character, when a list holds a character that is at no index 1..94, or when only EOS is left."""
    chars = [itos[i] for i in range(N_CLS)]
    for name, lst in (("allow", allow), ("deny", deny)):
        for ch in lst or "":
            if ch not in chars[1:]:
                raise ValueError(f"{name} holds {ch!r}, which names no class")
    m = np.zeros(3, np.uint32)
    m[0] = 1
    n = 0
    for i in range(1, N_CLS):
        if (not allow or chars[i] in allow) and not (deny and chars[i] in deny):
            m[i >> 5] |= np.uint32(1 << (i & 31))
            n += 1
    if n == 0:
        raise ValueError("only EOS is left")
    return m


def allowed(mask) -> np.ndarray:
    """bool [95] from the three words"""
    mask = np.asarray(mask, np.uint32)
    return np.array([(int(mask[c >> 5]) >> (c & 31)) & 1 for c in range(N_CLS)], bool)


def confidence64(ids, prob):
    """The confidence rule (DESIGN.md "Recognition confidence") in float64: the product over the positions before the first EOS whose id is kept by the
    decoder (not 88, inside [0, 98)), times the EOS's probability when there is one."""
    c = 1.0
    for i, p in zip(ids, prob):
        if i == 0:
            c *= float(p)
            break
        if i == 88 or i < 0 or i >= 98:
            continue
        c *= float(p)
    return c


def masked_decode(logits, mask):
    """float64: ids [n, 26] = the first maximal index among the allowed classes, prob [n, 26] = 1 / sum over allowed c of exp(x[c] - x[id]),
    conf [n] = the confidence product."""
    a = allowed(mask)
    x = np.asarray(logits).astype(np.float64).reshape(-1, 26, N_CLS)
    xm = np.where(a[None, None, :], x, -np.inf)
    ids = xm.argmax(-1)                                    # numpy: the first maximal index
    mx = xm.max(-1, keepdims=True)
    prob = 1.0 / np.exp(xm - mx).sum(-1)
    conf = np.array([confidence64(i, p) for i, p in zip(ids, prob)], np.float64)
    return ids, prob, conf


def gap2(logits, mask) -> np.ndarray:
    """[n, 26] float64: the gap between the two best allowed classes"""
    a = allowed(mask)
    x = np.asarray(logits).astype(np.float64)[..., a]
    s = np.sort(x, -1)
    return s[..., -1] - s[..., -2] if x.shape[-1] > 1 else np.full(x.shape[:-1], np.inf)


def masked_forward(parseq, images, mask):
    """oracle.models.PARSeq.forward (early_exit = False, return_ar = True) with the masked argmax where it chooses tokens: the AR loop's next token and
    the refinement pass's input.  images: float tensor [N, 3, 32, 128].  Returns (refined logits, AR logits), both untouched by the mask itself: with a
    full mask they are the plain forward's bit for bit."""
    import torch
    blocked = torch.from_numpy(~allowed(mask))

    def choose(p):                                        # p [..., 95]
        return p.masked_fill(blocked, float("-inf")).argmax(-1)

    with torch.no_grad():
        bs = images.shape[0]
        num_steps = parseq.max_label_length + 1
        memory = parseq.encode(images)
        pos_queries = parseq.pos_queries[:, :num_steps].expand(bs, -1, -1)
        tgt_mask = query_mask = torch.triu(torch.full((num_steps, num_steps), float("-inf")), 1)
        tgt_in = torch.full((bs, num_steps), parseq.PAD, dtype=torch.long)
        tgt_in[:, 0] = parseq.BOS
        logits = []
        for i in range(num_steps):
            j = i + 1
            tgt_out = parseq.decode(tgt_in[:, :j], memory, tgt_mask[:j, :j], tgt_query=pos_queries[:, i:j], tgt_query_mask=query_mask[i:j, :j])
            p_i = parseq.head(tgt_out)
            logits.append(p_i)
            if j < num_steps:
                tgt_in[:, j] = choose(p_i.squeeze(1))
        logits = torch.cat(logits, dim=1)
        ar_logits = logits
        query_mask = query_mask.clone()
        query_mask[torch.triu(torch.ones(num_steps, num_steps, dtype=torch.bool), 2)] = 0
        bos = torch.full((bs, 1), parseq.BOS, dtype=torch.long)
        tgt_in = torch.cat([bos, choose(logits[:, :-1])], dim=1)
        tgt_padding_mask = (tgt_in == parseq.EOS).int().cumsum(-1) > 0
        tgt_out = parseq.decode(tgt_in, memory, tgt_mask[: tgt_in.shape[1], : tgt_in.shape[1]], tgt_padding_mask,
                                tgt_query=pos_queries, tgt_query_mask=query_mask[:, : tgt_in.shape[1]])
        return parseq.head(tgt_out), ar_logits


def crops_to_images(crops):
    """u8 [N, 32, 128, 3] -> the oracle's input (tests/parity_rules.py: oracle_logits)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(crops)).permute(0, 3, 1, 2).float().div(255.0)


_memo = {}


def masked_oracle_logits(parseq, crops, mask):
    """(refined, AR) float32 [N, 26, 95] of masked_forward on the whole batch, memoised per (model, crops, mask): the tests that share a case compute it once"""
    import hashlib
    key = (id(parseq), crops.shape, hashlib.sha1(np.ascontiguousarray(crops).tobytes()).hexdigest(), tuple(int(v) for v in mask))
    if key not in _memo:
        r, a = masked_forward(parseq, crops_to_images(crops), mask)
        _memo[key] = (r.numpy(), a.numpy())
    r, a = _memo[key]
    return r.copy(), a.copy()


def sweep_crops(seed: int, n: int = 48) -> np.ndarray:
    """n crops from default_rng(seed): uniform noise for all n drawn first, then the second half overwritten with dark strokes on light paper
    (tests/test_gpu_x4_parity.py: test_x4_parseq_seed_sweep's recipe)"""
    rng = np.random.default_rng(seed)
    crops = rng.integers(0, 256, (n, 32, 128, 3), dtype=np.uint8)
    for i in range(n // 2, n):
        img = np.full((32, 128, 3), int(rng.integers(200, 256)), np.uint8)
        for _ in range(int(rng.integers(2, 10))):
            x, w, y, h = int(rng.integers(2, 118)), int(rng.integers(2, 9)), int(rng.integers(3, 14)), int(rng.integers(8, 18))
            img[y:y + h, x:x + w] = rng.integers(0, 90, (1, 1, 3), dtype=np.uint8)
        crops[i] = img
    return crops


def upto_first_eos(choices) -> np.ndarray:
    """[N, L] ids -> bool [N, L]: positions up to and including the first EOS (all of them when there is none)"""
    choices = np.asarray(choices)
    has = (choices == 0).any(1)
    up = np.where(has, (choices == 0).argmax(1) + 1, choices.shape[1])
    return np.arange(choices.shape[1])[None, :] < up[:, None]


def left_out(ref, ref_ar, mask, tau: float = 2e-3) -> np.ndarray:
    """bool [N]: the oracle's gap between its two best allowed classes is below tau at any refined position, or at any AR position up to the AR EOS"""
    ar_choice, _, _ = masked_decode(ref_ar, mask)
    near_rf = (gap2(ref, mask) < tau).any(1)
    near_ar = ((gap2(ref_ar, mask) < tau) & upto_first_eos(ar_choice)).any(1)
    return near_rf | near_ar
