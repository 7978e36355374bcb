"""The f16x4 attention kernels away from unit scale: inputs, float64 / fp32 references, the intended split arithmetic and the scale families.  TEST
INFRASTRUCTURE ONLY (tests/test_gpu_attn_scale.py, tests/test_attn_scale_cpu.py); numpy / torch, no engine.

The split is NOT restated here: every plane is craft_layer_ref.split_act (the restatement of tuatara_amd/csrc/split.h the detector's and the row kernels' tests
rest on), the bar is craft_layer_ref.bar applied per family through rowops_ref.grouped_bar.  What is stated here:

* ref64 / ref32 - softmax(q k^T / sqrt(dh) [+ mask]) v in float64 and in plain fp32 torch;
* model32       - the INTENDED split arithmetic of the matrix-core kernels (attn_cross_split.hip, attn_split.hip, the attention tile of gemm_sp.hip /
                  qkv_attn4.hip): Q the exact triple, K and V pairs (round-to-nearest where the kernel splits fp32 values itself, the first two planes of the
                  stored triple where it reads those), P the kernel's pair or triple, every lower plane AS STORED at its 2^11 scale with the 2^-11 applied
                  exactly (a power of two: it commutes with every fp32 rounding), fp32 accumulation in the MFMA's order (craft_layer_ref.STEP products per
                  rounding).  No f16 product plane / 2^11 appears in it: that product is subnormal below 2^-3 and is the defect the scale families are there
                  to catch (`down=True` restates it, for the CPU test only);
* the families  - (q, k, v) scalings from unit scale to small K under large Q, small and large V, with random signs per channel and one V channel per head
                  times 64, which is judged as a family of its own (a maximum over both would only see that channel).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import craft_layer_ref as R
from tests import rowops_ref as RO

F32, F64 = np.float32, np.float64
S = 128                               # keys of the encoder's and the cross-attention's geometry
OUTLIER = 64.0

# kind -> (heads, dh, K / V pairs rounded to nearest (else: the first two planes of the stored triple), planes of P)
KINDS = {"cross": (12, 32, True, 2), "fused": (6, 64, True, 2), "split": (6, 64, False, 3)}

# (name, q, k, v scale).  peaky: scores ~ 30.  small K under large Q: plane k0 / 2^11 would be subnormal, the scores are ordinary.  small V: down to the f16
# subnormal range of plane 0 itself (2^-15 N(0,1) < 2^-14).  The last: both.
FAMILIES = (("unit", 1.0, 1.0, 1.0), ("peaky", 6.0, 1.0, 3.0), ("k2^-6_q64", 64.0, 2.0 ** -6, 1.0), ("k2^-10_q1024", 1024.0, 2.0 ** -10, 1.0),
            ("v2^-6", 1.0, 1.0, 2.0 ** -6), ("v2^-10", 1.0, 1.0, 2.0 ** -10), ("v2^-15", 1.0, 1.0, 2.0 ** -15), ("v2^10", 1.0, 1.0, 2.0 ** 10),
            ("k2^-8_v2^-8_q256", 256.0, 2.0 ** -8, 2.0 ** -8))
SMALL_K = ("k2^-6_q64", "k2^-10_q1024", "k2^-8_v2^-8_q256")
SMALL_V = ("v2^-6", "v2^-10", "v2^-15", "k2^-8_v2^-8_q256")


# ---------------------------------------------------------------------------------------------------------------- planes
def _planes(x: np.ndarray, n: int, rn: bool = False):
    """split_act's planes of fp32 x as float64 VALUES (the lower planes' 2^-11 applied, exactly): n = 3 the exact triple, n = 2 the pair - rounded to nearest
    (split2_pair) or the first two planes of the triple (what a kernel reads of stored triples)"""
    parts = R.split_act(torch.from_numpy(np.ascontiguousarray(x, F32)), 2 if (n == 2 and rn) else 3)[:n]
    return [p.numpy().astype(F64) / (1.0 if i == 0 else 2048.0) for i, p in enumerate(parts)]


def as_triple(o: np.ndarray) -> np.ndarray:
    """an fp32 result as the exact triple the kernels store, joined in float64: the value itself wherever the third plane is a normal f16 number, within 2^-36
    otherwise (rowops_ref.split_contract) - the output format is part of the arithmetic, not an allowance on top of the bar"""
    return sum(_planes(o, 3))


def _f16(x: np.ndarray) -> np.ndarray:
    return x.astype(np.float16).astype(F64)


def _mfma(acc: np.ndarray, a: np.ndarray, b: np.ndarray, step: int) -> np.ndarray:
    """acc fp32 [..., M, N] += a [..., M, K] b[..., N, K]^T, `step` products per fp32 rounding (craft_layer_ref.Layer.split_acc: 8 for v_mfma_f32_16x16x32_f16).
    a, b hold f16 numbers times powers of two: a float64 sum of 8 products is exact."""
    for c in range(0, a.shape[-1], step):
        acc = (acc.astype(F64) + a[..., c:c + step] @ np.swapaxes(b[..., c:c + step], -1, -2)).astype(F32)
    return acc


def _lane_sum(e: np.ndarray) -> np.ndarray:
    """the kernels' fp32 row sum of e [..., 128]: lane g adds its keys 32 s + 8 g + e' in sequence, the four lanes join by a butterfly"""
    v = np.swapaxes(e.reshape(e.shape[:-1] + (4, 4, 8)), -3, -2).reshape(e.shape[:-1] + (4, 32))
    a = np.zeros(e.shape[:-1] + (4,), F32)
    for i in range(32):
        a = (a + v[..., i]).astype(F32)
    a = (a + a[..., [1, 0, 3, 2]]).astype(F32)
    return (a + a[..., [2, 3, 0, 1]]).astype(F32)[..., 0]


# ---------------------------------------------------------------------------------------------------------------- the three evaluations
def ref64(q, k, v):
    """q [B, Rq, dh], k, v [B, S, dh] -> float64 [B, Rq, dh]"""
    q, k, v = (np.asarray(t, F64) for t in (q, k, v))
    s = q @ np.swapaxes(k, -1, -2) / math.sqrt(q.shape[-1])
    p = np.exp(s - s.max(-1, keepdims=True))
    return (p / p.sum(-1, keepdims=True)) @ v


def ref32(q, k, v):
    """plain fp32: torch's attention arithmetic"""
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t, F32)) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * F32(1.0 / math.sqrt(q.shape[-1]))
    return (torch.softmax(s, -1) @ v).numpy()


def model32(q, k, v, kind: str, step: int = R.STEP, one_acc: bool = False, down: bool = False, drop_q1: bool = False, p_single: bool = False, k_trunc: bool = False,
            norm_rounded: bool = False):
    """The split arithmetic of the matrix-core kernel `kind` on q [B, Rq, dh], k, v [B, 128, dh] (one head per batch entry; Rq = 128 for the encoder's kinds).

    Scores: per 16-key tile, k0 q0 over the 32-deep d steps into one accumulator, k0 q1 + k0 q2 + k1 q0 into a second, s = fl(hi + lo) (the kernels' fma) - or,
    one_acc, the four products of a d step one after the other into ONE accumulator: the same products in another fp32 summation order (four roundings at the
    score's magnitude per 8 products instead of one), which the bar must not tell from the first (models(): the larger error counts).  The fused tile walks a
    query row's two d halves own half first: half (row >> 4) & 1.  Softmax in fp32, the sum in lane order.  Output: per 32-key step
    v0 p0 + v0 p1 (+ v0 p2) + v1 p0 into one accumulator, times fl(1 / sum), stored as an exact triple (as_triple).
    The flags break it on purpose (tests/test_attn_scale_cpu.py): down = the f16 products k0 / 2^11, k1s / 2^11, v0 / 2^11, v1s / 2^11 and ONE score accumulator
    (implies one_acc: the arithmetic before the fix); drop_q1 = no k0 q1 product; p_single = P as one f16 plane; k_trunc = K's pair by truncation where the kernel rounds;
    norm_rounded = the normaliser summed from P's first plane."""
    heads, dh, rn, pp = KINDS[kind]
    assert q.shape[-1] == dh and k.shape[-2] == S
    q0, q1, q2 = _planes(q, 3)
    k0, k1 = _planes(k, 2, rn and not k_trunc)
    v0, v1 = _planes(v, 2, rn)
    k0lo, v0lo = k0, v0                                       # the operand of the products with a lower plane of the other side
    if down:
        k0lo, k1 = _f16(k0 / 2048.0) * 2048.0, _f16(k1)      # f16(k0 / 2^11) meets q1s = 2^11 q1: (2^11 f16(k0 / 2^11)) q1; k1 = f16(k1s / 2^11)
        v0lo, v1 = _f16(v0 / 2048.0) * 2048.0, _f16(v1)
    B, Rq = q.shape[0], q.shape[1]
    halves = [slice(c, c + 32) for c in range(0, dh, 32)]

    def scores(order):
        hi = np.zeros((B, Rq, S), F32)
        lo = np.zeros((B, Rq, S), F32)
        for i in order:
            d = halves[i]
            hi = _mfma(hi, q0[..., d], k0[..., d], step)
            if down or one_acc:                              # one accumulator, the four products in turn
                if not drop_q1:
                    hi = _mfma(hi, q1[..., d], k0lo[..., d], step)
                hi = _mfma(hi, q2[..., d], k0lo[..., d], step)
                hi = _mfma(hi, q0[..., d], k1[..., d], step)
                continue
            if not drop_q1:
                lo = _mfma(lo, q1[..., d], k0lo[..., d], step)
            lo = _mfma(lo, q2[..., d], k0lo[..., d], step)
            lo = _mfma(lo, q0[..., d], k1[..., d], step)
        return (hi.astype(F64) + lo.astype(F64)).astype(F32)

    s = scores(range(len(halves)))
    if kind == "fused":
        odd = ((np.arange(Rq) >> 4) & 1).astype(bool)
        s = np.where(odd[None, :, None], scores((1, 0)), s)
    mx = s.max(-1, keepdims=True)
    e = np.exp((((s - mx).astype(F32)) * F32(1.0 / math.sqrt(dh))).astype(F32)).astype(F32)
    ps = _planes(e, pp, pp == 2)
    if p_single:
        ps = [_f16(e.astype(F64))]
    den = _lane_sum(ps[0].astype(F32) if norm_rounded else e)
    acc = np.zeros((B, Rq, dh), F32)
    for c in range(0, S, 32):
        kk = slice(c, c + 32)
        v0t, v0lt, v1t = (np.swapaxes(t[:, kk], -1, -2) for t in (v0, v0lo, v1))      # [B, dh, 32 keys]
        acc = _mfma(acc, ps[0][..., kk], v0t, step)
        for p in ps[1:]:
            acc = _mfma(acc, p[..., kk], v0lt, step)
        acc = _mfma(acc, ps[0][..., kk], v1t, step)
    rinv = (F32(1.0) / den).astype(F32)
    return as_triple((acc * rinv[..., None]).astype(F32))


# ---------------------------------------------------------------------------------------------------------------- [N, rows, heads dh] <-> [N heads, rows, dh]
def to_heads(x: np.ndarray, heads: int) -> np.ndarray:
    N, T, E = x.shape
    return np.ascontiguousarray(x.reshape(N, T, heads, E // heads).transpose(0, 2, 1, 3)).reshape(N * heads, T, E // heads)


def from_heads(x: np.ndarray, heads: int) -> np.ndarray:
    B, T, dh = x.shape
    return np.ascontiguousarray(x.reshape(B // heads, heads, T, dh).transpose(0, 2, 1, 3)).reshape(B // heads, T, heads * dh)


def models(qh, kh, vh, kind: str):
    """the intended arithmetic in its two summation orders of the scores"""
    return [model32(qh, kh, vh, kind), model32(qh, kh, vh, kind, one_acc=True)]


def three_ways(q, k, v, kind: str):
    """q [N, Rq, E], k, v [N, 128, E] (E = heads dh) -> (ref64, ref32, [model32 per summation order]) as [N, Rq, E]"""
    heads = KINDS[kind][0]
    qh, kh, vh = (to_heads(np.asarray(t, F32), heads) for t in (q, k, v))
    return from_heads(ref64(qh, kh, vh), heads), from_heads(ref32(qh, kh, vh), heads), [from_heads(m, heads) for m in models(qh, kh, vh, kind)]


def variant(q, k, v, kind: str, **flags):
    """model32 with flags, on [N, Rq, E] tensors: the CPU test's stand-ins for a kernel"""
    heads = KINDS[kind][0]
    return from_heads(model32(*(to_heads(np.asarray(t, F32), heads) for t in (q, k, v)), kind, **flags), heads)


# ---------------------------------------------------------------------------------------------------------------- inputs
def family_inputs(rng, slots, Rq: int, dh: int):
    """One (q [Rq, dh], k, v [128, dh]) head per entry of `slots` (indices into FAMILIES): N(0, 1) times the family's scales, a random sign per channel, and one
    V channel times 64 -> (q [n, Rq, dh], k, v [n, 128, dh], outlier channel per slot)."""
    n = len(slots)
    q, k, v = rng.standard_normal((n, Rq, dh)), rng.standard_normal((n, S, dh)), rng.standard_normal((n, S, dh))
    out = rng.integers(0, dh, n)
    for i, f in enumerate(slots):
        _, qs, ks, vs = FAMILIES[f]
        q[i] *= qs * rng.choice([-1.0, 1.0], dh)
        k[i] *= ks * rng.choice([-1.0, 1.0], dh)
        v[i] *= vs * rng.choice([-1.0, 1.0], dh)
        v[i, :, out[i]] *= min(OUTLIER, 2.0 ** 13 / vs)          # (2^10: times 8 - N(0, 1) 2^13 stays under the mode's range, 65504)
    assert max(np.abs(t).max() for t in (q, k, v)) < RO.F16_MAX
    return q.astype(F32), k.astype(F32), v.astype(F32), out


def slot_groups(slots, out, heads: int, shape):
    """name -> boolean mask over an output [N, Rq, heads dh] whose head n heads + h is slot n heads + h: a family's ordinary channels, and `name/x64` its
    outlier channels"""
    N, Rq, E = shape
    dh = E // heads
    groups = {}
    for i, f in enumerate(slots):
        n, h = divmod(i, heads)
        for name, cols in ((FAMILIES[f][0], [c for c in range(dh) if c != out[i]]), (FAMILIES[f][0] + "/x64", [int(out[i])])):
            m = groups.setdefault(name, np.zeros(shape, bool))
            m[n, :, [h * dh + c for c in cols]] = True
    return groups


def head_case(kind: str, Rq: int, slots, seed: int):
    """inputs of one call: head n heads + h of crop n is `slots[n heads + h]` -> (q [N, Rq, E], k, v [N, 128, E], groups)"""
    heads, dh = KINDS[kind][:2]
    assert len(slots) % heads == 0
    q, k, v, out = family_inputs(np.random.default_rng(seed), slots, Rq, dh)
    q, k, v = (from_heads(t, heads) for t in (q, k, v))
    return q, k, v, slot_groups(slots, out, heads, q.shape)


def cross_slots(crops_per_family: int = 2):
    """the decoder's geometry: a crop's 12 heads are one family, `crops_per_family` crops each"""
    return [f for f in range(len(FAMILIES)) for _ in range(crops_per_family * 12)]


def self_slots(call: int):
    """the encoder's geometry, N = 2 crops per call: the 12 (crop, head) slots walk the family list, each call going on where the last one stopped"""
    return [(call * 12 + i) % len(FAMILIES) for i in range(12)]


SELF_CALLS = 3                        # 36 slots: four heads per family


def judge(eng, refs, groups):
    """the project's bar (craft_layer_ref.bar: FACTOR x the larger of ref32's and model32's error, in the maximum and at the 99.99th percentile) in every
    group on its own; nothing is added for triple or fp32 outputs -> (ok, name -> figures)"""
    r64, r32, m32 = refs
    return RO.grouped_bar(np.asarray(eng), r64, r32, list(m32), groups, False)


def table(kernel: str, figs) -> str:
    return "\n".join(f"ATTN|{kernel}|{name}|{f['ratio_max']:.3f}|{f['ratio_p']:.3f}" + ("" if f["ok"] else "|FAIL") for name, f in figs.items())


# ---------------------------------------------------------------------------------------------------------------- the fused tile: from x, W and b
# A call of the fused tile: x rows of crop n scaled by 2^xs[n], head h's Q / K / V row blocks of W and b by 2^-e (e in 0 .. 8: the nine binades
# tests/test_gpu_split_gemm_range.py covers; x rows within its 2^-12 .. 2^13).  With x ~ N(0, 1) and W ~ 1.5 N(0, 1) / sqrt(384) a head's q, k, v are
# ~ 1.5 2^(xs - e).
# No group goes beyond the peaky family's scores (q k <= 36): at q, k ~ 24 (scores of several hundred) the softmax is one-hot except in a handful of near-tie rows, a
# group's maximum is a single draw from a heavy tail, and the ratio of two such maxima (0.15 to 1.9 between two crops of one measurement) says nothing.
HEADS_A = ((0, 0, 0), (0, 8, 4), (0, 0, 8), (0, 8, 8), (4, 4, 0), (0, 4, 6))
HEADS_B = ((0, 8, 4), (0, 8, 8), (4, 4, 0), (2, 2, 0), (0, 4, 6), (0, 6, 8))
HEADS_V = ((8, 8, 0), (8, 8, 0), (8, 7, 0), (7, 8, 0), (8, 8, 4), (8, 8, 8))
FUSED_CALLS = (("a", (0, -6), HEADS_A),       # xs 0: unit, small V, small K without a large Q;  xs -6: v ~ 1.5 2^-14, plane 0 in the f16 subnormals
               ("b", (4, 2), HEADS_B),        # xs 4: q ~ 24 on k ~ 0.09 (small K under large Q), v ~ 0.09, both; q, k ~ 6 and q ~ 24 on k ~ 1.5: peaky (scores ~ 30)
               ("c", (10, 9), HEADS_V))       # large V: v ~ 1.5 2^10 under q, k ~ 6 and 3
FUSED_N7 = ("n7", (4, 2, 0, -6, 4, 2, 0), HEADS_B)


def fused_seed(name: str) -> int:
    return 60 + sum(map(ord, name))


def fused_inputs(rng, xs, head_exps):
    N = len(xs)
    x = np.clip(rng.standard_normal((N, S, 384)), -7.0, 7.0) * (2.0 ** np.asarray(xs, F64))[:, None, None]
    w = rng.standard_normal((3, 6, 64, 384)) / math.sqrt(384.0) * 1.5
    b = 0.3 * rng.standard_normal((3, 6, 64))
    for h, es in enumerate(head_exps):
        for t, e in enumerate(es):
            w[t, h] *= 2.0 ** -e
            b[t, h] *= 2.0 ** -e
    return x.astype(F32), w.reshape(1152, 384).astype(F32), b.reshape(1152).astype(F32)


def fused_groups(xs, head_exps, shape):
    groups = {}
    for n, s in enumerate(xs):
        for h, (qe, ke, ve) in enumerate(head_exps):
            m = groups.setdefault(f"x2^{s} q2^{s - qe} k2^{s - ke} v2^{s - ve}", np.zeros(shape, bool))
            m[n, :, h * 64:(h + 1) * 64] = True
    return groups


def fused_three_ways(x, w, b, flags=None):
    """the fused qkv + attention tile from x [N, 128, 384], W [1152][384] (rows 384 c + 64 h + d), b: the projection in float64 / fp32 / as the split linear
    forms it (rowops_ref.gemm_refs: x as pairs, the MFMA's order), then the attention on each one's own q, k, v -> (ref64, ref32, [model32 per order]);
    with flags, the one flagged model32 as a fourth"""
    N = x.shape[0]
    p64, p32, (pm,) = RO.gemm_refs(x.reshape(N * S, 384), w, 2, bias=b, orders=("mfma",))
    cut = lambda p: [to_heads(np.ascontiguousarray(p.reshape(N, S, 3, 384)[:, :, t]), 6) for t in range(3)]
    qkv = [t.astype(F32) for t in cut(pm)]
    out = (from_heads(ref64(*cut(p64)), 6), from_heads(ref32(*cut(p32)), 6), [from_heads(m, 6) for m in models(*qkv, "fused")])
    return out if flags is None else out + (from_heads(model32(*qkv, "fused", **flags), 6),)


# ---------------------------------------------------------------------------------------------------------------- the decoder's self-attention (vector ALU: controls)
def dec_self_case(N: int, seed: int):
    """the decoder's self-attention: the position queries q [26, 384] are shared by the crops, so the 12 heads are the families (the list, then its first
    three again) -> (q [26, 384], kvcache [N, 26, 768] (K | V), slots and outlier channels per (crop, head) for slot_groups)"""
    rng = np.random.default_rng(seed)
    slots = [h % len(FAMILIES) for h in range(12)]
    q, k, v = rng.standard_normal((12, 26, 32)), rng.standard_normal((N, 12, 26, 32)), rng.standard_normal((N, 12, 26, 32))
    out = rng.integers(0, 32, 12)
    for h, f in enumerate(slots):
        _, qs, ks, vs = FAMILIES[f]
        q[h] *= qs * rng.choice([-1.0, 1.0], 32)
        k[:, h] *= ks * rng.choice([-1.0, 1.0], 32)
        v[:, h] *= vs * rng.choice([-1.0, 1.0], 32)
        v[:, h, :, out[h]] *= min(OUTLIER, 2.0 ** 13 / vs)
    flat = lambda t: np.ascontiguousarray(np.moveaxis(t, -3, -2)).reshape(t.shape[:-3] + (26, 384)).astype(F32)
    return flat(q), np.concatenate([flat(k), flat(v)], -1), slots * N, list(out) * N


def masked_three_ways(q, k, v, vis):
    """q [B, Rq, dh], k, v [B, J, dh], vis bool [B, Rq, J] -> (ref64, ref32, a second fp32 evaluation that adds its products one by one and
    leaves as an exact triple) - the kernel is plain fp32"""
    sc = 1.0 / math.sqrt(q.shape[-1])
    q6, k6, v6 = (np.asarray(t, F64) for t in (q, k, v))
    s = np.where(vis, q6 @ np.swapaxes(k6, -1, -2) * sc, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    r64 = (p / p.sum(-1, keepdims=True)) @ v6
    tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(t, F32)) for t in (q, k, v))
    ts = (tq @ tk.transpose(-1, -2)) * F32(sc)
    ts = torch.where(torch.from_numpy(vis), ts, torch.tensor(-math.inf))
    r32 = (torch.softmax(ts, -1) @ tv).numpy()
    s1 = np.zeros(s.shape, F32)
    for d in range(q.shape[-1]):
        s1 = (s1 + q[..., :, None, d] * k[..., None, :, d]).astype(F32)
    s1 = np.where(vis, (s1 * F32(sc)).astype(F32), F32(-np.inf))
    e = np.exp((s1 - s1.max(-1, keepdims=True)).astype(F32)).astype(F32)
    den = np.zeros(e.shape[:-1], F32)
    o = np.zeros(r64.shape, F32)
    for j in range(k.shape[-2]):
        den = (den + e[..., j]).astype(F32)
        o = (o + e[..., j, None] * v[..., None, j, :]).astype(F32)
    return r64, r32, as_triple((o / den[..., None]).astype(F32))
