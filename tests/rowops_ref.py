"""The f16x4 row kernels (the split, LayerNorm, the LayerNorm prologue) and the split linears away from unit scale: inputs, float64 references and derived
bars.  TEST INFRASTRUCTURE ONLY (tests/test_gpu_rowops.py, tests/test_gpu_split_gemm_range.py, tests/test_rowops_cpu.py); numpy / torch, no engine.

The split itself is NOT restated here: planes_bits() is craft_layer_ref.split_act (the restatement of tuatara_amd/csrc/split.h that the detector's per-layer
test already rests on) turned into f16 bit planes.  What is stated here independently of the kernels: the contract of split.h (split_contract), LayerNorm in
float64 with a worst-case fp32 error bound (ln64, ln_tol), the tiled planes layout (untile), and the inputs.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import craft_layer_ref as R

D = 384
F16_MAX = 65504.0
U = 2.0 ** -24                 # fp32 unit roundoff
SUB = 2.0 ** -36               # half the spacing (2^-35 in units of x) of the lower planes' f16 subnormals
A_TOL = B_TOL = 16.0


# ---------------------------------------------------------------------------------------------------------------- the split
def _pred(x):
    return np.nextafter(np.float32(x), np.float32(0))


def _succ(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def edge_values(n_random: int = 4096, seed: int = 20) -> np.ndarray:
    """The fp32 values on which the split is compared bit for bit: zeros, fp32 denormals, the f16 subnormal range and its rounding points, both sides of every
    power of two of the f16 range, the largest significand, the two round-to-nearest ties of a pair's first plane, the last float below 65504, all with
    their negative twins, and random bit patterns with the exponent uniform in [-30, 15].  Values of 65504 and more (the largest significand at 2^15, some
    random patterns of exponent 15) are outside the mode's one range condition: the planes are still compared (the kernel and the restatement saturate alike),
    the contract is not asked of them (split_contract)."""
    v = [0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24]
    for k in range(-14, 16):
        p = np.float32(2.0 ** k)
        v += [_pred(p), p, _succ(p), (2.0 - 2.0 ** -23) * 2.0 ** k, (1.0 + 2.0 ** -11) * 2.0 ** k, (1.0 + 3 * 2.0 ** -11) * 2.0 ** k]
    v.append(_pred(F16_MAX))
    pos = np.asarray(v, np.float64).astype(np.float32)
    assert np.array_equal(pos.astype(np.float64), np.asarray(v, np.float64))           # every listed value is an fp32 number
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, 2, n_random).astype(np.uint32) << 31) | ((rng.integers(-30, 16, n_random) + 127).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n_random).astype(np.uint32)
    return np.concatenate([pos, -pos, bits.view(np.float32)]).astype(np.float32)


def planes_bits(x: np.ndarray, planes: int) -> np.ndarray:
    """craft_layer_ref.split_act as f16 bit planes: fp32 [..., C] -> u16 [..., planes, C] (x0 | x1 (| x2), the lower planes scaled by 2^11 as they are stored)"""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    parts = R.split_act(t, planes)
    h = torch.stack([p.to(torch.float16) for p in parts], -2).contiguous()
    assert all(torch.equal(p, q.to(torch.float32)) for p, q in zip(parts, h.unbind(-2)))    # (the restatement's planes are f16 numbers)
    return h.numpy().view(np.uint16)


def same_bits(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """elementwise equality of f16 bit patterns, zeros of either sign counting as equal"""
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    return (a == b) | (((a | b) & 0x7FFF) == 0)


def join_bits(bits: np.ndarray) -> np.ndarray:
    """join2 / join3 in float64 from u16 bit planes [..., planes, C]"""
    h = np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)
    return h[..., 0, :] + h[..., 1:, :].sum(-2) / 2048.0


def split_contract(x: np.ndarray, bits: np.ndarray):
    """split.h's contract on the planes of x, for every |x| < 65504 -> (ok, worst excess).  A triple joins to x exactly wherever its third plane is a normal f16
    number, and wherever that plane is zero and |x| >= 2^-12 (there x is a multiple of 2^-35, the spacing of the third plane's subnormals, so nothing was rounded
    away); otherwise within 2^-36, half that spacing.  (Below 2^-12 a zero third plane may stand for a remainder that rounded to zero: 2^-149 has three zero
    planes.)  A pair joins to x within one fp32 ulp of x or 2^-36, whichever is larger."""
    x64 = np.asarray(x, np.float64)
    planes = bits.shape[-2]
    err = np.abs(join_bits(bits) - x64)
    inside = np.abs(x64) < F16_MAX
    if planes == 3:
        b2 = np.asarray(bits[..., 2, :], np.uint16)
        normal = (b2 & 0x7C00) != 0
        zero = (b2 & 0x7FFF) == 0
        allow = np.where(normal | (zero & (np.abs(x64) >= 2.0 ** -12)), 0.0, SUB)
    else:
        allow = np.maximum(R.ulp32(np.where(inside, x64, 0.0)), SUB)
    excess = np.where(inside, err - allow, 0.0)
    return bool((excess <= 0).all()), float(excess.max())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def ln64(x, gamma, beta, eps: float) -> np.ndarray:
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def ln_tol(x, gamma, beta, eps: float, pair: bool = False) -> np.ndarray:
    """Worst-case bound on |fp32 two-pass LayerNorm - ln64| per element, u = 2^-24, X = max |x| of the row, mu and r = 1 / sqrt(var + eps) in float64:

        tol = u (A |g| r X + B (|g| |x - mu| r + |beta|)) + (A u X r)^2 |y - beta|,      A = B = 16.

    A: the mean - a tree of 7 in-lane and 6 butterfly additions, each rounding a partial sum of at most 384 X to half an ulp, then the multiply by fl(1/384):
    an error of a few ulp(X), carried to every output by the factor |g| r.  B: the subtraction, the 16 roundings of the centred sum of squares (each relative
    u, halved by the square root), the reciprocal square root instruction (1 ulp), the multiply and the fused multiply-add - relative errors of the output's own
    terms.  Last term: the mean's error e shifts every centred value, which moves the variance by e^2 (the first-order term sums to zero): relative (e r)^2 on
    the scaled part y - beta.  A sequential fp32 sum of 384 values errs by up to 383 u X and does not fit A; a one-pass variance errs by u X^2 r^2 and fits
    nothing.  Where the output is a pair, one fp32 ulp of |y| (or 2^-36) more."""
    x = np.asarray(x, np.float64)
    g, b = np.abs(np.asarray(gamma, np.float64)), np.abs(np.asarray(beta, np.float64))
    X = np.abs(x).max(-1, keepdims=True)
    mu = x.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + eps)
    y = ln64(x, gamma, beta, eps)
    tol = U * (A_TOL * g * r * X + B_TOL * (g * np.abs(x - mu) * r + b)) + (A_TOL * U * X * r) ** 2 * np.abs(y - np.asarray(beta, np.float64))
    if pair:
        tol = tol + R.ulp32(y) + SUB
    return tol


CONSTANTS = (0.0, 4.0, -0.5, 2.0 ** -20, 2.0 ** 15)


def ln_families(rng, rows: int):
    """-> (families: name -> fp32 [rows][384] in a fixed order, gamma, beta).  gamma = 1 + 0.5 N(0,1), beta = 0.3 N(0,1) with |beta| kept at 2^-10 or more, so that
    every beta is its own exact triple (split_contract) and a constant row's planes can be held to beta's bit for bit.  The last family, "const", has one row
    per value of CONSTANTS whatever `rows` says."""
    z = lambda: rng.standard_normal((rows, D))
    gamma = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(D)).astype(np.float32)
    beta = np.where(np.abs(beta) < 2.0 ** -10, np.copysign(np.float32(2.0 ** -10), beta), beta).astype(np.float32)
    fam = {}
    fam["unit"] = z()
    fam["offset_1000"] = z() + 1000.0
    fam["offset_-30000"] = 4.0 * z() - 30000.0
    fam["small_1e-4"] = 1e-4 * z()
    fam["tiny_1e-6"] = 1e-6 * z()
    fam["large_6000"] = 6000.0 * z()
    o = z(); o[:, 7] = 5000.0; o[:, 200] = -800.0
    fam["outlier"] = o
    h = np.zeros((rows, D)); h[np.arange(rows), rng.integers(0, D, rows)] = 100.0
    fam["onehot_100"] = h
    fam["const"] = np.repeat(np.asarray(CONSTANTS, np.float64)[:, None], D, 1)
    fam = {k: v.astype(np.float32) for k, v in fam.items()}
    assert all(np.abs(v).max() < F16_MAX for v in fam.values())
    return fam, gamma, beta


def untile(raw: np.ndarray, M: int, planes: int) -> np.ndarray:
    """the tiled planes layout [M / 8][plane][6 blocks of 64 channels][8 rows][64] -> rows [M][planes][384]"""
    assert M % 8 == 0 and raw.size == M * planes * D
    return np.ascontiguousarray(raw.reshape(M // 8, planes, 6, 8, 64).transpose(0, 3, 1, 2, 4)).reshape(M, planes, D)


# fp32 LayerNorms on the CPU: the forms ln_tol must accept, and the wrong ones it must reject (tests/test_rowops_cpu.py)
def ln32_two_pass(x, gamma, beta, eps, ddof: int = 0, use_eps: bool = True, swap: bool = False):
    x = np.asarray(x, np.float32)
    n = np.float32(x.shape[-1])
    mu = (x.sum(-1, keepdims=True, dtype=np.float32) / n).astype(np.float32)
    d = (x - mu).astype(np.float32)
    var = ((d * d).sum(-1, keepdims=True, dtype=np.float32) / np.float32(x.shape[-1] - ddof)).astype(np.float32)
    r = (np.float32(1) / np.sqrt(var + np.float32(eps if use_eps else 0.0), dtype=np.float32)).astype(np.float32)
    g, b = (beta, gamma) if swap else (gamma, beta)
    return ((d * r).astype(np.float32) * np.asarray(g, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def ln32_tree(x, gamma, beta, eps):
    """The fp32 two-pass LayerNorm in the summation order the row kernels document (split.h: ln384_row8): 48 lanes x 8 consecutive values, each lane's 8 values
    added in sequence, the 64 lanes (16 of them idle) joined by a butterfly over lane distances 32 .. 1; mean = fl(s fl(1/384)); the centred squares likewise,
    by multiply-add; r = 1 / sqrt(fl(q fl(1/384) + eps)); y = fma(fl((v - mean) r), gamma, beta).  A model of the kernel's noise for the bars (multiply-adds
    through float64, the reciprocal square root correctly rounded), not a bit-exact restatement."""
    f32, f64 = np.float32, np.float64
    x = np.asarray(x, f32)
    rows = x.shape[0]
    lane = np.arange(64)

    def tree(part):                                         # part [rows][48]: the lanes' partial sums
        a = np.zeros((rows, 64), f32); a[:, :48] = part
        for o in (32, 16, 8, 4, 2, 1):
            a = (a + a[:, lane ^ o]).astype(f32)
        return a[:, :1]

    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    v = x.reshape(rows, 48, 8)
    s = np.zeros((rows, 48), f32)
    for e in range(8):
        s = (s + v[:, :, e]).astype(f32)
    mean = (tree(s) * f32(1.0 / 384.0)).astype(f32)
    d = (x - mean).astype(f32)
    dv = d.reshape(rows, 48, 8)
    q = np.zeros((rows, 48), f32)
    for e in range(8):
        q = fma(dv[:, :, e], dv[:, :, e], q)
    var = fma(tree(q), np.full((rows, 1), 1.0 / 384.0, f32), np.full((rows, 1), eps, f32))
    r = (1.0 / np.sqrt(var.astype(f64))).astype(f32)
    return fma((d * r).astype(f32), np.broadcast_to(np.asarray(gamma, f32), x.shape), np.broadcast_to(np.asarray(beta, f32), x.shape))


def ln32_one_pass(x, gamma, beta, eps):
    """E[x^2] - E[x]^2 in fp32: the variance a kernel must not form"""
    x = np.asarray(x, np.float32)
    n = np.float32(x.shape[-1])
    mu = (x.sum(-1, keepdims=True, dtype=np.float32) / n).astype(np.float32)
    ex2 = ((x * x).sum(-1, keepdims=True, dtype=np.float32) / n).astype(np.float32)
    var = np.maximum((ex2 - mu * mu).astype(np.float32), np.float32(0))
    r = (np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)).astype(np.float32)
    return (((x - mu) * r).astype(np.float32) * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)).astype(np.float32)


def ln32_torch(x, gamma, beta, eps):
    return F.layer_norm(torch.from_numpy(np.ascontiguousarray(x, np.float32)), (D,), torch.from_numpy(np.asarray(gamma, np.float32)),
                        torch.from_numpy(np.asarray(beta, np.float32)), eps).numpy()


# ---------------------------------------------------------------------------------------------------------------- split linears off unit scale
SCALES = (-12, -6, 0, 6, 13)              # row i is scaled by 2^SCALES[i % 5]
OUTLIER_CHANNELS = (7, 200, 383)
ACT_NONE, ACT_GELU = 0, 2


def gemm_inputs(rng, M: int = 296, K: int = 384, N: int = 392):
    """-> (x [M][K], w [N][K], groups: name -> row indices, row scale [M]).  x = clip(N(0,1), +-7) with row i scaled by 2^SCALES[i % 5]: 2^-12 puts plane 0 into
    the f16 subnormals, 2^13 sits under the range guard; three input channels times 64 (a ViT stream's outlier channels), everything clipped to +-60000.
    w = N(0,1) / sqrt(K), output row n scaled by 2^-(n % 9)."""
    x = np.clip(rng.standard_normal((M, K)), -7.0, 7.0)
    s = np.asarray(SCALES)[np.arange(M) % len(SCALES)]
    x = x * (2.0 ** s)[:, None]
    x[:, list(OUTLIER_CHANNELS)] *= 64.0
    x = np.clip(x, -60000.0, 60000.0).astype(np.float32)
    w = (rng.standard_normal((N, K)) / math.sqrt(K) * (2.0 ** -(np.arange(N) % 9))[:, None]).astype(np.float32)
    groups = {f"2^{e}": np.flatnonzero(s == e) for e in SCALES}
    return x, w, groups, (2.0 ** s).astype(np.float32)


def gelu64(y: np.ndarray) -> np.ndarray:
    """erf GELU in float64, y Phi(y) with Phi = erfc(-y / sqrt 2) / 2: 1 + erf(.) would cancel to multiples of 2^-53 in the negative tail"""
    y = np.ascontiguousarray(y, np.float64)
    return 0.5 * y * torch.erfc(torch.from_numpy(-y / math.sqrt(2.0))).numpy()


def gemm_refs(x, w, planes: int, bias=None, resid=None, act: int = ACT_NONE, mutate=None, orders=("mfma", "conv")):
    """One linear three ways through craft_layer_ref.Layer with ks = 1: (ref64, ref32, [model32 per summation order]) as [M][N] arrays.  `planes` = how the
    activation enters the product (2: pairs, 3: triples).  The residual is added and GELU applied in the dtype of each (float64 erf GELU on ref64, fp32 GELU
    on ref32 and model32)."""
    M, K = x.shape
    N = w.shape[0]
    L = R.Layer(np.asarray(w, np.float32).reshape(N, 1, 1, K), np.zeros(N, np.float32) if bias is None else bias, relu=False, planes=planes)
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32).T.copy()).view(1, K, 1, M)
    flat = lambda t: t.reshape(N, M).T.contiguous()
    r64 = flat(L.plain(xt, 0, 1, 0, 1, torch.float64))
    r32 = flat(L.plain(xt, 0, 1, 0, 1, torch.float32))
    ms = [flat(L.model(xt, 0, 1, 0, 1, mutate, o)) for o in orders]
    return gemm_epilogue(r64.numpy(), r32.numpy(), [m.numpy() for m in ms], resid, act)


def gemm_epilogue(r64, r32, ms, resid=None, act: int = ACT_NONE):
    """the residual and GELU on top of gemm_refs' plain linear (computed once, shared by the epilogue cases): each in its own dtype"""
    r64, r32, ms = torch.from_numpy(r64), torch.from_numpy(r32), [torch.from_numpy(m) for m in ms]
    if resid is not None:
        rt = torch.from_numpy(np.ascontiguousarray(resid, np.float32))
        r64 = r64 + rt.to(torch.float64)
        r32 = r32 + rt
        ms = [m + rt for m in ms]
    if act == ACT_GELU:
        r64 = torch.from_numpy(gelu64(r64.numpy()))
        r32 = F.gelu(r32)
        ms = [F.gelu(m) for m in ms]
    return r64.numpy(), r32.numpy(), [m.numpy() for m in ms]


def grouped_bar(eng, ref64, ref32, models, groups, pair_out: bool):
    """craft_layer_ref.bar on each group of rows that share a scale (a global maximum would only see the largest rows) -> (all ok, name -> figures)"""
    out, ok = {}, True
    for name, rows in groups.items():
        k, f = R.bar(eng[rows], ref64[rows], ref32[rows], [m[rows] for m in models], pair_out)
        f["ok"] = k
        out[name] = f
        ok = ok and k
    return ok, out
