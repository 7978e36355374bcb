"""One CRAFT layer of the f16x4 engine on its own, three ways on the CPU.  TEST INFRASTRUCTURE ONLY (tests/test_gpu_craft_layers.py,
tests/test_craft_layer_bar_cpu.py).

For a layer given by its input tensor(s), the fp32 weights [Cout][ks][ks][Cin] and bias of the weight file:

* ref64   - the layer in float64 (conv with its padding / dilation, bias, virtual concat, bilinear x2 of oracle/models.py, ReLU, 2x2 max-pool);
* ref32   - the same in fp32 torch: the reference's own arithmetic;
* model32 - the split product as the kernels form it (tuatara_amd/csrc/split.h), restated in fp32 torch: the weight pair w S = w0 + w1 and w0b = w0 / 2^11
            with S and the roundings of Engine::upload_linear, the activation pair of split2_pair (or the exact triple of split3_pair), the three or four
            partial products summed in fp32 into one accumulator, 8 products at a time as the f16 MFMA adds them (Layer.split_acc), times 1 / S, plus the
            bias.

bar(): assertion 1 of the per-layer test, |engine - ref64| <= 1.5 x max(|ref32 - ref64|, |model32 - ref64|) in the maximum and at the 99.99th percentile
(+ one fp32 ulp of |ref64| elementwise where the engine wrote a pair).

Tensors are NCHW torch tensors.  Every convolution can be evaluated on a band of output rows (a conv is local), so that a full page costs a quarter.
`mutate` hooks let the CPU test break the model on purpose (a dropped product, a shifted tap ...); nothing is ever broken on the GPU.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

FACTOR = 1.5          # the factor of the project's two float64 budgets (tests/test_gpu_x4_parity.py: test_x4_error_budget_against_fp64_*)
PCT = 99.99
STEP = 8              # products per fp32 rounding of the accumulator (Layer.split_acc)


def set_threads():
    """torch's CPU threads from the environment (a GPU box hands a job 16 CPUs of many more)"""
    n = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or 16
    torch.set_num_threads(max(1, n))


# ---------------------------------------------------------------------------------------------------------------- split.h on the CPU
def weight_planes(w: torch.Tensor):
    """Engine::upload_linear: S = 2^e with max |w| S in [2^13, 2^14); w0 = f16(w S), w1 = f16(w S - w0), w0b = f16(w0 / 2^11) -> (w0, w0b, w1, 1 / S), fp32"""
    mx = float(w.abs().max())
    e = 0
    if mx > 0:
        e = 14 - math.frexp(mx)[1]
    e = max(-24, min(40, e))
    v = w.to(torch.float32) * (2.0 ** e)                      # exact
    w0 = v.to(torch.float16).to(torch.float32)
    w1 = (v - w0).to(torch.float16).to(torch.float32)
    w0b = (w0 * (1.0 / 2048.0)).to(torch.float16).to(torch.float32)
    return w0, w0b, w1, 2.0 ** -e


def _rtz_f16(x: torch.Tensor) -> torch.Tensor:
    """round toward zero to f16, as fp32 (v_cvt_pkrtz_f16_f32); |x| < 65504"""
    bits = x.contiguous().view(torch.int32)
    norm = (bits & ~0x1FFF).view(torch.float32)               # 10 significand bits kept
    sub = torch.trunc(x * 2.0 ** 24) * 2.0 ** -24              # f16 subnormals: multiples of 2^-24
    return torch.where(x.abs() >= 2.0 ** -14, norm, sub)


def split_act(x: torch.Tensor, planes: int):
    """split2_pair (planes = 2) / split3_pair (3): fp32 -> [x0, x1 (, x2)], the lower planes scaled by 2^11 as they are stored"""
    x = x.to(torch.float32)
    if planes == 2:
        x = x.clamp(-65504.0, 65504.0)
        x0 = x.to(torch.float16).to(torch.float32)
        x1 = ((x - x0) * 2048.0).to(torch.float16).to(torch.float32)
        return [x0, x1]
    x0 = _rtz_f16(x)
    r = (x - x0) * 2048.0
    x1 = _rtz_f16(r)
    x2 = (r - x1).to(torch.float16).to(torch.float32)
    return [x0, x1, x2]


def join(parts):
    """join2 / join3"""
    lo = parts[1] if len(parts) == 2 else parts[1] + parts[2]
    return parts[0] + lo * (1.0 / 2048.0)


def ulp32(x) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- convolution on row bands
def conv_rows(x: torch.Tensor, row0: int, H: int, w: torch.Tensor, dil: int, r0: int, r1: int) -> torch.Tensor:
    """Output rows [r0, r1) of the zero-padded 'same' convolution of an H-row image, of which x holds rows [row0, row0 + x.shape[2]) - at least
    [max(r0 - pad, 0), min(r1 + pad, H)).  w OIHW.  No bias."""
    ks = w.shape[-1]
    pad = dil * (ks // 2)
    top, bot = r0 - pad, r1 + pad
    a, b = max(top, 0), min(bot, H)
    assert row0 <= a and b <= row0 + x.shape[2], (row0, x.shape, r0, r1)
    xs = x[:, :, a - row0:b - row0]
    if a - top or bot - b:
        xs = F.pad(xs, (0, 0, a - top, bot - b))
    return F.conv2d(xs, w, None, 1, (0, pad), dil)


def bands(H: int, patch: int = 16, banded: bool = True):
    """Row bands [r0, r1) of an H-row map: all of it, or (banded, H >= 128) the first and the last 16 rows and one interior band across the patch-row seam at
    H / 2 - together at least a quarter of the rows; every edge even (a 2x2 pool pairs rows)."""
    if not banded or H < 128:
        return [(0, H)]
    mid = H // 2 // patch * patch
    half = max(16, (H // 4 - 32 + 1) // 2)
    half = (half + 1) // 2 * 2
    out = [(0, 16), (mid - half, mid + half), (H - 16, H)]
    assert out[0][1] <= out[1][0] and out[1][1] <= out[2][0] and sum(b - a for a, b in out) * 4 >= H
    return out


# ---------------------------------------------------------------------------------------------------------------- a layer, three ways
class Layer:
    """conv (ks x ks, dilation dil) over cat(in0, in1) + bias, then act; outputs out / out_relu / out_pool (2x2 max of ReLU(out) or of out, which is the same
    thing behind a ReLU).  w [Cout][ks][ks][Cin] as in the weight file."""

    def __init__(self, w: np.ndarray, b: np.ndarray, dil: int = 1, relu: bool = True, planes: int = 2):
        self.w = torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float32))).permute(0, 3, 1, 2).contiguous()   # OIHW
        self.b = torch.from_numpy(np.ascontiguousarray(np.asarray(b, np.float32)))
        self.dil, self.relu, self.planes = dil, relu, planes

    # -- the plain layer in a dtype
    def plain(self, x: torch.Tensor, row0: int, H: int, r0: int, r1: int, dt) -> torch.Tensor:
        y = conv_rows(x.to(dt), row0, H, self.w.to(dt), self.dil, r0, r1) + self.b.to(dt).view(1, -1, 1, 1)
        return y.clamp_min(0) if self.relu else y

    # -- the split product
    def split_acc(self, x: torch.Tensor, row0: int, H: int, r0: int, r1: int, w=None, mutate=None, order: str = "mfma") -> torch.Tensor:
        """The partial products into ONE fp32 accumulator, times 1 / S (no bias), summed the way the kernels sum.  v_mfma_f32_16x16x32_f16 takes 8 consecutive k
        values from each of its four lane groups (the `fg * 8` of every fragment address in the kernels) and adds the four 8-term dot products to the
        accumulator one after the other, each add rounded to fp32 (inferred from the engine's measured noise, which steps of 8 reproduce in maximum, percentile and
        rms while steps of 32 and 4 miss it by 2 x either way - not a documented property of the instruction): an output takes taps x Cin / 8 x 3 (or 4) roundings in sequence - 1728 for a 3x3 over 512
        channels - and its noise grows with the root of that count.  torch's own convolution blocks its sums otherwise, and differently from CPU to CPU
        (the same slice5.1 tensor: max |conv32 - conv64| 2.6e-6 on one machine, 7.4e-6 on another), so a model summed by F.conv2d restates the products but
        not the noise of their summation (profiles/craft_layers_fp64.md has the measurement that told steps of 8 from steps of 32 and 4).  Here a step
        is one addmm_ over 8 channels of one tap and one partial product (x0 w0, x1 w0b, (x2 w0b,) x0 w1), pixel block by pixel block so that the
        accumulators stay in cache.  The order of the steps (tap, channel group, product) is one kernel's; the kernels differ among themselves in it and
        agree in the count.  Layers of fewer than 8 input channels (conv1_1: its 27 inputs are ONE MFMA per product) take one convolution over the stacked
        planes - which is also what order = "conv" does for every layer: the partial convolutions summed by torch's own convolution, the other
        restatement the bar knows (bar(): the larger of the two errors counts).  mutate(xs, ws) may edit the lists of activation planes and of weight planes [w0, w0b, w1] in place (broken models)."""
        w0, w0b, w1, inv = weight_planes(self.w if w is None else w)
        xs = split_act(x, self.planes)
        ws = [w0, w0b, w1]
        if mutate:
            mutate(xs, ws)
        Cout, C, ks = ws[0].shape[0], ws[0].shape[1], ws[0].shape[-1]
        if C < STEP or order == "conv":
            xa = torch.cat(xs + [xs[0]], 1)
            wa = torch.cat([ws[0]] + [ws[1]] * (len(xs) - 1) + [ws[2]], 1)
            return conv_rows(xa, row0, H, wa, self.dil, r0, r1) * inv
        dil, pad = self.dil, self.dil * (ks // 2)
        top, bot = r0 - pad, r1 + pad
        a, b = max(top, 0), min(bot, H)
        assert row0 <= a and b <= row0 + x.shape[2] and C % STEP == 0, (row0, x.shape, r0, r1)
        B, Wd, h, G = x.shape[0], x.shape[3], r1 - r0, C // STEP
        prods = [(0, 0)] + [(i, 1) for i in range(1, len(xs))] + [(0, 2)]
        # planes as [group][B][rows + 2 pad][W + 2 pad][8] and weights as [plane][tap][group][8][Cout]: every step's operands are contiguous rows
        xp = [F.pad(t[:, :, a - row0:b - row0], (pad, pad, a - top, bot - b)).view(B, G, STEP, h + 2 * pad, Wd + 2 * pad).permute(1, 0, 3, 4, 2).contiguous() for t in xs]
        wt = [t.view(Cout, G, STEP, ks, ks).permute(3, 4, 1, 2, 0).contiguous() for t in ws]
        out = torch.empty(B, h, Wd, Cout, dtype=torch.float32)
        rb = max(1, min(h, (1 << 18) // (Cout * Wd)))                      # rows per block: ~1 MB of accumulators
        for n in range(B):
            for y0 in range(0, h, rb):
                y1 = min(h, y0 + rb)
                acc = torch.zeros((y1 - y0) * Wd, Cout, dtype=torch.float32)
                for ky in range(ks):
                    for kx in range(ks):
                        cols = [t[:, n, y0 + ky * dil:y1 + ky * dil, kx * dil:kx * dil + Wd].reshape(G, (y1 - y0) * Wd, STEP) for t in xp]
                        for g in range(G):
                            for xi, wi in prods:
                                acc.addmm_(cols[xi][g], wt[wi][ky, kx, g])
                out[n, y0:y1] = acc.view(y1 - y0, Wd, Cout)
        return out.permute(0, 3, 1, 2) * inv

    def model(self, x: torch.Tensor, row0: int, H: int, r0: int, r1: int, mutate=None, order: str = "mfma") -> torch.Tensor:
        y = self.split_acc(x, row0, H, r0, r1, None, mutate, order) + self.b.view(1, -1, 1, 1)
        return y.clamp_min(0) if self.relu else y


def pool2(y: torch.Tensor, relu: bool) -> torch.Tensor:
    y = F.max_pool2d(y, 2)
    return y.clamp_min(0) if relu else y


def upsample2x(z: torch.Tensor) -> torch.Tensor:
    """the bilinear x2 of oracle/models.py (F.interpolate, align_corners=False)"""
    return F.interpolate(z, scale_factor=2, mode="bilinear", align_corners=False)


def upsample2x_expr32(v: np.ndarray) -> np.ndarray:
    """The engine's own expression (split_ops.hip: bilerp_s; craft_ops.hip: bilerp), rounding by rounding, on fp32 NHWC: top = fma(lx1, v01, lx0 v00),
    bot likewise, out = fma(ly1, bot, ly0 top).  The weights are 0, 1/4, 3/4, 1: every product is exact in float64 and a float64 sum of two such terms
    rounded to fp32 is the fma's result."""
    v = np.asarray(v, np.float32)
    B, H, W, C = v.shape

    def taps(n, N):
        s = np.maximum(0.5 * (np.arange(n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
        i0 = s.astype(np.int64)
        i1 = i0 + (i0 < N - 1)
        l1 = (s - i0.astype(np.float32)).astype(np.float32)
        return i0, i1, (np.float32(1) - l1).astype(np.float64), l1.astype(np.float64)

    y0, y1, ly0, ly1 = taps(2 * H, H)
    x0, x1, lx0, lx1 = taps(2 * W, W)
    v64 = v.astype(np.float64)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]

    def row(r):
        a = (lx0 * r[:, :, x0]).astype(np.float32).astype(np.float64)
        return (lx1 * r[:, :, x1] + a).astype(np.float32).astype(np.float64)

    top, bot = row(v64[:, y0]), row(v64[:, y1])
    a = (ly0[None, :, None, None] * top).astype(np.float32).astype(np.float64)
    return (ly1[None, :, None, None] * bot + a).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the bar
def bar(eng, ref64, ref32, model32, pair_out: bool):
    """Assertion 1.  Returns (ok, figures): figures = max / p99.99 of |engine - ref64| (less one fp32 ulp of |ref64| where the output is a pair), of
    |ref32 - ref64| and |model32 - ref64|, and the ratio of the engine's figure to the larger of the two, each way.  model32 may be a list of restatements
    of the same split product in different fp32 summation orders (Layer.split_acc: the MFMA's and torch's): the larger error counts, both are reported."""
    r64 = np.asarray(ref64, np.float64)
    e = np.abs(np.asarray(eng, np.float64) - r64)
    if pair_out:
        e = np.maximum(e - ulp32(r64), 0.0)
    a = np.abs(np.asarray(ref32, np.float64) - r64)
    ms = [np.abs(np.asarray(m, np.float64) - r64) for m in (model32 if isinstance(model32, (list, tuple)) else [model32])]
    f = dict(e_max=float(e.max()), r32_max=float(a.max()), m32_max=max(float(m.max()) for m in ms),
             e_p=float(np.percentile(e, PCT)), r32_p=float(np.percentile(a, PCT)), m32_p=max(float(np.percentile(m, PCT)) for m in ms),
             m32_each=[float(m.max()) for m in ms])
    bmax, bp = max(f["r32_max"], f["m32_max"]), max(f["r32_p"], f["m32_p"])
    f["ratio_max"] = f["e_max"] / bmax if bmax > 0 else (0.0 if f["e_max"] == 0 else float("inf"))
    f["ratio_p"] = f["e_p"] / bp if bp > 0 else (0.0 if f["e_p"] == 0 else float("inf"))
    ok = bool(np.isfinite(np.asarray(eng)).all()) and f["e_max"] <= FACTOR * bmax and f["e_p"] <= FACTOR * bp
    return ok, f
