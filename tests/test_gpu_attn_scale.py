"""-m gpu: the attention kernels of the default precision (f16x4) away from unit scale, each on its own against float64.

The unit-scale tests (tests/test_gpu_attn.py, test_gpu_cross_attn.py, test_gpu_dec_self_attn.py) feed q, k ~ N(0, 1 .. 6) and v ~ 3 and judge with fixed bars.
Here every kernel meets the scale families of tests/attn_ref.py - unit, peaky, small K under large Q, small V down to the f16 subnormal range of plane 0,
large V, both small - and is held, in every family on its own, to the project's bar (craft_layer_ref.bar):

    |engine - ref64| <= 1.5 x max(|ref32 - ref64|, |model32 - ref64|)      in the maximum and at the 99.99th percentile,

ref32 = plain fp32 torch, model32 = the intended split arithmetic (planes as stored, the 2^-11 applied exactly, fp32 accumulation in the MFMA's order; both
orders of summing a score's four products).  Nothing is added for triple or fp32 outputs.  tests/test_attn_scale_cpu.py shows on the same inputs that the bar
rejects the f16 products plane / 2^11 the matrix-core kernels used to form (subnormal below 2^-3: 2 x to 1000 x fp32's error at small K and small V).

The matrix-core kernels: the fused qkv + attention tile (gemm_sp.hip, and qkv_attn4.hip: same bits), attn_split.hip, attn_cross_split.hip.  The vector-ALU
kernels (the other three cross-attention forms, the decoder's self-attention on both precisions, the fp32 encoder attention) are plain fp32 and run as
controls under the same bar.  Every case: finite outputs, bit-identical reruns, and `ATTN|kernel|family|max ratio|p ratio` lines."""
import functools
import time

import numpy as np
import pytest

from tests import attn_ref as A
from tests.test_gpu_dec_self_attn import _token_rows, _visible

pytestmark = pytest.mark.gpu

T0 = time.perf_counter()


def _twice(fn):
    a, b = fn(), fn()
    assert np.isfinite(a).all() and np.array_equal(a, b)
    return a


def _hold(kernel, got, refs, groups):
    ok, figs = A.judge(got, refs, groups)
    print(A.table(kernel, figs))
    print(f"ATTN|wall|{kernel}|{time.perf_counter() - T0:.1f} s since the file was imported")
    assert ok, (kernel, {n: (round(f["ratio_max"], 2), round(f["ratio_p"], 2)) for n, f in figs.items() if not f["ok"]})


# ---------------------------------------------------------------------------------------------------------------- the fused qkv + attention tile
@functools.lru_cache(maxsize=None)
def _fused(name):
    _, xs, heads = next(c for c in A.FUSED_CALLS + (A.FUSED_N7,) if c[0] == name)
    x, w, b = A.fused_inputs(np.random.default_rng(A.fused_seed(name)), xs, heads)
    return x, w, b, A.fused_three_ways(x, w, b), A.fused_groups(xs, heads, x.shape)


@pytest.mark.parametrize("name", [c[0] for c in A.FUSED_CALLS] + [A.FUSED_N7[0]])
def test_fused_qkv_attention_tile_in_every_family(eng_x4, name):
    """gemm_sp.hip's attention epilogue and its four-wave twin qkv_attn4.hip, N = 2 crops per call with the six heads as six families (W's and b's Q / K / V
    row blocks scaled within the nine binades of tests/test_gpu_split_gemm_range.py, whole x rows by powers of two), and one N = 7 call: 42 tiles, so that a
    workgroup takes a second tile.  References from x, W and b.  Both kernels hold the bar and agree bit for bit."""
    x, w, b, refs, groups = _fused(name)
    outs = {}
    try:
        for v in (0, 1):
            assert eng_x4.set_tuning(b"qkv_attn4", v) == 0
            outs[v] = _twice(lambda: eng_x4.dbg_qkv_attn(x, w, b))
    finally:
        eng_x4.set_tuning(b"qkv_attn4", 0)
    _hold(f"gemm_sp {name}", outs[0], refs, groups)
    _hold(f"qkv_attn4 {name}", outs[1], refs, groups)
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- attn_split.hip / the fp32 encoder attention
@functools.lru_cache(maxsize=None)
def _self(call):
    q, k, v, groups = A.head_case("split", 128, A.self_slots(call), 50 + call)
    return np.concatenate([q, k, v], -1), A.three_ways(q, k, v, "split"), groups


@pytest.mark.parametrize("call", range(A.SELF_CALLS))
def test_encoder_attention_alone_in_every_family(eng_x4, eng_f32, call):
    """ttr_dbg_attn_enc: on the f16x4 engine attn_split.hip the way the encoder runs it behind a separate qkv GEMM (fp32 qkv -> exact triples -> the kernel, which
    reads K and V as the first two planes of the triples); on the f32 engine the fp32 kernel, as a control.  N = 2 crops per call, a family per (crop, head)."""
    qkv, refs, groups = _self(call)
    _hold(f"attn_split {call}", _twice(lambda: eng_x4.dbg_attn_enc(qkv)), refs, groups)
    _hold(f"attn_enc f32 {call}", _twice(lambda: eng_f32.dbg_attn_enc(qkv)), refs, groups)


# ---------------------------------------------------------------------------------------------------------------- the decoder's cross-attention
FORMS = {"matrix cores": dict(cross_split=1, cross_crop=1), "per crop": dict(cross_split=0, cross_crop=1),
         "per row": dict(cross_split=0, cross_crop=0, cross_rows_hsplit=1), "per row, head groups": dict(cross_split=0, cross_crop=0, cross_rows_hsplit=4)}


@pytest.fixture
def knobs(eng_x4):
    def set_(**kw):
        for k, v in kw.items():
            assert eng_x4.set_tuning(k.encode(), v) == 0, k
    yield set_
    set_(cross_split=1, cross_crop=1, cross_rows_hsplit=4)


@functools.lru_cache(maxsize=None)
def _cross(R):
    q, k, v, groups = A.head_case("cross", R, A.cross_slots(2 if R == 26 else 1), 40 + R)
    return q, np.concatenate([k, v], -1), A.three_ways(q, k, v, "cross"), groups


@pytest.mark.parametrize("R", [26, 7])
def test_cross_attention_forms_in_every_family(eng_x4, knobs, R):
    """ttr_dbg_cross_attn, the four forms of tests/test_gpu_cross_attn.py: attn_cross_split.hip on the matrix cores, and the three vector-ALU forms (plain
    fp32: controls under the same bar).  A crop's 12 heads are one family: two crops per family at R = 26, one at R = 7.  The per-row forms agree bit for bit."""
    q, kv, refs, groups = _cross(R)
    got = {}
    for name, kn in FORMS.items():
        knobs(**kn)
        got[name] = _twice(lambda: eng_x4.dbg_cross_attn(q, kv))
    assert np.array_equal(got["per row"], got["per row, head groups"])
    for name in FORMS:
        _hold(f"cross {name} R={R}", got[name], refs, groups)


# ---------------------------------------------------------------------------------------------------------------- the decoder's self-attention (controls)
@pytest.fixture(params=["f16x4", "f32"])
def eng(request, eng_x4, eng_f32):
    return eng_x4 if request.param == "f16x4" else eng_f32


@functools.lru_cache(maxsize=None)
def _dec(mode):
    N = 6 if mode else 48                                                              # (one row per crop in mode 0: more crops, for groups of a size)
    q, kv, slots, out = A.dec_self_case(N, 70 + mode)
    tokens = _token_rows(N, 8)
    rows = list(range(26)) if mode else [25]
    vis = _visible(tokens, rows, mode)                                                 # [N, R, 26]
    h = lambda t: A.to_heads(t, 12)
    qh = h(np.broadcast_to(q[rows][None], (N, len(rows), 384)).copy())
    r64, r32, seq = A.masked_three_ways(qh, h(kv[..., :384]), h(kv[..., 384:]), np.repeat(vis, 12, 0))
    return q, kv, tokens, rows, tuple(A.from_heads(t, 12) for t in (r64, r32)) + ([A.from_heads(seq, 12)],), A.slot_groups(slots, out, 12, (N, len(rows), 384))


@pytest.mark.parametrize("mode", [0, 1])
def test_decoder_self_attention_in_every_family(eng, request, mode):
    """ttr_dbg_dec_self_attn on both precisions (the vector-ALU kernel: plain fp32, exact triples out on f16x4): AR step 25 (26 keys) and the 26 refinement
    rows with their masks (tests/test_gpu_dec_self_attn.py) of N = 6 crops (48 for the single row of the AR step), the 12 heads as the families; model32 here is a second fp32 evaluation that adds
    its products one by one."""
    q, kv, tokens, rows, refs, groups = _dec(mode)
    got = _twice(lambda: eng.dbg_dec_self_attn(q, kv, tokens, len(rows) if mode else 1, 0 if mode else rows[0], mode))
    _hold(f"dec_self {request.node.callspec.params['eng']} mode {mode}", got, refs, groups)
