"""-m gpu: CRAFT's slice5.1 and slice5.2 folded into upconv1.0 (f16x4 engines, tuning key fc7_fold, the default).

slice5.1 (3x3, dilation 6), slice5.2 (1x1) and upconv1.0's fc7 columns (1x1) have no activation between them: the engine folds them at load time into one 3x3
of 512 -> 512 and runs upconv1.0 as two launches, z = W_skip . relu5_3 and out = ReLU(conv3x3_dil6(mp; Wf) / S + bf + z) (Engine::fc7_folded).

1. The folded pair against float64: from the engine's OWN mp and relu5_3 (the second tap list, Engine.craft_fold_taps) and the weight file, ref64 / ref32 = the
   ORIGINAL three layers in float64 / fp32; |out - ref64| <= 1.5 x |ref32 - ref64| at the maximum and the 99.99th percentile, plus one fp32 ulp where out is a pair
   (tests/fc7_fold_ref.judge -> craft_layer_ref.bar; tests/test_fc7_fold_cpu.py shows the fold's arithmetic meets that bar by itself).
2. Shapes: 256 x 320 as one page and as a batch of two (a 16 x 20 map: taps in and out of range, images bordering each other), 128 x 96 (an 8 x 6 map, narrower
   than the dilated footprint: the centre tap alone is ever in range), one 1024 x 768 page (the 64-row tiles); gsp_ks3 = 0 / 1 / 3 bit-identical to one another;
   craft_products = 4 once.
3. The switch: fc7_fold 1 -> 0 -> 1 reproduces the first heat map exactly; with 0 no folded launch runs and upconv1.0's output is, bit for bit, what a tapped
   pass with the fold on computes beside it from the three original layers.
4. End to end: 16 of the benchmark's pages with the fold on and off - every box equal, every string identical, heat maps within the end-to-end bar (1e-3,
   tests/test_gpu_x4_parity.py: TOL)."""
import os

import numpy as np
import pytest
import torch

from tests import craft_layer_ref as R
from tests import fc7_fold_ref as FR

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from tuatara_amd import weights as W
    from tuatara_amd.engine import Engine
    R.set_threads()
    d = str(tmp_path_factory.mktemp("w_fold"))
    W.make_synthetic_weights(d, seed=0, structured=False)            # fully random: every layer carries signal
    e = Engine(d, precision="f16x4")
    yield e, W.read_ttrw(os.path.join(d, W.CRAFT_FILE))
    e.close()


def _canvas(hw, B):
    return np.random.default_rng(hw[0] + hw[1] + B).integers(0, 256, (B, *hw, 3), dtype=np.uint8)


def _nchw(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2)


class _Knobs:
    DEFAULTS = dict(fc7_fold=1, gsp_ks3=1, craft_products=3)

    def __init__(self, eng, **kv):
        self.eng, self.kv = eng, kv

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                assert self.eng.set_tuning(k, v) == 0, k
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k in self.kv:
            self.eng.set_tuning(k, self.DEFAULTS[k])


def _tapped(eng, cv):
    """one tapped pass -> (heat, the three layers' records by (layer, role), the folded launches' records by role, their tensors)"""
    heat, recs = eng.craft_taps(cv)
    fold = {r["role"]: r for r in eng.craft_fold_taps()}
    t = {k: eng.craft_tap_read(r) for k, r in fold.items()}
    return heat, {(r["layer"], r["role"]): r for r in recs}, fold, t


def _judge(eng, W, cv, label, pair_out=True):
    heat, recs, fold, t = _tapped(eng, cv)
    assert set(fold) == {"in0", "in1", "z", "out"} and all(r["layer"] == "upconv1.0" for r in fold.values()), fold
    assert fold["z"]["form"] == 0 and fold["out"]["form"] == (2 if pair_out else 3) and all(np.isfinite(a).all() for a in t.values())
    assert ("slice5.1", "out") in recs and ("slice5.2", "out") in recs and ("upconv1.0", "out") in recs          # the three layers ran beside, with their records
    assert np.array_equal(t["in0"], eng.craft_tap_read(recs[("slice5.1", "in0")])) and np.array_equal(t["in1"], eng.craft_tap_read(recs[("upconv1.0", "in1")]))
    assert np.array_equal(t["in0"], torch.nn.functional.max_pool2d(_nchw(t["in1"]), 3, 1, 1).permute(0, 2, 3, 1).numpy())
    ok, f = FR.judge(t["out"], W, _nchw(t["in0"]), _nchw(t["in1"]), pair_out=pair_out)
    print(f"{label} | {fold['out']['kind']} | max |engine - ref64| {f['e_max']:.3e} | max |ref32 - ref64| {f['r32_max']:.3e} | ratio max {f['ratio_max']:.2f} | ratio p99.99 {f['ratio_p']:.2f}")
    assert ok, (label, f)
    return heat, t


@pytest.mark.parametrize("hw,B", [((256, 320), 1), ((256, 320), 2), ((128, 96), 1), ((1024, 768), 1)])
def test_folded_pair_against_float64(ctx, hw, B):
    eng, W = ctx
    cv = _canvas(hw, B)
    heat, _ = _judge(eng, W, cv, f"{hw[0]}x{hw[1]} B={B}")
    if B == 1:
        assert np.array_equal(heat[0], eng.craft_heatmap(cv[0]))                                                # the tapped pass is the untapped one


def test_folded_pair_exact_triples(ctx):
    eng, W = ctx
    with _Knobs(eng, craft_products=4):
        _judge(eng, W, _canvas((256, 320), 1), "256x320 B=1 craft_products=4", pair_out=False)


def test_folded_3x3_same_bits_on_every_loop(ctx):
    """gsp_ks3 = 0 (gemm2.hip's loop), 1 (gemm_sp.hip's, tile by shape), 3 (never the 64-row tile): the same sums in the same order, as slice5.1's own test asserts"""
    eng, W = ctx
    outs = {}
    for hw, B in (((256, 320), 1), ((256, 320), 2)):
        cv = _canvas(hw, B)
        for k in (1, 0, 3):
            with _Knobs(eng, gsp_ks3=k):
                heat, _, _, t = _tapped(eng, cv)
            outs[k] = (heat, t["z"], t["out"])
        for k in (0, 3):
            for a, b in zip(outs[1], outs[k]):
                assert np.array_equal(a, b), (hw, B, k)


def test_the_switch(ctx):
    eng, W = ctx
    cv = _canvas((256, 320), 2)
    first = np.stack([eng.craft_heatmap(c) for c in cv])
    _, recs_on, fold_on, _ = _tapped(eng, cv)
    side = eng.craft_tap_read(recs_on[("upconv1.0", "out")])              # u1a': the three layers, beside the folded launches
    with _Knobs(eng, fc7_fold=0):
        off = np.stack([eng.craft_heatmap(c) for c in cv])
        heat_off, recs_off, fold_off, _ = _tapped(eng, cv)
        assert not fold_off and np.array_equal(eng.craft_tap_read(recs_off[("upconv1.0", "out")]), side)
        assert ("slice5.1", "out") in recs_off and ("slice5.2", "out") in recs_off
    again = np.stack([eng.craft_heatmap(c) for c in cv])
    assert np.array_equal(first, again)
    scale = max(1.0, float(np.abs(off).max()))
    print(f"fc7_fold 1 vs 0, random weights 256x320: max |dheat| {np.abs(first - off).max():.3e} (max |heat| {scale:.2f})")
    assert np.abs(first - off).max() < TOL * scale


def test_end_to_end_boxes_and_strings_unchanged(eng_x4):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    P = 16
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=40, layout="cells5x8") for i in range(P)])
    buf = DeviceBuffer(pages.size)
    buf.upload(pages)
    key = lambda batch: [[(tuple(x["bbox"]), x["text"]) for x in pg] for pg in batch]
    try:
        on = key(eng_x4.pages_to_data_dev(buf, P, 1024, 768))
        heat_on = eng_x4.last_heat(P, 1024, 768)
        try:
            assert eng_x4.set_tuning("fc7_fold", 0) == 0
            off = key(eng_x4.pages_to_data_dev(buf, P, 1024, 768))
            heat_off = eng_x4.last_heat(P, 1024, 768)
        finally:
            eng_x4.set_tuning("fc7_fold", 1)
    finally:
        buf.free()
    n = sum(len(pg) for pg in on)
    d = float(np.abs(heat_on - heat_off).max())
    print(f"fc7_fold 1 vs 0, {P} benchmark pages: {n} boxes, max |dheat| {d:.3e} (max |heat| {float(np.abs(heat_off).max()):.2f})")
    assert n >= 20 * P
    for k in range(P):
        assert np.array_equal(np.array([b for b, _ in on[k]]), np.array([b for b, _ in off[k]])), k
        assert [t for _, t in on[k]] == [t for _, t in off[k]], k
    assert d < TOL
