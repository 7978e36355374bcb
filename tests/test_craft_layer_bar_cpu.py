"""CPU suite: the per-layer bar of tests/test_gpu_craft_layers.py can tell a wrong split kernel from a right one.

Three representative layers at small maps (a 3x3 of 64 -> 64 with its fused 2x2 pool, slice5.1's 3x3 at dilation 6 at reduced width, upconv1.0's two-source
1x1 at reduced width; weights scaled as make_synthetic_weights scales them, ReLU-like inputs that are exact pairs, as the engine's tensors are).  For each:

* a correct kernel passes: the split product restated once more with the products summed in ANOTHER order (tap by tap, product by product - roughly what a
  K loop over taps does) and its output rounded to a pair stays under 1.5 x max(|ref32 - ref64|, |model32 - ref64|);
* deliberately broken CPU models miss it by at least 10 x: the x0 w1 product dropped in one 64-channel K chunk of one tap; x1 zeroed for one block of 64
  channels; one tap's w0b taken from the neighbouring tap; the left halo column taken as zero one pixel too early; the bias added after instead of before
  the pooled ReLU.  (The two tap faults need a 3x3; the pool fault needs the pool: each fault runs on every layer it is defined on.)

Nothing here touches a GPU, and nothing is ever broken on one: the broken variants are torch restatements only."""
import math

import numpy as np
import pytest
import torch

from tests import craft_layer_ref as R

MARGIN = 10.0


def _layer(seed, cin, cout, ks, dil, relu):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((cout, ks, ks, cin)) * math.sqrt(2.0 / (cin * ks * ks))).astype(np.float32)     # synth_craft: He-scaled, gain 2 under a BN
    b = (rng.standard_normal(cout) * 0.05).astype(np.float32)
    return R.Layer(w, b, dil=dil, relu=relu, planes=2)


def _input(seed, c, h, w):
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((2, c, h, w)).astype(np.float32)).clamp_min(0)
    return R.join(R.split_act(x, 2))            # exactly a pair, as every tensor the engine hands a layer


CASES = {
    "conv3x3_64_64_pool": dict(layer=lambda: _layer(1, 64, 64, 3, 1, True), x=lambda: _input(11, 64, 32, 64), pool=True),
    "slice5.1_dilated": dict(layer=lambda: _layer(2, 128, 256, 3, 6, False), x=lambda: _input(12, 128, 16, 24), pool=False),
    "upconv1.0_two_source_1x1": dict(layer=lambda: _layer(3, 256 + 128, 128, 1, 1, True), x=lambda: _input(13, 256 + 128, 16, 24), pool=False),
}


def _refs(case):
    L, x = case["layer"](), case["x"]()
    H = x.shape[2]
    fin = (lambda y: R.pool2(y, True)) if case["pool"] else (lambda y: y)
    with torch.no_grad():
        r64 = fin(L.plain(x, 0, H, 0, H, torch.float64)).numpy()
        r32 = fin(L.plain(x, 0, H, 0, H, torch.float32)).numpy()
        m32 = [fin(L.model(x, 0, H, 0, H)).numpy(), fin(L.model(x, 0, H, 0, H, order="conv")).numpy()]     # the bar of the GPU test: both summation orders
    return L, x, fin, r64, r32, m32


def _acc(L, xs, ws, H):
    """the three products of a pair, each tap on its own, summed product by product: another fp32 summation order than Layer.split_acc's"""
    ks = L.w.shape[-1]
    acc = None
    for xi, wi in ((0, 0), (1, 1), (0, 2)):
        for ky in range(ks):
            for kx in range(ks):
                wt = torch.zeros_like(ws[wi])
                wt[:, :, ky, kx] = ws[wi][:, :, ky, kx]
                y = R.conv_rows(xs[xi], 0, H, wt, L.dil, 0, H)
                acc = y if acc is None else acc + y
    return acc


@pytest.mark.parametrize("name", list(CASES))
def test_a_correct_kernel_in_another_summation_order_passes(name):
    R.set_threads()
    L, x, fin, r64, r32, m32 = _refs(CASES[name])
    H = x.shape[2]
    with torch.no_grad():
        w0, w0b, w1, inv = R.weight_planes(L.w)
        y = _acc(L, R.split_act(x, 2), [w0, w0b, w1], H) * inv + L.b.view(1, -1, 1, 1)
        y = fin(y.clamp_min(0) if L.relu else y)
        y = R.join(R.split_act(y, 2)).numpy()                       # written as a pair
    ok, f = R.bar(y, r64, r32, m32, pair_out=True)
    print(name, f)
    assert ok, f
    steps = L.w.shape[2] * L.w.shape[3] * L.w.shape[1] // R.STEP * 3     # the model is an fp32 summation itself, not a loose bound: a random walk of
    assert f["m32_max"] <= 2 * math.sqrt(steps) * R.ulp32(np.abs(r64).max()), f   # `steps` roundings of at most half an ulp of the largest value


def _drop_x0w1_chunk(xs, ws):
    ws[2][:, 0:64, ws[2].shape[2] // 2, 0] = 0


def _zero_x1_block(xs, ws):
    xs[1][:, -64:] = 0


def _w0b_from_neighbour_tap(xs, ws):
    ws[1][:, :, 1, 1] = ws[1][:, :, 1, 2]


def _halo_early(L, x, H):
    """taps that read to the left see column 0 as zero already (the halo column one pixel too early)"""
    w0, w0b, w1, inv = R.weight_planes(L.w)
    xs = R.split_act(x, 2)
    left = [t.clone() for t in (w0, w0b, w1)]
    rest = [t.clone() for t in (w0, w0b, w1)]
    for t in left:
        t[..., 1:] = 0
    for t in rest:
        t[..., 0] = 0
    xz = [t.clone() for t in xs]
    for t in xz:
        t[..., 0] = 0

    def acc(a, b):
        return R.conv_rows(torch.cat(a + [a[0]], 1), 0, H, torch.cat([b[0], b[1], b[2]], 1), L.dil, 0, H)

    y = (acc(xs, rest) + acc(xz, left)) * inv + L.b.view(1, -1, 1, 1)
    return y.clamp_min(0) if L.relu else y


def _bias_after_pool(L, x, H):
    return R.pool2(L.split_acc(x, 0, H, 0, H), True) + L.b.view(1, -1, 1, 1)


FAULTS = [(n, f) for n in CASES for f in ("drop_x0w1_chunk", "zero_x1_block")] + \
         [(n, f) for n in ("conv3x3_64_64_pool", "slice5.1_dilated") for f in ("w0b_from_neighbour_tap", "halo_early")] + \
         [("conv3x3_64_64_pool", "bias_after_pool")]


@pytest.mark.parametrize("name,fault", FAULTS)
def test_a_broken_model_misses_the_bar_by_10x(name, fault):
    R.set_threads()
    case = CASES[name]
    L, x, fin, r64, r32, m32 = _refs(case)
    H = x.shape[2]
    with torch.no_grad():
        if fault == "halo_early":
            y = fin(_halo_early(L, x, H))
        elif fault == "bias_after_pool":
            y = _bias_after_pool(L, x, H)
        else:
            y = fin(L.model(x, 0, H, 0, H, mutate=globals()["_" + fault]))
    ok, f = R.bar(y.numpy(), r64, r32, m32, pair_out=True)
    print(name, fault, f)
    assert not ok
    assert f["e_max"] >= MARGIN * R.FACTOR * max(f["r32_max"], f["m32_max"]) or f["e_p"] >= MARGIN * R.FACTOR * max(f["r32_p"], f["m32_p"]), f


def test_bands_cover_what_the_layer_test_promises():
    for H in (1024, 512, 256, 128, 64, 48, 16, 2):
        b = R.bands(H)
        assert b[0][0] == 0 and b[-1][1] == H and all(r0 % 2 == 0 and r1 % 2 == 0 for r0, r1 in b)
        assert b[0][1] >= min(16, H) and H - b[-1][0] >= min(16, H)
        assert sum(r1 - r0 for r0, r1 in b) * 4 >= H
        if len(b) > 1:
            assert any(r0 < s < r1 for r0, r1 in b[1:-1] for s in range(16, H, 16))      # an interior band across a patch-row seam


def test_split_act_is_split_h():
    """pairs: exact for about three values in four, one fp32 ulp off for the rest; triples: exact (above the range where the third plane is an f16 subnormal)"""
    x = torch.from_numpy((np.random.default_rng(5).standard_normal(1 << 16) * 3).astype(np.float32))
    j2, j3 = R.join(R.split_act(x, 2)), R.join(R.split_act(x, 3))
    big = x.abs() >= 2.0 ** -10
    assert torch.equal(j3[big], x[big]) and (j3 - x).abs().max() < 2.0 ** -35
    d = (j2 - x).abs().numpy()
    assert (d <= R.ulp32(x.numpy()))[big.numpy()].all() and 0.6 < (d == 0).mean() < 0.9
    v = np.random.default_rng(6).standard_normal((1, 3, 5, 8)).astype(np.float32)
    up = R.upsample2x_expr32(v)
    ref = R.upsample2x(torch.from_numpy(v).permute(0, 3, 1, 2).double()).permute(0, 2, 3, 1).numpy()
    assert np.abs(up - ref).max() <= 4 * R.ulp32(ref).max()


def test_weight_file_layers_chain_to_the_oracle(tmp_path):
    """The layer specs the GPU test rebuilds from the weight file (BN folded, [Cout][ks][ks][Cin], which layers skip their ReLU, slice5.1's dilation, the
    concat order of the up-convolutions) chained in fp32 give the heat map of the oracle's module built from the same state: folding and channel order are
    the file's."""
    import os
    import torch.nn.functional as F
    from oracle import pipeline
    from tuatara_amd import weights as WW
    R.set_threads()
    c, p = WW.make_synthetic_weights(str(tmp_path), seed=0, structured=False)
    W = WW.read_ttrw(os.path.join(str(tmp_path), WW.CRAFT_FILE))
    craft, _ = pipeline.load_models(c, p)
    canvas = np.random.default_rng(3).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    no_relu = {"slice1.10", "slice2.17", "slice3.27", "slice4.37", "slice5.1", "slice5.2", "conv_cls.8"}          # test_gpu_craft_layers.NO_RELU

    def conv(name, x):
        L = R.Layer(W[name + ".w"], W[name + ".b"], dil=6 if name == "slice5.1" else 1, relu=name not in no_relu)
        return L.plain(x, 0, x.shape[2], 0, x.shape[2], torch.float32)

    with torch.no_grad():
        x = torch.from_numpy(canvas).permute(2, 0, 1)[None].float() / 255.0
        p1 = F.max_pool2d(conv("slice1.3", conv("slice1.0", x)), 2)
        c22 = conv("slice1.10", conv("slice1.7", p1))
        c32 = conv("slice2.17", conv("slice2.14", F.max_pool2d(c22, 2).clamp_min(0)))
        p3 = F.max_pool2d(conv("slice3.20", c32.clamp_min(0)), 2)
        c42 = conv("slice3.27", conv("slice3.24", p3))
        p4 = F.max_pool2d(conv("slice4.30", c42.clamp_min(0)), 2)
        c52 = conv("slice4.37", conv("slice4.34", p4))
        fc7 = conv("slice5.2", conv("slice5.1", F.max_pool2d(c52, 3, 1, 1)))
        u = conv("upconv1.3", conv("upconv1.0", torch.cat([fc7, c52], 1)))
        for n, skip in (("upconv2", c42), ("upconv3", c32), ("upconv4", c22)):
            u = conv(n + ".3", conv(n + ".0", torch.cat([R.upsample2x(u), skip], 1)))
        for n in ("conv_cls.0", "conv_cls.2", "conv_cls.4", "conv_cls.6", "conv_cls.8"):
            u = conv(n, u)
    ref = pipeline.craft_heatmap(craft, canvas)
    got = u[0].permute(1, 2, 0).numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
