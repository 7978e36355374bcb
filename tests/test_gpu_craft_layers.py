"""-m gpu: every layer of the f16x4 (split-operand) CRAFT path on its own against float64.

The detector's split kernels (conv3p.hip in its 32 / 64 / 128-wide, packed-pairs, fused-first and fused-head-tail forms, conv3h.hip, conv1u.hip, gemm2's split
1x1 / dilated loop, gemm_sp.hip's ks = 3 loop, conv1_split_kernel, the planes max-pool and upsample) are otherwise seen through the final heat map only, 27
layers downstream.  Here the engine's tap (Engine.craft_taps: where every tensor of one forward pass lives) hands each layer's own input and output, and the
layer is rebuilt ALONE on the CPU from the engine's exact input and the weight file (tests/craft_layer_ref.py: ref64, ref32, model32 - the split product
restated in two fp32 summation orders, the f16 MFMA's 8 products per rounding and torch's own convolution; the larger of their errors counts):

1. |engine - ref64| <= 1.5 x max(|ref32 - ref64|, |model32 - ref64|), in the maximum and at the 99.99th percentile, plus one fp32 ulp of |ref64| elementwise
   where the output is a pair, nothing where it is a triple or fp32 (1.5: the factor of test_x4_error_budget_against_fp64_*);
2. pure selections are exact: out_relu == max(out, 0), out_pool == 2x2 max, the planes max-pool, the planes upsample's own fp32 expression;
3. padding channels are exactly zero, also after the re-layouts head_packed 1 -> 0 -> 1 and craft_products 3 -> 4 -> 3;
4. everything finite; two tapped runs give identical tensors; craft_heatmap is bit-identical before and after a tapped run, and equal to the tapped heat.

Where a fusion hides a tensor the group is checked in one evaluation (canvas -> pooled conv1_2; conv_cls.4 -> .6 -> .8 -> heat; conv + pool), and the same canvas
runs again with the fusions off so that each member is seen alone.  A 1024 x 768 page is checked on row bands (craft_layer_ref.bands: each image's first and last
16 rows, a band across a patch-row seam, a quarter of the rows, all columns and channels; 1x1 layers and everything smaller on every pixel).

First MI355X run (profiles/craft_layers_fp64.md): stale padding channels in upconv4.3's output on small pages behind a large one (engine bug, fixed); slice5.1 at
1.71 x with model32 summed by torch's convolution alone (cause: the model's summation order, see craft_layer_ref.Layer.split_acc); every layer <= 1.31 / 1.35 since.

Every layer prints its figures; with TUATARA_LAYER_TABLE=<file> the rows are appended there as a markdown table (profiles/craft_layers_fp64.md)."""
import os
import time
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import craft_layer_ref as R

pytestmark = pytest.mark.gpu

NO_RELU = {"slice1.10", "slice2.17", "slice3.27", "slice4.37", "slice5.1", "slice5.2", "conv_cls.8"}      # oracle/models.py: the skips are pre-ReLU
CONV3 = {"slice1.0", "slice1.3", "slice1.7", "slice1.10", "slice2.14", "slice2.17", "slice3.20", "slice3.24", "slice3.27", "slice4.30", "slice4.34", "slice4.37",
         "slice5.1", "upconv1.3", "upconv2.3", "upconv3.3", "upconv4.3", "conv_cls.0", "conv_cls.2", "conv_cls.4"}
HEAD = {"upconv4.3", "conv_cls.0", "conv_cls.2", "conv_cls.4", "conv_cls.6", "conv_cls.8"}
UPCONV = {"upconv1.0", "upconv2.0", "upconv3.0", "upconv4.0", "upconv2.0.upsample", "upconv3.0.upsample", "upconv4.0.upsample"}
WIDE3 = {"slice1.7", "slice1.10", "slice2.14", "slice2.17", "slice3.20"}
DEEP3 = {"slice3.24", "slice3.27", "slice4.30", "slice4.34", "slice4.37", "upconv1.3", "upconv2.3"}
FUSIONS = ("first_fused", "head_tail", "head_persistent", "up_resident", "up_commute")
T0 = time.time()


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    from tuatara_amd import weights as W
    from tuatara_amd.engine import Engine
    R.set_threads()
    d = str(tmp_path_factory.mktemp("w_layers"))
    W.make_synthetic_weights(d, seed=0, structured=False)            # fully random: every layer carries signal
    e = Engine(d, precision="f16x4")
    _table("| canvas / knobs | layer | output | kernel kind | max abs(engine - ref64) | max abs(ref32 - ref64) | max abs(model32 - ref64): summed as the MFMA / by torch's conv | ratio max | ratio p99.99 |\n|---|---|---|---|---|---|---|---|---|\n")
    yield e, W.read_ttrw(os.path.join(d, W.CRAFT_FILE))
    e.close()
    print(f"tests/test_gpu_craft_layers.py: {time.time() - T0:.1f} s wall")
    _table(f"\nwall time of this file: {time.time() - T0:.1f} s\n")


def _table(line):
    path = os.environ.get("TUATARA_LAYER_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(line)


def _canvas(hw, seed, B=1):
    return np.random.default_rng(seed).integers(0, 256, (B, *hw, 3), dtype=np.uint8)


def _nchw(a):
    return torch.from_numpy(a).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


class _Run:
    """one tapped forward pass: the records by layer, tensors fetched on demand, assertions 3 and 4 on everything fetched"""

    def __init__(self, eng, canvases, label):
        self.eng, self.label = eng, label
        self.heat, recs = eng.craft_taps(canvases)
        self.layers = OrderedDict()
        for r in recs:
            assert r["role"] not in self.layers.setdefault(r["layer"], {}), (label, r)
            self.layers[r["layer"]][r["role"]] = r
        self.crc = {}

    def get(self, rec):
        a = self.eng.craft_tap_read(rec)
        key = (rec["layer"], rec["role"])
        self.crc[key] = zlib.crc32(a.tobytes())
        assert np.isfinite(a).all(), (self.label, key, "not finite")
        if rec["ld"] > rec["C"]:
            assert not a[..., rec["C"]:].any(), (self.label, key, "padding channels are not zero", float(np.abs(a[..., rec["C"]:]).max()))
        return a[..., :rec["C"]]


def _rows(a, bands_):
    return a if len(bands_) == 1 else np.concatenate([a[:, r0:r1] for r0, r1 in bands_], 1)


def _over(bands_, fn):
    """fn(r0, r1) -> dict of NCHW tensors for output rows [r0, r1); the bands joined along the rows, as NHWC numpy"""
    parts = [fn(r0, r1) for r0, r1 in bands_]
    return {k: np.concatenate([_nhwc(p[k]) for p in parts], 1) for k in parts[0]}


def _three(fn):
    """fn(mode) for mode in ref64 / ref32 / model32 (summed as the MFMA sums) / model32c (summed by torch's convolution) -> ref64, ref32, {output: [model32, model32c]}"""
    with torch.no_grad():
        a, b = fn("model32"), fn("model32c")
        return fn("ref64"), fn("ref32"), {k: [a[k], b[k]] for k in a}


def _order(mode):
    return "conv" if mode == "model32c" else "mfma"


def _check_layer(run, W, name, roles, banded, planes):
    """-> list of (role, kind, figures, ok)"""
    eng_t = {k: run.get(r) for k, r in roles.items()}
    out = []

    def judge(role, r64, r32, m32, bands_, pooled=False):
        rec = roles[role]
        bb = [(a // 2, b // 2) for a, b in bands_] if pooled else bands_
        ok, f = R.bar(_rows(eng_t[role], bb), r64, r32, m32, pair_out=rec["form"] in (1, 2))
        out.append((role, rec["kind"], f, ok))

    # ---- pure selections
    if name == "maxpool3x3":
        ref = _nhwc(torch.nn.functional.max_pool2d(_nchw(eng_t["in0"]), 3, 1, 1))
        assert np.array_equal(eng_t["out"], ref), (run.label, name, "planes max-pool is not the 3x3 maximum of its input")
        return out
    if name.endswith(".upsample"):
        ref = R.upsample2x_expr32(eng_t["in0"])
        d = np.abs(eng_t["out"].astype(np.float64) - ref)
        # a pair may sit one fp32 ulp off the value it was made from - or, below 2^-10, half the f16 subnormal spacing of its second plane: 2^-25 / 2^11
        lim = np.maximum(R.ulp32(ref), 2.0 ** -36) if roles["out"]["form"] == 2 else 0.0
        assert (d <= lim).all(), (run.label, name, "planes upsample is not its own fp32 expression", float(d.max()))
        return out

    H = roles["in1"]["H"] if "z" in roles else roles["canvas" if "canvas" in roles else "in0"]["H"]          # rows at the convolution's own resolution
    bands_ = R.bands(H, banded=banded and name in CONV3)
    wt, bs = W[name + ".w"], W[name + ".b"]
    dil = 6 if name == "slice5.1" else 1
    if "out" in roles and "out_relu" in roles:
        assert np.array_equal(eng_t["out_relu"], np.maximum(eng_t["out"], 0)), (run.label, name, "out_relu is not max(out, 0)")
    if "out" in roles and "out_pool" in roles:
        ref = _nhwc(torch.nn.functional.max_pool2d(_nchw(eng_t["out"]), 2).clamp_min(0))
        assert np.array_equal(eng_t["out_pool"], ref), (run.label, name, "out_pool is not the 2x2 maximum of ReLU(out)")

    # ---- the fused first pair: canvas -> conv1_1 -> ReLU -> conv1_2 -> ReLU -> pool
    if "canvas" in roles and name == "slice1.3":
        L0, L1 = R.Layer(W["slice1.0.w"], W["slice1.0.b"], planes=planes), R.Layer(wt, bs, planes=planes)
        c = _nchw(eng_t["canvas"])

        def grp(mode):
            x = c.double() / 255.0 if mode == "ref64" else c / 255.0
            dt = torch.float64 if mode == "ref64" else torch.float32

            def band(r0, r1):
                a0, a1 = max(r0 - 1, 0), min(r1 + 1, H)
                t = L0.model(x, 0, H, a0, a1) if mode.startswith("model32") else L0.plain(x, 0, H, a0, a1, dt)
                y = L1.model(t, a0, H, r0, r1, order=_order(mode)) if mode.startswith("model32") else L1.plain(t, a0, H, r0, r1, dt)
                return {"out_pool": R.pool2(y, True)}
            return _over(bands_, band)
        r64, r32, m32 = _three(grp)
        judge("out_pool", r64["out_pool"], r32["out_pool"], m32["out_pool"], bands_, pooled=True)
        return out

    # ---- conv_cls.4 with conv_cls.6 + conv_cls.8 in its epilogue: in0 -> heat
    if "heat" in roles and name == "conv_cls.4":
        L4, L6, L8 = R.Layer(wt, bs), R.Layer(W["conv_cls.6.w"], W["conv_cls.6.b"]), R.Layer(W["conv_cls.8.w"], W["conv_cls.8.b"], relu=False)
        x = _nchw(eng_t["in0"])

        def grp(mode):
            dt = torch.float64 if mode == "ref64" else torch.float32

            def band(r0, r1):
                if mode.startswith("model32"):
                    v = L4.model(x, 0, H, r0, r1, order=_order(mode))
                    return {"heat": L8.model(L6.model(v, r0, H, r0, r1, order=_order(mode)), r0, H, r0, r1, order=_order(mode))}
                v = L4.plain(x, 0, H, r0, r1, dt)
                return {"heat": L8.plain(L6.plain(v, r0, H, r0, r1, dt), r0, H, r0, r1, dt)}
            return _over(bands_, band)
        r64, r32, m32 = _three(grp)
        judge("heat", r64["heat"], r32["heat"], m32["heat"], bands_)
        return out

    # ---- a commuted up-convolution: z = W_up . y at the low resolution, out = ReLU(W_skip . skip + b + upsample(z))
    if "z" in roles:
        C0 = roles["in0"]["C"]
        La = R.Layer(wt[..., :C0], np.zeros_like(bs), relu=False, planes=planes)
        Lb = R.Layer(wt[..., C0:], bs, planes=planes)
        Lf = R.Layer(wt, bs, planes=planes)
        y, s = _nchw(eng_t["in0"]), _nchw(eng_t["in1"])
        Hl = H // 2

        def grp(mode):
            if mode.startswith("model32"):
                z = La.split_acc(y, 0, Hl, 0, Hl, order=_order(mode))
                o = (Lb.split_acc(s, 0, H, 0, H, order=_order(mode)) + Lb.b.view(1, -1, 1, 1) + R.upsample2x(z)).clamp_min(0)
            else:
                dt = torch.float64 if mode == "ref64" else torch.float32
                z = La.plain(y, 0, Hl, 0, Hl, dt)
                o = Lf.plain(torch.cat([R.upsample2x(y.to(dt)), s.to(dt)], 1), 0, H, 0, H, dt)
            return {"z": _nhwc(z), "out": _nhwc(o)}
        r64, r32, m32 = _three(grp)
        judge("z", r64["z"], r32["z"], m32["z"], [(0, Hl)])
        judge("out", r64["out"], r32["out"], m32["out"], [(0, H)])
        return out

    # ---- a convolution with whatever outputs it wrote (conv + pool alone where out is null)
    relu = name not in NO_RELU
    f32_kernel = name in ("conv_cls.6", "conv_cls.8")                  # the two 1x1 head layers run on the fp32 MFMA kernel: its model is fp32 itself
    in_form = roles["in0"]["form"] if "in0" in roles else 0
    L = R.Layer(wt, bs, dil=dil, relu=False, planes=3 if in_form == 3 else 2 if in_form in (1, 2) else planes)
    if "canvas" in roles:
        c = _nchw(eng_t["canvas"])
        x32, x64 = c / 255.0, c.double() / 255.0
    else:
        x32 = torch.cat([_nchw(eng_t[k]) for k in ("in0", "in1") if k in roles], 1)
        x64 = x32.double()
    outs = [k for k in ("out", "out_relu", "out_pool", "heat") if k in roles]

    def lay(mode):
        def band(r0, r1):
            if mode.startswith("model32") and not f32_kernel:
                y = L.model(x32, 0, H, r0, r1, order=_order(mode))
            else:
                y = L.plain(x64 if mode == "ref64" else x32, 0, H, r0, r1, torch.float64 if mode == "ref64" else torch.float32)
            d = {}
            if "out" in roles:
                d["out"] = y.clamp_min(0) if relu else y
            if "heat" in roles:
                d["heat"] = y
            if "out_relu" in roles:
                d["out_relu"] = y.clamp_min(0)
            if "out_pool" in roles:
                d["out_pool"] = R.pool2(y, True)
            return d
        return _over(bands_, band)
    r64, r32, m32 = _three(lay)
    for k in outs:
        judge(k, r64[k], r32[k], m32[k], bands_, pooled=k == "out_pool")
    return out


def _check(eng, W, canvases, label, banded=False, only=None, twice=False, expect=None):
    """One tapped pass over the canvases, every layer (or the layers in `only`) checked; -> the run.  Fails naming every layer over the bar."""
    planes = None
    run = _Run(eng, canvases, label)
    for roles in run.layers.values():                                   # planes per value of this pass: what the first planes tensor says
        for r in roles.values():
            if planes is None and r["form"] in (2, 3):
                planes = r["form"]
    bad = []
    for name, roles in run.layers.items():
        if only is not None and name not in only:
            continue
        for role, kind, f, ok in _check_layer(run, W, name, roles, banded, planes):
            line = (f"{label} | {name} | {role} | {kind} | {f['e_max']:.3e} | {f['r32_max']:.3e} | {' / '.join('%.3e' % v for v in f['m32_each'])} | {f['ratio_max']:.2f} | {f['ratio_p']:.2f}")
            print(("   " if ok else "!! ") + line)
            _table("| " + line + " |\n")
            if not ok:
                bad.append(line)
    if expect:
        for name in expect:
            assert name in run.layers, (label, name, "no tap record", list(run.layers))
    assert np.isfinite(run.heat).all()
    if twice:                                                           # assertion 4: a second tapped pass gives the same tensors
        again = _Run(eng, canvases, label + " (again)")
        assert np.array_equal(again.heat, run.heat)
        for name, roles in again.layers.items():
            for role, rec in roles.items():
                if (name, role) in run.crc:
                    again.get(rec)
                    assert again.crc[(name, role)] == run.crc[(name, role)], (label, name, role, "differs between two tapped runs")
    assert not bad, "layers over the bar (canvas | layer | output | kernel | e | ref32 | model32 | ratio max | ratio p99.99):\n" + "\n".join(bad)
    return run


class _Knobs:
    """set tuning keys for a block, restore the defaults behind it"""
    DEFAULTS = dict(first_fused=1, head_tail=1, head_persistent=1, up_resident=1, up_commute=1, craft_products=3, c3_c128_waves=4, c3_c32=1, c3_narrow64=2,
                    gsp_ks3=1, split_conv3p=1, up_2d=0, head_packed=1)

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


def test_full_page_every_layer_and_the_tap_changes_nothing(ctx):
    """1024 x 768, one page: the shipping kernels at every level (8 x 32 patches down to the 64 x 48 level's 16 x 16 patches).  The tap compiled in and switched
    off leaves craft_heatmap bit-identical: before a tapped run, after it, and equal to the heat map the tapped run returns."""
    eng, W = ctx
    cv = _canvas((1024, 768), 1)
    before = eng.craft_heatmap(cv[0])
    run = _check(eng, W, cv, "1024x768", banded=True, twice=True, expect=["slice1.3", "slice5.1", "upconv2.0", "conv_cls.4", "maxpool3x3"])
    assert eng.lib.ttr_dbg_craft_tap_count(eng.h) == sum(len(r) for r in run.layers.values())
    after = eng.craft_heatmap(cv[0])
    assert np.array_equal(before, after) and np.array_equal(before, run.heat[0])
    assert "canvas" in run.layers["slice1.3"] and "heat" in run.layers["conv_cls.4"] and "z" in run.layers["upconv4.0"]     # the fusions ran


def test_full_page_batch_of_two(ctx):
    """1024 x 768, two different pages in one launch: halos at the image boundary inside a batch, the 128-wide tiles the batch picks"""
    eng, W = ctx
    cv = np.concatenate([_canvas((1024, 768), 2), _canvas((1024, 768), 3)], 0)
    _check(eng, W, cv, "1024x768 B=2", banded=True)


@pytest.mark.parametrize("hw,B", [((576, 1024), 1), ((96, 160), 2), ((64, 96), 1), ((32, 32), 2)])
def test_smaller_canvases_every_pixel(ctx, hw, B):
    """the ragged page of the other tests, and levels that fall to gemm2's split loop: a map narrower than slice5.1's dilated footprint, maps where every pixel is
    a border pixel.  Every pixel of every layer."""
    eng, W = ctx
    _check(eng, W, _canvas(hw, hw[0] + hw[1], B), f"{hw[0]}x{hw[1]}" + (f" B={B}" if B > 1 else ""), twice=hw == (96, 160))


@pytest.mark.parametrize("value", [0, 255])
def test_constant_canvases(ctx, value):
    """all-zero (bias-only outputs) and all-255 (saturated first layer) at 128 x 256"""
    eng, W = ctx
    _check(eng, W, np.full((1, 128, 256, 3), value, np.uint8), f"128x256 all {value}")


@pytest.mark.parametrize("hw,banded", [((1024, 768), True), ((96, 160), False)])
def test_fusions_off_each_member_alone(ctx, hw, banded):
    """first_fused, head_tail, head_persistent, up_resident, up_commute off: conv1_1, conv1_2, the upsampled tensors, the two-source 1x1s and conv_cls.4 / .6 / .8
    each with tensors of their own"""
    eng, W = ctx
    with _Knobs(eng, **{k: 0 for k in FUSIONS}):
        run = _check(eng, W, _canvas(hw, 7), f"{hw[0]}x{hw[1]} fusions off", banded=banded,
                     expect=["slice1.0", "upconv2.0.upsample", "upconv4.0.upsample", "conv_cls.6", "conv_cls.8"])
    assert "canvas" not in run.layers["slice1.3"] and "z" not in run.layers["upconv4.0"] and "heat" in run.layers["conv_cls.8"]


KNOBS = [
    (dict(craft_products=4), (1024, 768), 1, None),
    (dict(craft_products=4), (96, 160), 2, None),
    (dict(c3_c128_waves=8), (1024, 768), 2, WIDE3),                    # (the 128-wide tiles a batch of two picks)
    (dict(c3_c32=0), (1024, 768), 1, HEAD & CONV3),                   # (32-wide tiles serve Cout <= 32)
    (dict(c3_narrow64=1), (1024, 768), 1, DEEP3),                      # (64-wide tiles on the 16 x 16-patch maps, Cout > 64)
    (dict(gsp_ks3=0), (1024, 768), 1, {"slice5.1"}),
    (dict(gsp_ks3=3), (1024, 768), 1, {"slice5.1"}),
    (dict(gsp_ks3=3), (1024, 768), 2, {"slice5.1"}),
    (dict(split_conv3p=0), (1024, 768), 1, CONV3),
    (dict(split_conv3p=0), (96, 160), 1, CONV3),
    (dict(up_2d=1), (1024, 768), 1, UPCONV),
    (dict(up_2d=1, up_resident=0), (576, 1024), 1, UPCONV),
    (dict(head_packed=0), (1024, 768), 1, HEAD),
    (dict(head_packed=0, head_tail=0), (96, 160), 1, HEAD),
]


@pytest.mark.parametrize("kv,hw,B,only", KNOBS, ids=[",".join(f"{k}={v}" for k, v in kv.items()) + f"@{hw[0]}x{hw[1]}x{B}" for kv, hw, B, _ in KNOBS])
def test_kernel_variants(ctx, kv, hw, B, only):
    """each selection knob on the canvases where it changes the kernel; the layers it cannot reach are left to the runs above"""
    eng, W = ctx
    label = f"{hw[0]}x{hw[1]}" + (f" B={B}" if B > 1 else "") + " " + ",".join(f"{k}={v}" for k, v in kv.items())
    with _Knobs(eng, **kv):
        _check(eng, W, _canvas(hw, 11, B), label, banded=hw == (1024, 768), only=only)


def test_padding_channels_stay_zero_across_relayouts(ctx):
    """head_packed 1 -> 0 -> 1 and craft_products 3 -> 4 -> 3 move the head tensors' zero padding channels (the workspaces start afresh): after every step the
    padding is exactly zero (asserted on every tensor _Run.get fetches) and the head layers are under the bar; the last heat map is the first one."""
    eng, W = ctx
    cv = _canvas((256, 192), 5)
    first = None
    for kv in (dict(head_packed=1), dict(head_packed=0), dict(head_packed=1), dict(head_packed=0, head_tail=0), dict(craft_products=3), dict(craft_products=4),
               dict(craft_products=4, head_packed=0), dict(craft_products=3)):
        with _Knobs(eng, **kv):
            run = _check(eng, W, cv, "256x192 relayout " + ",".join(f"{k}={v}" for k, v in kv.items()), only=HEAD)
        if kv in (dict(head_packed=1), dict(craft_products=3)):
            first = run.heat if first is None else first
            assert np.array_equal(first, run.heat)
