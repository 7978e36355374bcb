"""CPU suite: folding slice5.1 and slice5.2 into upconv1.0 (tuning key fc7_fold) meets the per-layer bar by its own arithmetic.

The GPU test (tests/test_gpu_fc7_fold.py) holds the engine's folded launches to |out - ref64| <= 1.5 x |ref32 - ref64| with ref64 / ref32 the ORIGINAL
three-layer chain in float64 / fp32.  Here the split product of craft_layer_ref.Layer stands in for the kernels (tests/fc7_fold_ref.model: weights folded in
float64 and rounded to fp32, scaled and split as Engine::upload_linear does, products summed 8 at a time as the f16 MFMA sums them, or by torch's
convolution), on the real layer sizes and a 256 x 320 canvas pair run through the weight file's own trunk: if this misses the bar, no kernel can meet it.
Also: the folded weights reproduce the chain in float64 up to their own rounding to fp32, borders included."""
import os

import numpy as np
import pytest
import torch

from tests import craft_layer_ref as R
from tests import fc7_fold_ref as FR


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from tuatara_amd import weights as WW
    R.set_threads()
    d = str(tmp_path_factory.mktemp("w_fold_cpu"))
    WW.make_synthetic_weights(d, seed=0, structured=False)
    W = WW.read_ttrw(os.path.join(d, WW.CRAFT_FILE))
    canvas = np.random.default_rng(320).integers(0, 256, (2, 256, 320, 3), dtype=np.uint8)
    mp, c52 = FR.trunk32(W, canvas)
    return W, mp, c52


def test_the_fold_is_the_chain_in_float64(case):
    """conv(mp; Wf) + Wskip . relu5_3 + bf in float64 from the fp32-rounded folded weights against the three layers in float64: what is left is the rounding of
    Wf and bf to fp32: one rounding of at most 2^-25 relative per term of a 4608 + 512-term sum, where the fp32 chain rounds every term's product AND every
    partial sum of three layers in a row - so the fold's own error has to stay below the fp32 chain's, at the image borders as inside."""
    W, mp, c52 = case
    wf, bf, wskip = FR.fold(W)
    H = mp.shape[2]
    with torch.no_grad():
        ref = FR.chain(W, mp, c52, torch.float64)
        got = (R.Layer(wf, bf, dil=6, relu=False).plain(mp, 0, H, 0, H, torch.float64) +
               R.Layer(wskip, np.zeros(512, np.float32), relu=False).plain(c52, 0, H, 0, H, torch.float64)).clamp_min(0)
        r32 = FR.chain(W, mp, c52, torch.float32)
    d = (got - ref).abs()
    e32 = (r32.double() - ref).abs().max()
    print(f"fold vs chain in float64: max {float(d.max()):.3e} (border rows / columns {float(max(d[:, :, [0, -1]].max(), d[:, :, :, [0, -1]].max())):.3e}), "
          f"fp32 chain's own error {float(e32):.3e}, max |u1a| {float(ref.abs().max()):.3f}")
    assert float(d.max()) < float(e32)


@pytest.mark.parametrize("planes,order", [(2, "mfma"), (2, "conv"), (3, "mfma")])
def test_the_split_model_of_the_folded_pair_meets_the_bar(case, planes, order):
    W, mp, c52 = case
    with torch.no_grad():
        _, out = FR.model(W, mp, c52, planes=planes, order=order)
    ok, f = FR.judge(out.permute(0, 2, 3, 1).numpy(), W, mp, c52, pair_out=planes == 2)
    print(f"model planes={planes} order={order}: max |model - ref64| {f['e_max']:.3e}, |ref32 - ref64| {f['r32_max']:.3e}, ratio max {f['ratio_max']:.2f}, p99.99 {f['ratio_p']:.2f}")
    assert ok, f

