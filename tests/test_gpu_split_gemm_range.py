"""The split linears (tests/test_gpu_split_gemm.py has them at unit scale) across the f16 range: rows from 2^-12 (plane 0 in the f16 subnormals) to 2^13 (just
under the range guard), outlier input channels, weight rows over nine binades, GELU far beyond its table's +-8 on both sides, and fc2's input as it is - a GELU
output full of tiny negatives.  Every kernel form and epilogue is held to the project's own bar against float64 (tests/craft_layer_ref.py: bar; the split
product restated by Layer with ks = 1), separately on each group of rows that share a scale.  Inputs and references: tests/rowops_ref.py; that the grouped bar
rejects a dropped product in every group: tests/test_rowops_cpu.py."""
import numpy as np
import pytest

from tests import craft_layer_ref as R
from tests import rowops_ref as RO

pytestmark = pytest.mark.gpu

# (name, products, cfg, g2_split_stream): pairs on the streamlined kernels' three tiles, pairs on gemm2.hip's own loop, triples on two tiles, the skinny kernel
FORMS = [("pairs", 3, 2, 2), ("pairs", 3, 3, 2), ("pairs", 3, 6, 2), ("pairs_general", 3, 3, 0), ("pairs_general", 3, 6, 0), ("triples", 4, 3, 2),
         ("triples", 4, 6, 2), ("triples_skinny", 4, 7, 2)]
# (name, act, out_planes, residual)
EPILOGUES = [("f32", RO.ACT_NONE, 0, False), ("pairs_out", RO.ACT_NONE, 2, False), ("triples_out", RO.ACT_NONE, 3, False), ("residual", RO.ACT_NONE, 0, True),
             ("gelu", RO.ACT_GELU, 0, False)]


@pytest.fixture(scope="module")
def case():
    R.set_threads()
    rng = np.random.default_rng(5)
    x, w, groups, scale = RO.gemm_inputs(rng)
    resid = (rng.standard_normal((x.shape[0], w.shape[0])) * scale[:, None]).astype(np.float32)      # row-scaled: of the size of the row's outputs
    lin = {planes: RO.gemm_refs(x, w, planes) for planes in (2, 3)}
    assert np.abs(lin[3][0]).max() < 60000
    refs = {}
    for planes in (2, 3):
        for name, act, _, with_resid in EPILOGUES:
            refs[planes, name] = RO.gemm_epilogue(*lin[planes], resid if with_resid else None, act)
            assert np.abs(refs[planes, name][0]).max() < 60000
    g = refs[3, "gelu"][0]
    assert (lin[3][0] > 8).any() and (lin[3][0] < -8).any() and np.abs(g).max() > 8            # the table's clamp is reached on both sides
    return dict(x=x, w=w, groups=groups, resid=resid, refs=refs)


def _run(eng, x, w, products, act, out_planes, resid, cfg, stream):
    if stream == 2:
        return eng.dbg_split_gemm(x, w, None, np_products=products, act=act, out_planes=out_planes, resid=resid, cfg=cfg)
    assert eng.set_tuning("g2_split_stream", stream) == 0
    try:
        return eng.dbg_split_gemm(x, w, None, np_products=products, act=act, out_planes=out_planes, resid=resid, cfg=cfg)
    finally:
        assert eng.set_tuning("g2_split_stream", 2) == 0


@pytest.mark.parametrize("epi", EPILOGUES, ids=[e[0] for e in EPILOGUES])
@pytest.mark.parametrize("form", FORMS, ids=[f"{f[0]}-cfg{f[2]}" for f in FORMS])
def test_split_linear_holds_the_bar_in_every_scale_group(eng_x4, case, form, epi):
    fname, products, cfg, stream = form
    ename, act, out_planes, with_resid = epi
    r64, r32, ms = case["refs"][2 if products == 3 else 3, ename]
    got = _run(eng_x4, case["x"], case["w"], products, act, out_planes, case["resid"] if with_resid else None, cfg, stream)
    ok, f = RO.grouped_bar(got, r64, r32, ms, case["groups"], out_planes == 2)
    for n, v in f.items():
        print(f"ROWOPS|gemm|{fname} cfg {cfg}|{ename}|{n}|max {v['ratio_max']:.3f} p {v['ratio_p']:.3f}")
    assert ok, {n: (v["ratio_max"], v["ratio_p"]) for n, v in f.items()}


@pytest.fixture(scope="module")
def fc2_case():
    R.set_threads()
    rng = np.random.default_rng(9)
    M, K, N = 296, 1536, 384
    x = RO.gelu64(3.0 * rng.standard_normal((M, K))).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    resid = rng.standard_normal((M, N)).astype(np.float32)
    assert (x < 0).mean() > 0.4 and np.abs(x[x < 0]).min() < 1e-20
    return x, w, resid, RO.gemm_refs(x, w, 2, resid=resid)


@pytest.mark.parametrize("cfg", [0, 3, 6])
def test_fc2_like_linear_on_a_gelu_output(eng_x4, fc2_case, cfg):
    """x = GELU(3 z) in float64, rounded to fp32 (half of it negatives, from -0.17 down to far below the f16 subnormals), K = 1536 -> 384, as pairs plus a
    residual"""
    x, w, resid, (r64, r32, ms) = fc2_case
    M = x.shape[0]
    got = eng_x4.dbg_split_gemm(x, w, None, np_products=3, resid=resid, cfg=cfg)
    ok, f = RO.grouped_bar(got, r64, r32, ms, {"all": np.arange(M)}, False)
    print(f"ROWOPS|gemm|fc2-like pairs cfg {cfg}|residual|all|max {f['all']['ratio_max']:.3f} p {f['all']['ratio_p']:.3f}")
    assert ok, f
