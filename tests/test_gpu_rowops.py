"""The three pieces under every f16x4 recogniser layer, each on its own against a plain reference (tests/rowops_ref.py): the inline-asm split
(split_planes_kernel: split3_pair / split2_pair of tuatara_amd/csrc/split.h) bit for bit against its restatement on chosen values, layernorm_planes_kernel /
ln384_row8 against float64 LayerNorm under a derived worst-case bound on rows far from unit scale, and gemm_skx.hip's LayerNorm prologue against the two
separate kernels.  tests/test_rowops_cpu.py shows that the bars reject the wrong kernels they are there for."""
import numpy as np
import pytest

from tests import craft_layer_ref as R
from tests import rowops_ref as RO

pytestmark = pytest.mark.gpu

PRED_MAX = float(np.nextafter(np.float32(RO.F16_MAX), np.float32(0)))


# ---------------------------------------------------------------------------------------------------------------- a. the split
def _edge_rows(ld):
    """the edge values cycled over 131 rows of 64 channels (every value at least once, the second cycle in other lanes); columns behind the 64th are NaN"""
    v = RO.edge_values()
    x = np.full((131, ld), np.nan, np.float32)
    x[:, :64] = np.resize(v, 131 * 64).reshape(131, 64)
    return x


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("ld", [64, 72])
def test_split_kernel_matches_its_restatement_bit_for_bit(eng_x4, ld, planes, relu):
    x = _edge_rows(ld)
    raw, tripped = eng_x4.dbg_split_planes(x, 64, planes=planes, relu=relu)
    v = np.maximum(x[:, :64], 0) if relu else x[:, :64]
    want = RO.planes_bits(v, planes)
    same = RO.same_bits(raw, want)
    bad = np.argwhere(~same)
    assert same.all(), [(float(v[m, c]), p, hex(raw[m, p, c]), hex(want[m, p, c])) for m, p, c in bad[:8]]
    ok, excess = RO.split_contract(v, raw)
    assert ok, excess
    assert tripped            # (the set holds values of 65504 and more: the largest significand at 2^15)


@pytest.mark.parametrize("planes", [2, 3])
def test_split_kernel_range_watch(eng_x4, planes):
    base = np.clip(_edge_rows(64), -PRED_MAX, PRED_MAX)
    assert np.abs(base).max() == np.float32(PRED_MAX)

    def trip(x, relu=0):
        return eng_x4.dbg_split_planes(x, 64, planes=planes, relu=relu)[1]

    assert not trip(base)                                     # max = pred(65504)
    for bad, relu, want in ((65504.0, 0, True), (-65504.0, 0, True), (np.inf, 0, True), (np.nan, 0, False), (-70000.0, 1, False), (-70000.0, 0, True)):
        x = base.copy()
        x[77, 13] = bad
        assert trip(x, relu) == want, (bad, relu)
    assert not trip(base)                                     # (each launch watches a fresh word)


# ---------------------------------------------------------------------------------------------------------------- b. LayerNorm
@pytest.fixture(scope="module")
def ln_case():
    fam, g, b = RO.ln_families(np.random.default_rng(31), 4)
    names = list(fam)
    x = np.concatenate([fam[n] for n in names] + [fam["unit"][:3]])          # 8 x 4 + 5 constant rows = 37 (ragged), + 3 = 40 = 8 k
    label = np.concatenate([np.full(len(fam[n]), i) for i, n in enumerate(names)] + [np.zeros(3, int)])
    assert x.shape == (40, RO.D)
    return dict(x=x, g=g, b=b, names=names, label=label, const=np.flatnonzero(label == names.index("const")))


def _ld(x, ld):
    out = np.full((x.shape[0], ld), np.nan, np.float32)
    out[:, :x.shape[1]] = x
    return out


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("ld", [384, 400])
def test_layernorm_planes_against_float64(eng_x4, ln_case, ld, eps):
    c = ln_case
    x, g, b = c["x"], c["g"], c["b"]
    y64 = RO.ln64(x, g, b, eps)
    joined = {}
    for planes in (3, 2):
        raw = eng_x4.dbg_layernorm_planes(_ld(x, ld), g, b, eps, planes=planes, tiled=0).reshape(40, planes, RO.D)
        tiled = RO.untile(eng_x4.dbg_layernorm_planes(_ld(x, ld), g, b, eps, planes=planes, tiled=1), 40, planes)
        assert np.array_equal(raw, tiled)
        ragged = eng_x4.dbg_layernorm_planes(_ld(x[:37], ld), g, b, eps, planes=planes, tiled=0).reshape(37, planes, RO.D)
        assert np.array_equal(raw[:37], ragged)
        y = joined[planes] = RO.join_bits(raw)
        ratio = np.abs(y - y64) / RO.ln_tol(x, g, b, eps, pair=planes == 2)
        for i, n in enumerate(c["names"]):
            print(f"ROWOPS|ln|ld {ld} eps {eps:g} planes {planes}|{n}|{ratio[c['label'] == i].max():.4f}")
        assert np.isfinite(y).all() and ratio.max() <= 1.0, [(n, float(ratio[c["label"] == i].max())) for i, n in enumerate(c["names"])]
        # constant rows: beta itself (as its planes), bit for bit
        want = np.broadcast_to(RO.planes_bits(b, planes), (len(c["const"]), planes, RO.D))
        assert RO.same_bits(raw[c["const"]], want).all()
        if planes == 3:
            assert np.array_equal(y[c["const"]], np.broadcast_to(b.astype(np.float64), (len(c["const"]), RO.D)))
    assert (np.abs(joined[2] - joined[3]) <= R.ulp32(joined[3]) + RO.SUB).all()


@pytest.mark.parametrize("planes", [2, 3])
def test_layernorm_rows_do_not_depend_on_their_neighbours(eng_x4, ln_case, planes):
    """every row of the batch equals the same row run alone, bit for bit (a reduction that crossed rows would not)"""
    c = ln_case
    x, g, b = c["x"], c["g"], c["b"]
    raw = eng_x4.dbg_layernorm_planes(x, g, b, 1e-5, planes=planes).reshape(40, planes, RO.D)
    for m in range(40):
        alone = eng_x4.dbg_layernorm_planes(x[m:m + 1], g, b, 1e-5, planes=planes).reshape(planes, RO.D)
        assert np.array_equal(raw[m], alone), m


# ---------------------------------------------------------------------------------------------------------------- c. the LayerNorm prologue
EPS_DEC = 1e-5


@pytest.fixture(scope="module")
def lnlin_case():
    R.set_threads()
    rng = np.random.default_rng(47)
    fam, g, b = RO.ln_families(rng, 5)
    names = [n for n in fam if n != "const"]
    x = np.concatenate([fam[n] for n in names])
    label = np.repeat(np.arange(len(names)), 5)
    assert x.shape == (40, RO.D)
    refs = {}
    for N in (768, 95):
        w = (rng.standard_normal((N, RO.D)) / np.sqrt(RO.D)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        r64 = RO.ln64(x, g, b, EPS_DEC) @ w.astype(np.float64).T + bias.astype(np.float64)
        r32 = RO.gemm_refs(RO.ln32_torch(x, g, b, EPS_DEC), w, 3, bias=bias)[1]               # the reference's own arithmetic: fp32 LayerNorm, fp32 linear
        ms = RO.gemm_refs(RO.ln32_tree(x, g, b, EPS_DEC), w, 3, bias=bias)[2]                 # the split product on the fp32 LayerNorm in the kernels' order
        refs[N] = (w, bias, r64, r32, ms)
    return dict(x=x, g=g, b=b, names=names, label=label, refs=refs)


@pytest.mark.parametrize("N", [768, 95])
@pytest.mark.parametrize("M", [40, 1, 17])
def test_layernorm_prologue_against_the_two_kernels_and_float64(eng_x4, lnlin_case, M, N):
    c = lnlin_case
    w, bias, r64, r32, ms = c["refs"][N]
    rows = np.arange(40) if M == 40 else np.array([12]) if M == 1 else np.arange(17) * 40 // 17       # (17 rows: two or three of every family)
    x = c["x"][rows]
    two = eng_x4.dbg_ln_linear(x, c["g"], c["b"], EPS_DEC, w, bias, fused=0)
    one = eng_x4.dbg_ln_linear(x, c["g"], c["b"], EPS_DEC, w, bias, fused=1)
    assert np.isfinite(two).all() and np.array_equal(one, two)
    groups = {n: np.flatnonzero(c["label"][rows] == i) for i, n in enumerate(c["names"]) if (c["label"][rows] == i).any()}
    ok, f = RO.grouped_bar(two, r64[rows], r32[rows], [m[rows] for m in ms], groups, False)
    for n, v in f.items():
        print(f"ROWOPS|lnlin|M {M} N {N}|{n}|max {v['ratio_max']:.3f} p {v['ratio_p']:.3f}")
    assert ok, {n: (v["ratio_max"], v["ratio_p"]) for n, v in f.items()}
