"""The bars of tests/test_gpu_rowops.py and tests/test_gpu_split_gemm_range.py bite: on the CPU they accept correct fp32 forms and reject the wrong kernels they
are there to catch (tests/rowops_ref.py).  Nothing is ever broken on the GPU."""
import numpy as np
import pytest

from tests import craft_layer_ref as R
from tests import rowops_ref as RO


@pytest.fixture(scope="module")
def fams():
    R.set_threads()
    return RO.ln_families(np.random.default_rng(31), 5)


def _ratio(y, x, g, b, eps, pair=False):
    return float((np.abs(np.asarray(y, np.float64) - RO.ln64(x, g, b, eps)) / RO.ln_tol(x, g, b, eps, pair)).max())


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_ln_tol_accepts_fp32_layernorms(fams, eps):
    """numpy's fp32 two-pass form (pairwise sums) and torch's fp32 layer_norm sit well inside the worst-case bound on every family"""
    fam, g, b = fams
    for name, x in fam.items():
        a, t = _ratio(RO.ln32_two_pass(x, g, b, eps), x, g, b, eps), _ratio(RO.ln32_torch(x, g, b, eps), x, g, b, eps)
        k = _ratio(RO.ln32_tree(x, g, b, eps), x, g, b, eps)                 # the kernels' documented summation order
        print(f"eps {eps:g} {name:14s} two-pass {a:.3f} torch {t:.3f} tree {k:.3f}")
        assert a <= 0.5 and t <= 0.5 and k <= 0.5, (name, a, t, k)
        if name == "const":
            assert np.array_equal(RO.ln32_tree(x, g, b, eps), np.broadcast_to(b, x.shape))


def test_ln_tol_rejects_wrong_layernorms(fams):
    """a one-pass variance (on the offset rows), 1 / (D - 1) (on the unit rows), a missing eps (where eps dominates), gamma and beta swapped"""
    fam, g, b = fams
    eps = 1e-5
    worst = lambda f: max(_ratio(f(x), x, g, b, eps) for n, x in fam.items() if n != "const")
    for name in ("offset_1000", "offset_-30000"):
        x = fam[name]
        assert _ratio(RO.ln32_one_pass(x, g, b, eps), x, g, b, eps) > 50, name
    x = fam["unit"]
    assert _ratio(RO.ln32_two_pass(x, g, b, eps, ddof=1), x, g, b, eps) > 50
    x = fam["tiny_1e-6"]
    assert _ratio(RO.ln32_two_pass(x, g, b, eps, use_eps=False), x, g, b, eps) > 50
    assert _ratio(RO.ln32_two_pass(fam["unit"], g, b, eps, swap=True), fam["unit"], g, b, eps) > 50
    assert worst(lambda x: RO.ln32_two_pass(x, g, b, eps)) <= 0.5          # (the same sweep passes when nothing is broken)


def test_constant_rows_come_out_as_beta(fams):
    """sums of 384 equal powers of two are exact and fl(384 c) fl(1/384) = c: a correct two-pass kernel returns beta itself, and beta is its own exact triple"""
    fam, g, b = fams
    for c in RO.CONSTANTS:
        assert np.float32(np.float32(384.0) * np.float32(c)) * np.float32(1.0 / 384.0) == np.float32(c), c
    for eps in (1e-6, 1e-5):
        assert np.array_equal(RO.ln32_two_pass(fam["const"], g, b, eps), np.broadcast_to(b, fam["const"].shape))
    assert np.array_equal(RO.join_bits(RO.planes_bits(b, 3)), b.astype(np.float64))


def test_restated_split_meets_the_contract_on_the_edge_values():
    x = RO.edge_values()
    assert len(x) == 2 * (7 + 30 * 6 + 1) + 4096 and np.isfinite(x).all()
    for planes in (2, 3):
        for v in (x, np.maximum(x, 0)):
            ok, excess = RO.split_contract(v, RO.planes_bits(v, planes))
            assert ok, (planes, excess)
    # the contract bites: a truncating third plane, a flushed subnormal first plane, a truncating pair
    bits = RO.planes_bits(x, 3).copy()
    bits[..., 0, :] = np.where((bits[..., 0, :] & 0x7C00) == 0, bits[..., 0, :] & 0x8000, bits[..., 0, :])
    assert not RO.split_contract(x, bits)[0]
    bits = RO.planes_bits(x, 3).copy()
    bits[..., 2, :] = 0
    assert not RO.split_contract(x, bits)[0]
    bits = RO.planes_bits(x, 2).copy()
    bits[..., 1, :] &= 0xFFFC
    assert not RO.split_contract(x, bits)[0]


def test_untile_inverts_the_documented_layout():
    M, planes = 16, 3
    rows = np.arange(M * planes * RO.D, dtype=np.uint32).astype(np.uint16).reshape(M, planes, RO.D)
    raw = np.zeros(M * planes * RO.D, np.uint16)
    for m in range(M):
        for p in range(planes):
            for c in range(RO.D):
                raw[(((m // 8) * planes + p) * 6 + c // 64) * 512 + (m % 8) * 64 + c % 64] = rows[m, p, c]
    assert np.array_equal(RO.untile(raw, M, planes), rows)


@pytest.mark.parametrize("planes", [2, 3])
def test_grouped_gemm_bar_accepts_the_model_and_rejects_dropped_products(planes):
    """every scale group: model32 in either summation order passes as the engine; a model without x1 w0b and one without x0 w1 fail"""
    R.set_threads()
    x, w, groups, _ = RO.gemm_inputs(np.random.default_rng(5))
    r64, r32, ms = RO.gemm_refs(x, w, planes)
    assert np.abs(r64).max() < 60000
    for m in ms:
        ok, f = RO.grouped_bar(m, r64, r32, ms, groups, False)
        assert ok, f
    for name, f in RO.grouped_bar(ms[0], r64, r32, ms, groups, False)[1].items():
        assert 0.5 <= f["r32_max"] / f["m32_max"] <= 2.0, (name, f)          # the two halves of the bar are of one size in every group

    def drop_x1(xs, ws):
        xs[1].zero_()

    def drop_w1(xs, ws):
        ws[2].zero_()

    for mut in (drop_x1, drop_w1):
        bad = RO.gemm_refs(x, w, planes, mutate=mut, orders=("mfma",))[2][0]
        _, f = RO.grouped_bar(bad, r64, r32, ms, groups, False)
        assert all(not v["ok"] for v in f.values()), (mut.__name__, {k: (v["ratio_max"], v["ok"]) for k, v in f.items()})
