"""CPU suite: tiled pages' host rule (tuatara_amd/csrc/geometry.cpp: tile_plan, stitch_tiles; DESIGN.md "Tiled pages") against tests/tiles_ref.py.
No GPU: ttr_tile_plan and ttr_stitch_tiles need no engine.  Fails on the parent commit, where the library exports neither."""
import numpy as np
import pytest

from tests import tiles_ref as R


@pytest.fixture(scope="module")
def E():
    from tuatara_amd.build import build_lib
    from tuatara_amd import engine

    build_lib()
    engine.load()
    return engine


def overlaps(S):
    return list(range(64, S // 4 + 1, 32))


@pytest.mark.parametrize("S", [256, 512, 1024])
def test_plan_equals_restatement_and_keeps_its_promises(E, S):
    """every L from 1 to 5 S + 6, every permitted O: the exported plan is the restatement, and section 1's invariants hold"""
    for O in overlaps(S):
        most = 0
        for L in range(1, 5 * S + 7):
            n = R.axis_invariants(L, S, O)
            most = max(most, n)
            p, ref = E.tile_plan(L, L, S, O), R.plan(L, L, S, O)
            got = dict(ny=p.ny, nx=p.nx, oy=p.oy, ox=p.ox, ey=p.ey, ex=p.ex, Hc=p.Hc, Wc=p.Wc, H2=p.H2, W2=p.W2)
            assert got == ref, (L, S, O, got, ref)
        assert most >= 6, (S, O, most)


def test_plan_of_an_a4_scan(E):
    p = E.tile_plan(3508, 2480, 1024, 128)
    assert (p.oy, p.ox, p.tiles) == ([0, 896, 1792, 2496], [0, 896, 1472], 12)
    assert (p.Hc, p.Wc, p.H2, p.W2) == (1024, 1024, 3520 // 2, 2496 // 2)
    q = E.tile_plan(700, 1000, 1024, 128)          # fits one tile: the canvas of the engine with tiling off
    assert (q.tiles, q.oy, q.ox, q.ey, q.ex, q.Hc, q.Wc) == (1, [0], [0], [700], [1000], 704, 1024)
    r = E.tile_plan(300, 3000, 1024, 128)          # the axes are independent
    assert (r.ny, r.Hc, r.nx, r.Wc) == (1, 320, 4, 1024)


PLANS = [(448, 640, (2, 3)), (500, 700, (3, 4)), (256, 700, (1, 4))]


@pytest.mark.parametrize("h,w,shape", PLANS)
def test_stitch_equals_numpy_bit_for_bit(E, h, w, shape):
    p = E.tile_plan(h, w, 256, 64)
    assert (p.ny, p.nx) == shape
    pages = 2
    t = R.seeded_tiles(11 + h, p.tiles, p.Hc // 2, p.Wc // 2, pages)
    assert np.isnan(t).any() and (t == 0).any() and (np.abs(t[np.isfinite(t)]) > 1e38).any() and ((np.abs(t) < 1e-38) & (t != 0)).any()
    got = E.stitch_tiles(t, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    assert got.shape == (pages, p.H2, p.W2, 2)
    for pg in range(pages):
        ref = R.stitch(t[pg * p.tiles:(pg + 1) * p.tiles], p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
        assert np.array_equal(got[pg].view(np.uint32), ref.view(np.uint32)), (pg, int((got[pg].view(np.uint32) != ref.view(np.uint32)).sum()))
    # outside the bands the map is a copy of one tile; inside a band it differs from both neighbours somewhere
    cy, cx = R.seams(p.oy, p.Hc // 2), R.seams(p.ox, p.Wc // 2)
    x0 = cx[0] - 8
    assert np.array_equal(got[1][:8, :x0].view(np.uint32), t[p.tiles][:8, :x0].view(np.uint32))
    assert not np.array_equal(got[1][:8, x0:x0 + 16], t[p.tiles][:8, x0:x0 + 16])
    if cy:
        assert np.array_equal(got[1][-8:, -8:].view(np.uint32), t[2 * p.tiles - 1][-8:, -8:].view(np.uint32))


def test_blend_weights_are_the_odd_thirtyseconds(E):
    """two constant tiles 0 and 1: the band reads (2 j + 1) / 32, j = 0..15, and nothing else is touched"""
    p = E.tile_plan(256, 448, 256, 64)
    assert (p.ny, p.nx, p.ox) == (1, 2, [0, 192])
    t = np.zeros((2, 128, 128, 2), np.float32)
    t[1] = 1.0
    got = E.stitch_tiles(t, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)[0]
    c = R.seams(p.ox, 128)[0]
    assert c == (96 + 0 + 128) // 2 and c % 8 == 0
    assert np.array_equal(got[5, :, 0], np.concatenate([np.zeros(c - 8), (2 * np.arange(16) + 1) / 32.0, np.ones(p.W2 - c - 8)]).astype(np.float32))


def _refused(E, *a):
    with pytest.raises(E.EngineError) as ei:
        E.tile_plan(*a)
    return str(ei.value)


def test_every_refusal_carries_its_message(E):
    assert "canvas_size must be a positive multiple of 32, got 1000" in _refused(E, 2000, 2000, 1000, 128)
    assert "overlap must be a multiple of 32 in [64, canvas_size / 4 = 256], got 48" in _refused(E, 2000, 2000, 1024, 48)
    assert "got 32" in _refused(E, 2000, 2000, 1024, 32)
    assert "got 288" in _refused(E, 2000, 2000, 1024, 288)
    assert "got 96" in _refused(E, 2000, 2000, 256, 96)
    assert "mag_ratio must be 1.0" in _refused(E, 2000, 2000, 1024, 128, 1.5)
    assert "at most 8192 pixels, got 8193" in _refused(E, 8193, 100, 1024, 128)
    assert "at most 16 tiles per axis, the width 4000 needs 21" in _refused(E, 100, 4000, 256, 64)
    assert "at most 64 tiles per page, 2000 x 2000 needs 11 x 11 = 121" in _refused(E, 2000, 2000, 256, 64)
    assert "Error reading image from file" in _refused(E, 0, 100, 1024, 128)
    assert E.tile_plan(8192, 1024, 1024, 64).ny == 9


def test_stitch_refuses_origins_it_cannot_take(E):
    t = np.zeros((2, 128, 128, 2), np.float32)

    def bad(oy, ox, H2, W2):
        with pytest.raises(E.EngineError) as ei:
            E.stitch_tiles(t, oy, ox, 256, 256, H2, W2)
        return str(ei.value)

    assert "the last tile must end at the map's end 200, it ends at 224" in bad([0], [0, 192], 128, 200)
    assert "origin 1 must be a multiple of 32" in bad([0], [0, 200], 128, 228)
    assert "overlap by 0 pixels" in bad([0], [0, 256], 128, 256)
    assert "origins must ascend" in bad([0], [0, 0], 128, 128)
    assert "the first origin must be 0" in bad([0], [32, 192], 128, 224)
