"""GPU suite for local ink (DESIGN.md "Local ink"; tuatara_amd/csrc/ink.hip): ink_rows_kernel and ink_local_kernel through the stage call against the host rule
bit for bit - bits, bitsT and the record - on widths 1 to 193 at height 1, heights about the tile at width 70, radii 1, 16 and 64, windows that are not
dword-aligned and a 1300 x 1100 page; the engine's passes under it: deskew on 16 pages of one size (half of them inverted, auto polarity) and on a mixed-size
batch, tables on the shaded form through the list, device, mixed-size and streamed entry points against the fixed rule on the unshaded form, deskew on the shaded
tilted columns page against the layer-off result on the restatement's upright page; radius 0 against an engine that never called the setter; the stage call
after a poisoned scratch and after a larger page; pytuatara, ocr_cli and every refusal.  Every test here fails on the parent commit: Engine.set_local_ink /
Engine.ink_page and their symbols are absent."""
import numpy as np
import pytest

from tests import deskew_ref as D
from tests import ink_ref as R
from tests import tables_ref as T

pytestmark = pytest.mark.gpu

INK = (R.RADIUS, R.DROP, R.DARK)
TABLE_FIELDS = ("rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell")
ITEM_FIELDS = ("ids", "conf", "bbox", "quad")


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads) that batches mixed sizes; local ink, tables and deskew OFF at rest"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fresh(weights):
    """a second engine of the same configuration that never calls the ink setter"""
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


class layers:
    """local ink with tables and / or deskew on for a block; everything off again behind it"""
    def __init__(self, eng, ink=INK, tables=False, deskew=False):
        self.eng, self.ink, self.tables, self.deskew = eng, ink, tables, deskew

    def __enter__(self):
        self.eng.set_local_ink(self.ink)
        self.eng.set_tables(self.tables)
        self.eng.set_deskew(self.deskew)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_local_ink(False)
        self.eng.set_tables(False)
        self.eng.set_deskew(False)


def _dev(arr):
    from tuatara_amd.engine import DeviceBuffer
    arr = np.ascontiguousarray(arr)
    b = DeviceBuffer(arr.nbytes)
    b.upload(arr)
    return b


def stage_equals_host(eng, img, radius, drop, polarity, **kw):
    from tuatara_amd import engine as E
    got, want = eng.ink_page(img, radius, drop, polarity, **kw), E.ink_from_page(np.ascontiguousarray(img), radius, drop, polarity)
    assert R.same(got, want), (np.asarray(img).shape, radius, drop, polarity, kw, got["ink"], want["ink"])
    return got


# ------------------------------------------------------------------------------------------------- 1. the kernels against the host rule
@pytest.mark.parametrize("radius", [1, 16, 64])
def test_widths_1_to_193_at_height_1(eng, radius):
    page = R.random_page(radius, 1, 193)
    for w in range(1, 194):
        stage_equals_host(eng, page[:, :w], radius, (1, 255, 38)[w % 3], w % 3)


@pytest.mark.parametrize("radius", [1, 16, 64])
def test_heights_about_the_tile_at_width_70(eng, radius):
    """63, 64, 65 and 64 + R rows: the last row of a tile, the first of the next, and a vertical halo that reaches across the tile row"""
    page = R.random_page(radius, 64 + radius, 70)
    for h in (63, 64, 65, 64 + radius):
        for pol in (0, 1, 2):
            stage_equals_host(eng, page[:h], radius, 38, pol)


@pytest.mark.parametrize("offset,pad", [(3, 5), (1, 0), (4, 2), (2, 4)])
def test_a_window_that_is_not_dword_aligned(eng, offset, pad):
    """base and row stride that are no multiples of 4 (and the other ways of missing the alignment): the byte-load path gives the same bits"""
    for img, radius in ((R.random_page(4, 90, 333), 16), (R.shade(T.grid_page(), 0.35), 64), (R.random_page(5, 20, 257), 1)):
        w = img.shape[1]
        got = stage_equals_host(eng, img, radius, 38, 2, dev_offset=offset, dev_stride=3 * w + pad)
        assert R.same(got, eng.ink_page(img, radius, 38, 2))


@pytest.mark.parametrize("radius", [16, 64])
def test_a_page_of_many_tiles(eng, radius):
    """1300 x 1100: 5 x 21 tiles of the second pass, vertical halos across tile rows, horizontal halos across tile columns"""
    from tuatara_amd import synth
    page = R.shade(synth.synthetic_page(7, 1300, 1100, n_words=60), 0.35)
    got = stage_equals_host(eng, page, radius, 38, 0)
    assert got["bits"].any()
    want = R.ink_ref(page, radius, 38, 0)                                             # and the restatement itself, once at this size
    assert R.same(got, want)


def test_the_shared_pages_and_the_stated_consequences(eng):
    for img in (T.grid_page(), 255 - T.grid_page(), R.shade(T.grid_page(), 0.35), R.tie_page(), np.full((70, 300, 3), 255, np.uint8), np.zeros((70, 300, 3), np.uint8)):
        for pol in (0, 1, 2):
            stage_equals_host(eng, img, 16, 38, pol)
    a, b = eng.ink_page(T.grid_page(), 16, 38, R.DARK), eng.ink_page(255 - T.grid_page(), 16, 38, R.LIGHT)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["bitsT"], b["bitsT"]) and a["bits"].any()
    assert not eng.ink_page(np.zeros((70, 300, 3), np.uint8), 16, 38, 2)["bits"].any()


# ------------------------------------------------------------------------------------------------- 2. the engine's passes
def test_sixteen_pages_in_one_batch_half_of_them_inverted(eng):
    """deskew with local ink under auto polarity on 16 pages of one size: every page's skew record is the host rule's under the local mask, its ink record the
    host rule's, and the inverted pages are read as light ink"""
    from tuatara_amd import engine as E
    base = T.grid_page()
    slopes = (0, 5, -9, 18, 27, -37, 45, 2, -3, 12, -18, 33, 9, -27, 40, -5)
    pages = [D.tilt(base, s) if k % 2 == 0 else 255 - D.tilt(base, s) for k, s in enumerate(slopes)]
    with layers(eng, (16, 38, R.AUTO), deskew=True):
        res = eng.images_to_data(pages)
    for k, (p, r) in enumerate(zip(pages, res)):
        want = E.deskew_from_page_ink(p, D.MAX_SLOPE, D.GAIN, (16, 38, R.AUTO))
        assert r.skew == want["skew"], (k, r.skew, want["skew"])
        assert r.ink == E.ink_from_page(p, 16, 38, R.AUTO)["ink"] and r.ink["inverted"] == k % 2, (k, r.ink)
    assert sum(1 for r in res if r.skew["slope"] != 0) >= 8


def test_a_mixed_size_batch_of_two_pages(eng):
    from tuatara_amd import engine as E
    form = R.shade(D.tilt(D.form_page(words=True), 18), 0.35)
    pages = [form, np.ascontiguousarray(form[:470, :996])]
    with layers(eng, INK, deskew=True):
        res = eng.images_to_data(pages)
    for p, r in zip(pages, res):
        assert r.skew == E.deskew_from_page_ink(p, D.MAX_SLOPE, D.GAIN, INK)["skew"] and r.skew["slope"] != 0
        assert r.ink == E.ink_from_page(p, *INK)["ink"]


def _same_tables(a, b, what, items=True):
    assert a.table_mode == b.table_mode == 1, what
    for k in TABLE_FIELDS if items else TABLE_FIELDS[:4]:
        x, y = getattr(a, k), getattr(b, k)
        assert x is not None and y is not None and x.shape == y.shape and np.array_equal(x, y), (what, k)


def test_tables_on_the_shaded_form_equal_the_fixed_rule_on_the_clean_form(eng):
    """the list, device, mixed-size and streamed entry points: rulings, tables, lines and cells of the shaded form under the local rule are those of the clean form
    under the fixed rule, the words' tables and cells included; every word's cell is also the host rule's for the result's own quads"""
    from tuatara_amd import engine as E
    clean = D.form_page(words=True)
    shaded = R.shade(clean, 0.35)
    win_c, win_s = np.ascontiguousarray(clean[:470, :996]), R.shade(np.ascontiguousarray(clean[:470, :996]), 0.35)
    eng.set_tables((48, 128))
    try:
        want, want_win = eng.images_to_data([clean])[0], eng.images_to_data([win_c])[0]
        fixed = eng.images_to_data([shaded])[0]
    finally:
        eng.set_tables(False)
    assert len(want.table_rects) == 1 and len(want.cells) == 30 and (want.item_cell >= 0).sum() >= 20
    assert fixed.table_rects is None or len(fixed.table_rects) == 0                  # the fixed rule loses the table on the shaded form

    def check(res, page, ref, what):
        _same_tables(res, ref, what)                                                   # (item cells included: the detector boxes the same words on both pages)
        host = E.tables_from_page_ink(page, res.quad, 48, INK)
        assert np.array_equal(res.item_table, host["item_table"]) and np.array_equal(res.item_cell, host["item_cell"]), what
        assert res.ink == E.ink_from_page(page, *INK)["ink"], what

    bufs = []
    with layers(eng, INK, tables=(48, 128)):
        check(eng.images_to_data([shaded])[0], shaded, want, "list")
        lst = eng.images_to_data([shaded, win_s])                                    # one canvas, two sizes: a mixed batch
        check(lst[0], shaded, want, "mixed 0")
        check(lst[1], win_s, want_win, "mixed 1")
        ub = _dev(np.stack([shaded, shaded]))
        bufs.append(ub)
        for g in eng.pages_to_data_dev(ub, 2, *shaded.shape[:2]):
            check(g, shaded, want, "device")
        rows = []
        for k, p in enumerate((shaded, win_s)):                                      # page 1 with an odd row stride
            h, w = p.shape[:2]
            stride = w * 3 + (7 if k == 1 else 0)
            host = np.full((h, stride), 0xAB, np.uint8)
            host[:, :w * 3] = p.reshape(h, w * 3)
            bufs.append(_dev(host))
            rows.append((bufs[-1], h, w, stride if k == 1 else 0))
        got = eng.pages_to_data_dev_v(rows)
        check(got[0], shaded, want, "device rows 0")
        check(got[1], win_s, want_win, "device rows 1")
        streamed = []
        for push in (lambda: eng.stream_push_v(rows), lambda: eng.stream_push(ub, 2, *shaded.shape[:2]), lambda: eng.stream_push_v(rows[::-1])):
            r = push()
            if r:
                streamed.append(r)
        from tuatara_amd.engine import EngineError
        with pytest.raises(EngineError, match="streamed batches are in flight"):     # the setter and the stage call refuse while batches stream
            eng.set_local_ink(False)
        with pytest.raises(EngineError, match="streamed batches are in flight"):
            eng.ink_page(shaded)
        while True:
            r = eng.stream_flush()
            if not r:
                break
            streamed.append(r)
        assert len(streamed) == 3
        for batch, pages, refs in zip(streamed, ((shaded, win_s), (shaded, shaded), (win_s, shaded)), ((want, want_win), (want, want), (want_win, want))):
            for g, p, ref in zip(batch, pages, refs):
                check(g, p, ref, "streamed")
    for b in bufs:
        b.free()


def test_deskew_on_the_shaded_tilted_columns_page_equals_the_layer_off_result_on_the_upright_page(eng):
    shaded = R.shade(D.tilt(D.columns_page(), 27), 0.35)
    ref = R.deskew_ref_ink(shaded, D.MAX_SLOPE, D.GAIN, INK)
    assert ref["skew"]["slope"] == 27
    off = eng.images_to_data([ref["image"]], conf=True)[0]
    eng.set_deskew(True)
    try:
        fixed = eng.images_to_data([shaded])[0]
    finally:
        eng.set_deskew(False)
    assert fixed.skew["slope"] == 0 and fixed.skew["found"] == 27                     # the fixed rule finds the tilt and the gate refuses it
    with layers(eng, INK, deskew=True):
        on = eng.images_to_data([shaded], conf=True)[0]
    assert on.skew == ref["skew"], on.skew
    assert len(on) >= 8 and list(on.texts) == list(off.texts)
    for k in ITEM_FIELDS:
        assert np.array_equal(getattr(on, k), getattr(off, k)), k
    assert on.ink["inverted"] == 0 and (on.ink["radius"], on.ink["drop"], on.ink["polarity"]) == INK


def test_radius_0_is_an_engine_that_never_called_the_setter(eng, fresh, funsd):
    pages = [D.tilt(D.form_page(words=True), 18), funsd]
    for e in (eng, fresh):
        e.set_tables(True)
        e.set_deskew(True)
    try:
        eng.set_local_ink(INK)
        eng.set_local_ink(False)                                                      # on and off again: nothing of it is left
        assert eng.local_ink is None and fresh.local_ink is None
        for p in pages:
            a, b = eng.images_to_data([p], conf=True)[0], fresh.images_to_data([p], conf=True)[0]
            assert a.ink is None and b.ink is None and list(a.texts) == list(b.texts) and a.skew == b.skew
            for k in ITEM_FIELDS + TABLE_FIELDS:
                assert np.array_equal(getattr(a, k), getattr(b, k)), k
    finally:
        for e in (eng, fresh):
            e.set_tables(False)
            e.set_deskew(False)


def test_the_stage_call_whatever_the_engine_ran_before(eng, fresh):
    """after every fill of the poison hook, and after a larger page, the stage call's bytes are a fresh engine's (whose first ink call this is)"""
    small, big = R.random_page(9, 75, 201), R.shade(D.form_page(words=True), 0.5)
    want = fresh.ink_page(small, 16, 38, 2)
    assert R.same(want, R.ink_ref(small, 16, 38, 2))
    for pattern in (0, 1, 2):
        eng.ink_page(big, 64, 38, 2)
        eng.poison_scratch(pattern)
        assert R.same(eng.ink_page(small, 16, 38, 2), want), pattern
    eng.ink_page(big, 64, 200, 1)                                                     # a large page before the small one, nothing in between
    assert R.same(eng.ink_page(small, 16, 38, 2), want)
    assert R.same(eng.ink_page(small, 16, 38, 2, dev_offset=1, dev_stride=3 * 201 + 3), want)


# ------------------------------------------------------------------------------------------------- 3. refusals and callers
def test_refusals(eng):
    from tuatara_amd.engine import EngineError
    img = T.grid_page()
    for bad in ((65, 38, 0), (-1, 38, 0), (16, 0, 0), (16, 256, 0), (16, 38, 3), (16, 38, -1)):
        with pytest.raises(EngineError, match="ttr_engine_set_ink: radius must be 0 .off. or lie in 1..64"):
            eng.set_local_ink(bad)
        assert eng.local_ink is None
        with pytest.raises(EngineError, match="radius must lie in 1..64"):
            eng.ink_page(img, *bad)
    with pytest.raises(EngineError, match="radius must lie in 1..64"):
        eng.ink_page(img, 0, 38, 0)
    with pytest.raises(EngineError, match="bad device offset or stride"):
        eng.ink_page(img, 16, 38, 0, dev_offset=1, dev_stride=5)
    eng.set_local_ink(True)                                                           # accepted with neither tables nor deskew on: nothing runs
    try:
        assert eng.local_ink == (16, 38, 2)
        res = eng.images_to_data([D.form_page(words=True)])[0]
        assert res.ink is None and res.rulings is None and res.skew is None
        eng.set_tables((48, 128))                                                     # the stage calls keep the fixed rule, whatever the engine's setting
        from tuatara_amd import engine as E
        shaded = R.shade(T.grid_page(), 0.35)
        assert T.same(eng.tables_page(shaded, T.grid_words(), 16, 128), E.tables_from_page(shaded, T.grid_words(), 16, 128))
        assert D.same(eng.deskew_page(shaded, 64, 288, 128), E.deskew_from_page(shaded, 64, 288, 128))
        assert np.array_equal(eng.tables_debug(shaded, 16, 128)["bits"], T.ink_bits(shaded, 128))
    finally:
        eng.set_tables(False)
        eng.set_local_ink(False)


def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, monkeypatch, tmp_path):
    import os
    import subprocess
    import sys
    from PIL import Image
    from tests.conftest import ROOT
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    shaded = R.shade(D.form_page(words=True), 0.35)
    eng_x4.set_tables(True)                                                           # the callers' engine: plain crops
    eng_x4.set_local_ink(True)
    try:
        want = eng_x4.images_to_data([shaded])[0]
        want_bgr = eng_x4.images_to_data([np.ascontiguousarray(shaded[:, :, ::-1])])[0]   # (the CLI feeds BGR; the rule treats the channels alike)
    finally:
        eng_x4.set_tables(False)
        eng_x4.set_local_ink(False)
    assert (want.item_cell >= 0).sum() >= 20
    fixed = pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True)
    on = pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True, local_ink=True)
    assert all(d["cell"] == -1 for d in fixed)
    assert [d["text"] for d in on] == list(want.texts) and [d["cell"] for d in on] == want.item_cell.tolist()
    assert [d["cell"] for d in pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True, local_ink=(16, 38, 2))] == want.item_cell.tolist()
    assert all(d["cell"] == -1 for d in pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True))   # the call's setting is gone afterwards
    with pytest.raises(RuntimeError, match="radius must be 0 .off. or lie in 1..64"):
        pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True, local_ink=(65, 38, 2))
    with pytest.raises(TypeError, match="local_ink must be"):
        pytuatara.image_to_data(shaded, weights["dir"], "o", local_ink="yes")
    monkeypatch.setenv("TUATARA_LOCAL_INK", "1")                                      # the C++ switch
    assert [d["cell"] for d in pytuatara.image_to_data(shaded, weights["dir"], "o", tables=True)] == want.item_cell.tolist()
    monkeypatch.delenv("TUATARA_LOCAL_INK")
    png = str(tmp_path / "page.png")
    Image.fromarray(shaded).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--local-ink", "--tables", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    t0 = want_bgr.table_rects[0]
    assert lines[0] == "# table 0 " + " ".join(str(int(v)) for v in t0[:6])
    grid = want_bgr.table_grid(0)
    assert [ln.split("\t") for ln in lines[1:1 + int(t0[4])]] == [[c.replace("\n", " / ") for c in row] for row in grid]
    with_r = subprocess.run([cli, "--local-ink", "16", "--tables", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert with_r.returncode == 0 and with_r.stdout == out.stdout
    plain = subprocess.run([cli, "--tables", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert plain.returncode == 0 and not plain.stdout.startswith("# table 0")          # the fixed rule finds no table on the shaded form
    bad = subprocess.run([cli, "--local-ink", "65", "--tables", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode != 0 and "1..64" in bad.stderr
