"""GPU suite for tables (DESIGN.md "Tables"; tuatara_amd/csrc/tables.hip): table_ink_kernel and table_grid_kernel through the stage call against the host rule
bit for bit on the pages of tests/test_tables_cpu.py (the widths about 64, runs across word boundaries and up to a row's last pixel, and the overflow pages
included); the developer hook's bitmap and run lists against numpy; a window 3 bytes into a device buffer with an odd row stride; a 1300 x 1100 page for a
multi-tile launch; page calls on the FUNSD page and on a synthetic page with a drawn grid - items identical to an engine without tables, table views equal to
the host rule on the page and the returned quads - through the list, mixed-size, device, streamed and tiled entry points; the views with the layer off; every
refusal.  Every test here fails on the parent commit: Engine.set_tables / Engine.tables_page and their symbols are absent."""
import numpy as np
import pytest

from tests import tables_ref as T

pytestmark = pytest.mark.gpu

VIEWS = ("rulings", "tables", "lines", "cells", "item_table", "item_cell")


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads) that batches mixed sizes; tables OFF at rest: every test that turns them on turns them off again"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


class tables_on:
    def __init__(self, eng, arg=True):
        self.eng, self.arg = eng, arg

    def __enter__(self):
        self.eng.set_tables(self.arg)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_tables(False)


def _grid_over(page, y0, x0, rows, cols, ch, cw):
    """draws a rows x cols grid of 2-px lines over a page, in place"""
    for i in range(rows + 1):
        T.hline(page, y0 + i * ch, x0, x0 + cols * cw + 1)
    for j in range(cols + 1):
        T.vline(page, x0 + j * cw, y0, y0 + rows * ch + 1)
    return page


@pytest.fixture(scope="module")
def grid_synth():
    """a synthetic page of words with a 6 x 4 grid drawn over it"""
    from tuatara_amd import synth
    return _grid_over(synth.synthetic_page(3, 512, 640, n_words=24), 20, 16, 6, 4, 78, 150)


@pytest.fixture(scope="module")
def big_page():
    from tuatara_amd import synth
    return _grid_over(synth.synthetic_page(7, 1300, 1100, n_words=60), 30, 25, 9, 5, 138, 209)


def _cases():
    out = [("grid", T.grid_page(), T.grid_words(), 16, 128), ("spans", T.grid_page(True, True), T.grid_words(), 16, 128), ("two tables", T.two_tables_page(), None, 16, 128),
           ("dashes: the run cap", T.dashes_page(), T.random_quads(0, 5, 400, 400), 16, 128)]
    L = T.grid_page()
    L[22:60, 50:52] = 255
    L[60:62, 12:50] = 255
    out.append(("an L-shaped merge", L, T.grid_words(), 16, 128))
    for deg in (1, 2, -2):
        img, q = T.rotated_grid(deg)
        out.append((f"rotated {deg}", img, q, 16, 128))
    bar = T.blank()
    bar[40:70, 30:130] = 0
    T.hline(bar, 100, 30, 129, t=12)
    out.append(("a bar and a thick ruling", bar, None, 16, 128))
    edge = T.blank(64, 128)
    T.hline(edge, 0, 0, 127); T.hline(edge, 62, 0, 127); T.vline(edge, 0, 0, 63); T.vline(edge, 126, 0, 63)
    out.append(("the page's edges", edge, np.array([[60, 30, 70, 30, 70, 36, 60, 36]], np.float32), 16, 128))
    for w in (1, 63, 64, 65, 129, 193, 257):
        img = T.blank(70, w)
        T.hline(img, 5, 0, w - 1); T.hline(img, 30, max(w - 20, 0), w - 1); T.vline(img, w - 1, 0, 69, t=1); T.vline(img, 0, 0, 69, t=1)
        if w > 66:
            T.hline(img, 40, 60, 66, t=1)         # a short run across the first word boundary: no run (7 px), and one of 14 px
            T.hline(img, 44, 55, 68, t=1)
        out.append((f"width {w}", img, None, 16, 128))
    th = T.blank(40, 100)
    th[10, 10:60] = (99, 100, 100)
    th[20, 10:60] = (100, 100, 100)
    out.append(("the ink threshold", th, None, 16, 100))
    comb = T.blank(600, 40)
    comb[0:600:2, 4:36] = 0
    out.append(("a comb: the ruling cap", comb, None, 16, 128))
    for name in ("two_caps_page", "many_lines_page", "many_tables_page", "many_cells_page"):   # -2 (not -4), -6, -6, -7
        img = getattr(T, name)()
        out.append((name, img, T.random_quads(3, 6, img.shape[0], img.shape[1]), 16, 128))
    for s in range(8):
        img = T.random_page(s, h=80 + 7 * s, w=120 + 11 * s, p=0.5 + 0.04 * s)
        out.append((f"random {s}", img, T.random_quads(s, 40, img.shape[0], img.shape[1]), 16 + s, 128))
    return out


# ------------------------------------------------------------------------------------------------- 1. the kernels against the host rule
def test_stage_call_equals_the_host_rule(eng):
    from tuatara_amd import engine as E
    modes = set()
    for name, img, quads, min_len, ink in _cases():
        want, got = E.tables_from_page(img, quads, min_len, ink), eng.tables_page(img, quads, min_len, ink)
        assert got["mode"] == want["mode"], name
        for k in VIEWS:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
        assert got["runs"] == want["runs"], name
        modes.add(got["mode"])
    assert modes == {1, -2, -4, -6, -7}
    by_name = {c[0]: c for c in _cases()}
    assert eng.tables_page(*by_name["two_caps_page"][1:])["mode"] == -2        # both directions' runs are counted before any ruling is formed


def test_debug_hook_bitmap_and_runs_equal_numpy(eng, big_page):
    for name, img, _, min_len, ink in _cases() + [("1300 x 1100", big_page, None, 48, 128)]:
        d = eng.tables_debug(img, min_len, ink)
        assert np.array_equal(d["bits"], T.ink_bits(img, ink)), name
        m = T.ink_mask(img, ink)
        rh, rv = T.runs_of(m), T.runs_of(m.T)
        assert d["mode"] == T.tables_ref(img, None, min_len, ink)["mode"], name
        if d["mode"] != 1:                                                            # a page beyond a cap reports its mode and nothing else
            assert len(d["runs_h"]) == 0 and len(d["runs_v"]) == 0, name
        else:
            assert d["runs_h"].tolist() == [list(r) for r in rh] and d["runs_v"].tolist() == [list(r) for r in rv], name


def test_funsd_run_counts_through_the_hook(eng, funsd):
    """the figures DESIGN.md states: 175 horizontal and 105 vertical runs"""
    d = eng.tables_debug(funsd, 48, 128)
    m = T.ink_mask(funsd, 128)
    assert (len(d["runs_h"]), len(d["runs_v"])) == (175, 105) == (len(T.runs_of(m)), len(T.runs_of(m.T)))
    assert np.array_equal(d["bits"], T.ink_bits(funsd, 128))


@pytest.mark.parametrize("offset,pad", [(3, 5), (1, 0), (4, 2), (2, 4)])
def test_a_window_that_is_not_dword_aligned(eng, offset, pad):
    """base 3 bytes into the device buffer and an odd row stride (and the other ways of missing the alignment): the byte-load path gives the same bits"""
    for img in (T.grid_page(), T.random_page(4, 90, 333), T.blank(70, 257)):
        w = img.shape[1]
        want, got = eng.tables_debug(img, 16, 128), eng.tables_debug(img, 16, 128, dev_offset=offset, dev_stride=3 * w + pad)
        assert np.array_equal(got["bits"], T.ink_bits(img, 128)) and np.array_equal(got["bits"], want["bits"])
        assert np.array_equal(got["runs_h"], want["runs_h"]) and np.array_equal(got["runs_v"], want["runs_v"])


def test_a_page_of_many_tiles(eng, big_page):
    """1300 x 1100: 5 x 21 tiles of the pixel pass, rows beyond one chunk of the grid pass"""
    from tuatara_amd import engine as E
    quads = T.random_quads(2, 200, 1300, 1100)
    want, got = E.tables_from_page(big_page, quads, 48, 128), eng.tables_page(big_page, quads, 48, 128)
    assert T.same(got, want) and len(got["tables"]) >= 1 and (got["item_cell"] >= 0).sum() > 50
    assert got["tables"][0, 4:6].tolist() == [9, 5]


# ------------------------------------------------------------------------------------------------- 2. page calls
def _items(res):
    return (list(res.texts), res.ids.tolist(), res.conf.tolist(), res.bbox.tolist(), res.quad.tolist())


def _views_equal_host(res, page, arg=(48, 128)):
    from tuatara_amd import engine as E
    want = E.tables_from_page(page, res.quad, *arg)
    assert res.table_mode == want["mode"]
    for k, got in (("rulings", res.rulings), ("tables", res.table_rects), ("lines", res.table_lines), ("cells", res.cells), ("item_table", res.item_table),
                   ("item_cell", res.item_cell)):
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k
    return want


def test_end_to_end(eng, funsd, grid_synth):
    for name, page in (("funsd", funsd), ("synthetic grid", grid_synth)):
        off = eng.images_to_data([page], conf=True)[0]
        assert off.rulings is None and off.item_table is None and off.tables == [] and off.table_mode == 0 and "table" not in off[0]
        with tables_on(eng):
            on = eng.images_to_data([page], conf=True)[0]
        assert len(on) >= 8 and _items(on) == _items(off), name                      # text, ids, conf, boxes, quads: every bit
        want = _views_equal_host(on, page)
        assert len(want["tables"]) >= 1 and (on.item_cell >= 0).any(), name
        d = on[int(np.nonzero(on.item_cell >= 0)[0][0])]
        assert d["table"] >= 0 and d["cell"] >= 0
        tabs = on.tables
        assert name != "funsd" or (len(tabs) == 3 and (tabs[0]["rows"], tabs[0]["cols"]) == (3, 5))
        assert len(tabs) == len(want["tables"]) and sum(len(t["cells"]) for t in tabs) == len(want["cells"])
        for t, tab in enumerate(tabs):
            grid = on.table_grid(t)
            assert len(grid) == tab["rows"] and all(len(r) == tab["cols"] for r in grid)
            for c in tab["cells"]:
                assert sorted(c["text"].split()) == sorted(w for i in c["items"] for w in on.texts[i].split()) and grid[c["row"]][c["col"]] == c["text"]
        assert eng.images_to_data([page], conf=True)[0].rulings is None              # off again


def test_other_settings_and_an_empty_page(eng, grid_synth):
    with tables_on(eng, (16, 200)):
        assert eng.tables == (16, 200)
        blank = np.full((64, 64, 3), 255, np.uint8)
        res = eng.images_to_data([grid_synth, blank])
        _views_equal_host(res[0], grid_synth, (16, 200))
        if len(res[1]) == 0:                                                          # an empty result: no views
            assert res[1].rulings is None and res[1].tables == [] and res[1].table_mode == 0
        else:                                                                         # (the detector may box a blank page's frame: then a page without rulings)
            assert len(_views_equal_host(res[1], blank, (16, 200))["rulings"]) == 0 and (res[1].item_cell == -1).all()
    assert eng.tables is None


def test_mixed_sizes_device_pages_and_streams(eng, funsd, grid_synth):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    small = np.ascontiguousarray(funsd[380:700, 40:680])                              # its own size: the first FUNSD table and some text
    pages = [funsd, grid_synth, small]
    with tables_on(eng):
        singles = [eng.images_to_data([p])[0] for p in pages]
        lst = eng.images_to_data(pages)
        for p, s, g in zip(pages, singles, lst):
            assert _items(g) == _items(s)
            _views_equal_host(g, p)
        bufs, rows = [], []
        for k, p in enumerate([grid_synth, grid_synth[:500, :630]]):                  # one canvas, two sizes; page 1 with an odd row stride
            h, w = p.shape[:2]
            stride = w * 3 + (7 if k == 1 else 0)
            host = np.full((h, stride), 0xAB, np.uint8)
            host[:, :w * 3] = np.ascontiguousarray(p).reshape(h, w * 3)
            b = DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
            rows.append((b, h, w, stride if k == 1 else 0))
        got = eng.pages_to_data_dev_v(rows)
        _views_equal_host(got[0], grid_synth)
        _views_equal_host(got[1], np.ascontiguousarray(grid_synth[:500, :630]))
        same = np.stack([grid_synth] * 2)
        ub = DeviceBuffer(same.nbytes)
        ub.upload(same)
        uni = eng.pages_to_data_dev(ub, 2, 512, 640)
        for g in uni:
            assert _items(g) == _items(singles[1])
            _views_equal_host(g, grid_synth)
        streamed = []
        for push in (lambda: eng.stream_push_v(rows), lambda: eng.stream_push(ub, 2, 512, 640), lambda: eng.stream_push_v(rows[::-1])):
            r = push()
            if r:
                streamed.append(r)
        with pytest.raises(EngineError, match="streamed batches are in flight"):     # the setter and the stage call refuse while batches stream
            eng.set_tables(False)
        with pytest.raises(EngineError, match="streamed batches are in flight"):
            eng.tables_page(grid_synth)
        while True:
            r = eng.stream_flush()
            if not r:
                break
            streamed.append(r)
        assert len(streamed) == 3
        for a, b in zip(streamed, [got, uni, got[::-1]]):
            for x, y in zip(a, b):
                assert _items(x) == _items(y) and x.cell_texts == y.cell_texts
                for k in ("rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell"):
                    assert np.array_equal(getattr(x, k), getattr(y, k)), k
    for b in bufs + [ub]:
        b.free()


def test_tiled_pages_read_the_page_at_its_own_scale(eng, big_page):
    eng.set_tiled(128)
    try:
        off = eng.images_to_data([big_page])[0]
        with tables_on(eng):
            on = eng.images_to_data([big_page])[0]
        assert on.tiles == 4 and _items(on) == _items(off)
        want = _views_equal_host(on, big_page)
        assert want["tables"][0, 4:6].tolist() == [9, 5]
    finally:
        eng.set_tiled(0)


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals(eng, grid_synth):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    for bad in ((15, 128), (4097, 128), (16, 0), (16, 256)):
        with pytest.raises(EngineError, match="ttr_engine_set_tables: min_len must be 0 .off. or lie in 16..4096 and ink in 1..255"):
            eng.set_tables(bad)
        assert eng.tables is None
        with pytest.raises(EngineError, match="min_len must lie in 16..4096 and ink in 1..255"):
            eng.tables_page(grid_synth, None, *bad)
    q = T.grid_words()
    q[2, 5] = -40000.0
    with pytest.raises(EngineError, match="quad 2 has a coordinate"):
        eng.tables_page(T.grid_page(), q, 16, 128)
    with tables_on(eng):                                                              # region calls leave the views empty
        out = eng.read_regions(grid_synth, [{"rect": (20, 24, 160, 60)}])
        assert len(out) == 1 and "table" not in out[0]
    buf = DeviceBuffer(grid_synth.nbytes)
    buf.upload(grid_synth)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            with pytest.raises(EngineError, match="ttr_engine_set_tables: tables are found by one engine alone, and a communicator is attached"):
                eng.set_tables(True)
            assert eng.tables is None
        finally:
            comm.attach(False)
        with tables_on(eng):
            with pytest.raises(EngineError, match="ttr_engine_attach_comm: tables are found by one engine alone"):
                comm.attach(True)
            with pytest.raises(EngineError, match="latency mode does not support tables"):
                comm.pages_to_data_sharded(buf, 1, 512, 640)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- 4. callers
def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, grid_synth, monkeypatch, tmp_path):
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
    with tables_on(eng_x4):                                                           # the callers' engine: plain crops
        want = eng_x4.images_to_data([grid_synth])[0]
        want_bgr = eng_x4.images_to_data([np.ascontiguousarray(grid_synth[:, :, ::-1])])[0]   # (the CLI feeds BGR)
    assert (want.item_cell >= 0).any()
    off = pytuatara.image_to_data(grid_synth, weights["dir"], "o")
    on = pytuatara.image_to_data(grid_synth, weights["dir"], "o", tables=True)
    assert "table" not in off[0] and [d["text"] for d in on] == [d["text"] for d in off] == list(want.texts)
    assert [d["table"] for d in on] == want.item_table.tolist() and [d["cell"] for d in on] == want.item_cell.tolist()
    assert [d["cell"] for d in pytuatara.image_to_data(grid_synth, weights["dir"], "o", tables=(48, 128))] == want.item_cell.tolist()
    assert "table" not in pytuatara.image_to_data(grid_synth, weights["dir"], "o")[0]        # the call's setting is gone afterwards
    with pytest.raises(RuntimeError, match="min_len in 16..4096"):
        pytuatara.image_to_data(grid_synth, weights["dir"], "o", tables=(15, 128))
    with pytest.raises(ValueError, match="regions"):
        pytuatara.image_to_data(grid_synth, weights["dir"], "o", tables=True, regions=[{"rect": (5, 5, 200, 25)}])
    png = str(tmp_path / "page.png")
    Image.fromarray(grid_synth).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--tables", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    t0 = want_bgr.table_rects[0]
    assert lines[0] == "# table 0 " + " ".join(str(int(v)) for v in t0[:6])
    grid = want_bgr.table_grid(0)
    assert [ln.split("\t") for ln in lines[1:1 + int(t0[4])]] == [[c.replace("\n", " / ") for c in row] for row in grid]
    bad = subprocess.run([cli, "--tables", "15", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode == 1 and "16..4096" in bad.stderr
