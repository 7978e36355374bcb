"""GPU suite for selection marks (DESIGN.md "Selection marks"; tuatara_amd/csrc/marks.hip): mark_cand_kernel and mark_page_kernel through the stage call against
the host rule bit for bit on the pages of tests/marks_ref.py (runs across word boundaries, the page's edges, 512 and 513 boxes, a 1300 x 1100 page of 35
bands); the hook's corner and band counts against numpy; windows that are not dword-aligned; page calls on the FUNSD page and on a synthetic form with drawn
boxes through the list, device, mixed-size, streamed and tiled entry points - items identical to marks off, views equal to the host rule on the returned
quads; batches asserted to hold no word, through the list, mixed-size, device and streamed entry points; tables and marks together; local ink on a shaded form; deskew on a tilted form; the stage call after a poisoned scratch;
the views with the layer off; every refusal.  Every test here fails on the parent commit: Engine.set_marks / Engine.marks_page and their symbols are absent."""
import numpy as np
import pytest

from tests import marks_ref as M

pytestmark = pytest.mark.gpu

ARG = (10, 64, 24, 128)


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads) that batches mixed sizes; marks OFF at rest: every test that turns them on turns them off again"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def fresh(weights):
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


class marks_on:
    def __init__(self, eng, arg=True):
        self.eng, self.arg = eng, arg

    def __enter__(self):
        self.eng.set_marks(self.arg)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_marks(False)


def _boxes_over(page, spots, t=1, ticked=(1,)):
    """clears a 28-px square at every spot and draws a 16-px frame in it, the `ticked` ones with an 8-px cross: found whatever the page held there"""
    for k, (x, y) in enumerate(spots):
        page[y - 6:y + 22, x - 6:x + 22] = 255
        M.frame(page, x, y, 16, t)
        if k in ticked:
            M.cross(page, x + 4, y + 4, 8)
    return page


SPOTS = [(10, 10), (170, 95), (330, 180), (490, 265), (10, 435), (600, 480)]


@pytest.fixture(scope="module")
def form_synth():
    """a synthetic page of words with six drawn boxes, the second one ticked"""
    from tuatara_amd import synth
    return _boxes_over(synth.synthetic_page(3, 512, 640, n_words=24), SPOTS)


@pytest.fixture(scope="module")
def big_form():
    from tuatara_amd import synth
    return _boxes_over(synth.synthetic_page(7, 1300, 1100, n_words=60), [(30 + 97 * k, 40 + 113 * k) for k in range(10)], t=2, ticked=(0, 3, 4))


def _same(got, want, what=""):
    for k in ("marks", "item_mark"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("mode", "corners", "kept"):
        assert got[k] == want[k], (what, k, got[k], want[k])


def _args(name):
    return (8, 128, 24, 128) if name.startswith("boxes") or name == "wide" else ARG


# ------------------------------------------------------------------------------------------------- 1. the kernels against the host rule
def test_stage_call_equals_the_host_rule(eng):
    from tuatara_amd import engine as E
    modes, found = set(), 0
    pages = dict(M.shared_pages())
    for s in range(4):
        pages[f"random {s}"] = M.random_page(s, h=90 + 13 * s, w=130 + 31 * s)
    for w in (1, 12, 63, 64, 65, 129):
        img = M.blank(40, w)
        if w >= 12:
            M.frame(img, w - 12, 3, 12, 1)
        pages[f"width {w}"] = (img, None)
    for name, (img, quads) in pages.items():
        want, got = E.marks_from_page(img, quads, *_args(name)), eng.marks_page(img, quads, *_args(name))
        _same(got, want, name)
        assert np.array_equal(want["marks"], M.marks_ref(img, quads, *_args(name))["marks"]), name
        modes.add(got["mode"])
        found += len(got["marks"])
    assert modes == {1, -6} and found >= 524
    assert eng.marks_page(M.hand_page())["marks"].tolist() == M.HAND_MARKS


def test_a_page_of_many_bands_and_the_hooks_counts(eng):
    """1300 x 1100: 35 bands, 21 words a row; the hook's corner count and band counts are numpy's"""
    from tuatara_amd import engine as E
    img, quads = M.many_bands_page()
    want = M.marks_ref(img, quads)
    _same(eng.marks_page(img, quads), E.marks_from_page(img, quads))
    _same(eng.marks_page(img, quads), want)
    d = eng.marks_debug(img)
    assert d["corners"] == want["corners"] == int(M.corners_of(M.ink_mask(img, 128)).sum())
    assert d["bands"].shape == (35, 2) and np.array_equal(d["bands"], want["bands"]) and (d["bands"][:, 0] > 0).sum() > 10
    assert np.array_equal(d["marks"], M.marks_ref(img)["marks"])                        # (the hook takes no items: labels -1)
    for name in ("hand", "boxes513"):
        img = M.shared_pages()[name][0]
        d, want = eng.marks_debug(img, *_args(name)), M.marks_ref(img, None, *_args(name))
        assert d["mode"] == want["mode"] and d["corners"] == want["corners"] and np.array_equal(d["bands"], want["bands"]), name


def test_funsd_through_the_hook(eng, funsd):
    """the figures DESIGN.md states: 3323 corners, no mark"""
    d = eng.marks_debug(funsd)
    assert d["mode"] == 1 and d["corners"] == 3323 and len(d["marks"]) == 0


@pytest.mark.parametrize("offset,pad", [(3, 5), (1, 0), (4, 2), (2, 4)])
def test_a_window_that_is_not_dword_aligned(eng, offset, pad):
    for img in (M.hand_page(), M.random_page(4, 90, 333)[0], M.shared_pages()["straddle"][0]):
        w = img.shape[1]
        want, got = M.marks_ref(img), eng.marks_debug(img, dev_offset=offset, dev_stride=3 * w + pad)
        assert got["corners"] == want["corners"] and np.array_equal(got["marks"], want["marks"]) and np.array_equal(got["bands"], want["bands"])


def test_the_stage_call_whatever_the_engine_ran_before(eng, fresh):
    """after every fill of the poison hook, and after a larger page, the stage call's bytes are a fresh engine's"""
    small, quads = M.random_page(5, 75, 201)
    big, bq = M.many_bands_page()
    want = fresh.marks_page(small, quads)
    _same(want, M.marks_ref(small, quads))
    for pattern in (0, 1, 2):
        eng.marks_page(big, bq)
        eng.poison_scratch(pattern)
        _same(eng.marks_page(small, quads), want, pattern)
    eng.marks_page(M.shared_pages()["boxes513"][0], None, 8, 64, 24, 128)                # a page beyond the cap before the small one, nothing in between
    _same(eng.marks_page(small, quads), want)


# ------------------------------------------------------------------------------------------------- 2. page calls
def _items(res):
    return (list(res.texts), res.ids.tolist(), res.conf.tolist(), res.bbox.tolist(), res.quad.tolist())


def _views_equal_host(res, page, arg=ARG, host=None):
    from tuatara_amd import engine as E
    want = host(page, res.quad) if host else E.marks_from_page(page, res.quad if len(res) else None, *arg)
    assert res.mark_mode == want["mode"]
    assert res.mark_recs.shape == want["marks"].shape and np.array_equal(res.mark_recs, want["marks"])
    assert res.item_mark.shape == want["item_mark"].shape and np.array_equal(res.item_mark, want["item_mark"])
    return want


def test_end_to_end(eng, funsd, form_synth):
    for name, page in (("funsd", funsd), ("synthetic form", form_synth)):
        off = eng.images_to_data([page], conf=True)[0]
        assert off.mark_recs is None and off.item_mark is None and off.marks == [] and off.mark_mode == 0 and "mark" not in off[0]
        with marks_on(eng):
            assert eng.marks == ARG
            on = eng.images_to_data([page], conf=True)[0]
        assert eng.marks is None
        assert len(on) >= 8 and _items(on) == _items(off), name                      # text, ids, conf, boxes, quads: every bit
        want = _views_equal_host(on, page)
        assert "mark" in on[0] and len(on.marks) == len(want["marks"])
        if name == "funsd":
            assert on.marks == []
        else:
            assert [m["box"][:2] for m in on.marks] == [list(s) for s in SPOTS] and [m["selected"] for m in on.marks] == [k == 1 for k in range(6)]
            m = on.marks[1]
            assert m["interior"] == [SPOTS[1][0] + 2, SPOTS[1][1] + 2, SPOTS[1][0] + 13, SPOTS[1][1] + 13] and m["fill"] == 16 / 144
            for m in on.marks:
                assert m["text"] == (on.texts[m["label"]] if m["label"] >= 0 else "")
        assert eng.images_to_data([page], conf=True)[0].mark_recs is None            # off again


class wordless:
    """Batches without a single word.  Under the suite's synthetic weights the detector boxes something on every page - one item on a blank page, thirteen on
    four drawn frames (measured) - so no page of the tree gives an empty detection by itself; the engine's own knob `detector_only` drops the detector's boxes
    before anything goes to the recogniser, which leaves exactly the batch an empty detection leaves: N = 0, no packer, no upload, no recogniser pass."""
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        assert self.eng.set_tuning("detector_only", 1) == 0
        return self.eng

    def __exit__(self, *a):
        assert self.eng.set_tuning("detector_only", 0) == 0


def _wordless_views(res, page, arg=ARG, host=None):
    """a result of a wordless batch: no item, and the page's marks all the same - every label -1, item_mark empty"""
    assert len(res) == 0 and res.item_mark.shape == (0,)
    want = _views_equal_host(res, page, arg, host)
    assert (want["marks"][:, 11] == -1).all()
    return want


def test_a_page_of_boxes_and_no_text(eng, form_synth):
    """the layer runs for a batch without words - a page of boxes only is a legitimate form - through the list, mixed-size, device and streamed entry points,
    behind a batch with words in the same slot, and under local ink; every call here asserts that its batch held no word"""
    from tests import ink_ref as R
    from tuatara_amd import engine as E
    from tuatara_amd.engine import DeviceBuffer
    page = _boxes_over(M.blank(256, 256), [(20, 20), (120, 20), (20, 120), (200, 200)], ticked=(2,))
    small = _boxes_over(M.blank(250, 240), [(30, 40), (150, 100)], t=2, ticked=(0,))   # (shares the 256 x 256 canvas: one mixed batch with `page`)
    blank = M.blank(256, 256)
    with wordless(eng):
        off = eng.images_to_data([page])[0]
        assert len(off) == 0 and off.mark_recs is None and off.item_mark is None and off.mark_mode == 0
    with marks_on(eng):
        wordy = eng.images_to_data([form_synth])[0]                                   # a batch with words first: its side block and its items' marks lie in the slot
        assert len(wordy) >= 8 and len(wordy.mark_recs) == 6
        with wordless(eng):
            res = eng.images_to_data([page])[0]
            want = _wordless_views(res, page)
            assert len(want["marks"]) == 4 and want["marks"][:, 10].tolist() == [0, 0, 1, 0] and res.marks[2]["selected"] and res.marks[2]["text"] == ""
            two = eng.images_to_data([page, blank])                                   # a uniform batch of two
            assert sum(len(r) for r in two) == 0
            _wordless_views(two[0], page)
            assert len(_wordless_views(two[1], blank)["marks"]) == 0
            mixed = eng.images_to_data([page, small, form_synth])                     # sizes of their own: the page table, and a page whose words are dropped
            assert sum(len(r) for r in mixed) == 0
            _wordless_views(mixed[0], page)
            assert len(_wordless_views(mixed[1], small)["marks"]) == 2
            assert len(_wordless_views(mixed[2], form_synth)["marks"]) == 6
            same = np.stack([page, blank, page])
            ub = DeviceBuffer(same.nbytes)
            ub.upload(same)
            try:
                dev = eng.pages_to_data_dev(ub, 3, 256, 256)
                assert sum(len(r) for r in dev) == 0
                streamed = []
                for _ in range(3):
                    r = eng.stream_push(ub, 3, 256, 256)
                    if r:
                        streamed.append(r)
                while True:
                    r = eng.stream_flush()
                    if not r:
                        break
                    streamed.append(r)
                assert len(streamed) == 3
                for batch in [dev] + streamed:
                    assert sum(len(r) for r in batch) == 0
                    for r, p in zip(batch, (page, blank, page)):
                        _wordless_views(r, p)
            finally:
                ub.free()
            ink = (R.RADIUS, R.DROP, R.DARK)
            shaded = R.shade(page, 0.35)
            eng.set_local_ink(ink)
            try:
                li = eng.images_to_data([shaded])[0]
            finally:
                eng.set_local_ink(False)
            got = _wordless_views(li, shaded, host=lambda p, q: E.marks_from_page_ink(p, None, *ARG[:3], local_ink=ink))
            assert got["marks"][:, :4].tolist() == want["marks"][:, :4].tolist() and li.ink == E.ink_from_page(shaded, *ink)["ink"]
        again = eng.images_to_data([form_synth])[0]                                   # and words again behind the wordless batches
        assert _items(again) == _items(wordy) and np.array_equal(again.mark_recs, wordy.mark_recs) and np.array_equal(again.item_mark, wordy.item_mark)


def test_mixed_sizes_device_pages_and_streams(eng, funsd, form_synth):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    small = np.ascontiguousarray(form_synth[60:500, 100:630])
    pages = [funsd, form_synth, small]
    bufs, rows = [], []
    lst_off = eng.images_to_data(pages)                                               # every call's items with marks off: what marks on must leave bit for bit
    with marks_on(eng):
        lst = eng.images_to_data(pages)
        for p, s, g in zip(pages, lst_off, lst):
            assert _items(g) == _items(s)
            _views_equal_host(g, p)
        for k, p in enumerate([form_synth, form_synth[:500, :630]]):                  # one canvas, two sizes; page 1 with an odd row stride
            h, w = p.shape[:2]
            stride = w * 3 + (7 if k == 1 else 0)
            host = np.full((h, stride), 0xAB, np.uint8)
            host[:, :w * 3] = np.ascontiguousarray(p).reshape(h, w * 3)
            b = DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
            rows.append((b, h, w, stride if k == 1 else 0))
        same = np.stack([form_synth] * 2)
        ub = DeviceBuffer(same.nbytes)
        ub.upload(same)
        bufs.append(ub)
        eng.set_marks(False)
        got_off, uni_off = eng.pages_to_data_dev_v(rows), eng.pages_to_data_dev(ub, 2, 512, 640)
        eng.set_marks(True)
        got = eng.pages_to_data_dev_v(rows)
        assert [_items(g) for g in got] == [_items(g) for g in got_off]
        assert len(_views_equal_host(got[0], form_synth)["marks"]) == 6
        assert len(_views_equal_host(got[1], np.ascontiguousarray(form_synth[:500, :630]))["marks"]) == 6
        uni = eng.pages_to_data_dev(ub, 2, 512, 640)
        for g, o in zip(uni, uni_off):
            assert _items(g) == _items(o)
            _views_equal_host(g, form_synth)
        fb = DeviceBuffer(funsd.nbytes)                                               # the FUNSD page through the same calls: device rows, a uniform device batch, streams
        fb.upload(np.ascontiguousarray(funsd))
        bufs.append(fb)
        frow = [(fb, funsd.shape[0], funsd.shape[1], 0)]
        eng.set_marks(False)
        f_off = eng.pages_to_data_dev(fb, 1, *funsd.shape[:2])[0]
        eng.set_marks(True)
        f_v, f_uni = eng.pages_to_data_dev_v(frow)[0], eng.pages_to_data_dev(fb, 1, *funsd.shape[:2])[0]
        for g in (f_v, f_uni):
            assert len(g) >= 8 and _items(g) == _items(f_off)
            assert len(_views_equal_host(g, funsd)["marks"]) == 0
        streamed = []
        for push in (lambda: eng.stream_push_v(rows), lambda: eng.stream_push(ub, 2, 512, 640), lambda: eng.stream_push_v(rows[::-1]),
                     lambda: eng.stream_push(fb, 1, *funsd.shape[:2]), lambda: eng.stream_push_v(frow)):
            r = push()
            if r:
                streamed.append(r)
        with pytest.raises(EngineError, match="streamed batches are in flight"):     # the setter and the stage call refuse while batches stream
            eng.set_marks(False)
        with pytest.raises(EngineError, match="streamed batches are in flight"):
            eng.marks_page(form_synth)
        while True:
            r = eng.stream_flush()
            if not r:
                break
            streamed.append(r)
        assert len(streamed) == 5
        for a, b in zip(streamed, [got, uni, got[::-1], [f_uni], [f_v]]):
            for x, y in zip(a, b):
                assert _items(x) == _items(y) and x.mark_mode == y.mark_mode
                assert np.array_equal(x.mark_recs, y.mark_recs) and np.array_equal(x.item_mark, y.item_mark)
    for b in bufs:
        b.free()


def test_tiled_pages_read_the_page_at_its_own_scale(eng, big_form, funsd):
    eng.set_tiled(128)
    try:
        off, f_off = eng.images_to_data([big_form])[0], eng.images_to_data([funsd])[0]
        with marks_on(eng):
            on, f_on = eng.images_to_data([big_form])[0], eng.images_to_data([funsd])[0]
        assert on.tiles == 4 and _items(on) == _items(off)
        want = _views_equal_host(on, big_form)
        assert len(want["marks"]) == 10 and want["marks"][:, 10].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 0, 0]
        assert f_on.tiles >= 1 and f_on.tiles == f_off.tiles and len(f_on) >= 8 and _items(f_on) == _items(f_off)   # the FUNSD page at its own scale: no mark, as on the host
        assert len(_views_equal_host(f_on, funsd)["marks"]) == 0
    finally:
        eng.set_tiled(0)


def test_tables_and_marks_together(eng):
    """both layers on: each one's views are what it gives alone, and the batch's ink pass is launched once - or twice when the two layers' `ink` differ"""
    from tests import deskew_ref as D
    page = D.form_page(words=True)
    _boxes_over(page, [(70, 112), (250, 152), (20, 20)], t=2, ticked=(0,))
    eng.set_tables((48, 128))
    try:
        tab = eng.images_to_data([page])[0]
    finally:
        eng.set_tables(False)
    with marks_on(eng):
        n0 = eng.page_ink_passes()
        mk = eng.images_to_data([page])[0]
        assert eng.page_ink_passes() == n0 + 1
        eng.set_tables((48, 128))
        try:
            n0 = eng.page_ink_passes()
            both = eng.images_to_data([page])[0]
            assert eng.page_ink_passes() == n0 + 1                                    # one pass, two readers
            eng.set_tables((48, 200))
            n0 = eng.page_ink_passes()
            other = eng.images_to_data([page])[0]
            assert eng.page_ink_passes() == n0 + 2                                    # another threshold: the marks keep their own
        finally:
            eng.set_tables(False)
    assert len(mk.mark_recs) == 3 and len(tab.table_rects) == 1 and len(mk) >= 20
    for r in (both, other):
        assert _items(r) == _items(mk) and np.array_equal(r.mark_recs, mk.mark_recs) and np.array_equal(r.item_mark, mk.item_mark)
    for k in ("rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell"):
        assert np.array_equal(getattr(both, k), getattr(tab, k)), k
    _views_equal_host(both, page)


def test_local_ink_on_a_shaded_form_equals_the_fixed_rule_on_the_clean_one(eng, form_synth):
    from tests import ink_ref as R
    from tuatara_amd import engine as E
    shaded = R.shade(form_synth, 0.35)
    ink = (R.RADIUS, R.DROP, R.DARK)
    with marks_on(eng):
        clean = eng.images_to_data([form_synth])[0]
        eng.set_local_ink(ink)
        try:
            on = eng.images_to_data([shaded])[0]
        finally:
            eng.set_local_ink(False)
    _views_equal_host(on, shaded, host=lambda p, q: E.marks_from_page_ink(p, q, *ARG[:3], local_ink=ink))
    assert np.array_equal(on.mark_recs[:, :4], clean.mark_recs[:, :4]) and np.array_equal(on.mark_recs[:, 10], clean.mark_recs[:, 10])
    assert on.ink == E.ink_from_page(shaded, *ink)["ink"]


def test_deskew_reads_the_upright_page(eng):
    """a tilted form: the marks are the layer-off engine's host rule on the upright page the deskew rule forms, and in its frame"""
    from tests import deskew_ref as D
    page = D.form_page(words=True)
    _boxes_over(page, [(70, 112), (250, 152), (600, 30), (20, 20)], t=3, ticked=(1,))
    tilted = D.tilt(page, 18)
    ref = D.deskew_ref(tilted)
    assert ref["skew"]["slope"] == 18
    off = eng.images_to_data([ref["image"]], conf=True)[0]
    eng.set_deskew(True)
    try:
        with marks_on(eng):
            on = eng.images_to_data([tilted], conf=True)[0]
    finally:
        eng.set_deskew(False)
    assert on.skew == ref["skew"] and _items(on) == _items(off)
    want = _views_equal_host(on, ref["image"])
    assert len(want["marks"]) == 4 and want["marks"][:, 10].sum() == 1
    back = on.to_page(np.asarray(on.mark_recs[:, :2], np.float32))
    assert back.shape == (4, 2) and np.abs(back - D.tilt_points(np.asarray([(70, 112), (250, 152), (600, 30), (20, 20)], np.float64)[[3, 2, 0, 1]], 18, 480, 1000)).max() < 2.0


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals(eng, form_synth):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    for bad in ((7, 64, 24, 128), (65, 128, 24, 128), (10, 9, 24, 128), (10, 129, 24, 128), (10, 64, 0, 128), (10, 64, 256, 128), (10, 64, 24, 0), (10, 64, 24, 256)):
        with pytest.raises(EngineError, match="ttr_engine_set_marks: min_side must be 0 .off., or min_side must lie in 8..64"):
            eng.set_marks(bad)
        assert eng.marks is None
        with pytest.raises(EngineError, match="min_side must lie in 8..64"):
            eng.marks_page(form_synth, None, *bad)
    q = np.asarray([M.quad_box(1, 1, 9, 9)] * 3, np.float32)
    q[2, 5] = -40000.0
    with pytest.raises(EngineError, match="quad 2 has a coordinate"):
        eng.marks_page(M.hand_page(), q)
    with marks_on(eng):                                                               # region calls leave the views empty
        out = eng.read_regions(form_synth, [{"rect": (20, 24, 160, 60)}])
        assert len(out) == 1 and "mark" not in out[0]
    buf = DeviceBuffer(form_synth.nbytes)
    buf.upload(form_synth)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            with pytest.raises(EngineError, match="ttr_engine_set_marks: selection marks are found by one engine alone, and a communicator is attached"):
                eng.set_marks(True)
            assert eng.marks is None
        finally:
            comm.attach(False)
        with marks_on(eng):
            with pytest.raises(EngineError, match="ttr_engine_attach_comm: selection marks are found by one engine alone"):
                comm.attach(True)
            with pytest.raises(EngineError, match="latency mode does not support selection marks"):
                comm.pages_to_data_sharded(buf, 1, 512, 640)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- 4. callers
def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, form_synth, monkeypatch, tmp_path):
    import os
    import subprocess
    import sys
    from PIL import Image
    from tuatara_amd import build as B
    from tuatara_amd import engine as E
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(B.ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    with marks_on(eng_x4):                                                            # the callers' engine: plain crops
        want = eng_x4.images_to_data([form_synth])[0]
        want_bgr = eng_x4.images_to_data([np.ascontiguousarray(form_synth[:, :, ::-1])])[0]   # (the CLI feeds BGR)
    assert len(want.mark_recs) == 6
    off = pytuatara.image_to_data(form_synth, weights["dir"], "o")
    assert pytuatara.last_call_marks() == []
    on = pytuatara.image_to_data(form_synth, weights["dir"], "o", marks=True)
    got = pytuatara.last_call_marks()
    assert "mark" not in off[0] and [d["text"] for d in on] == [d["text"] for d in off] == list(want.texts)
    assert [d["mark"] for d in on] == want.item_mark.tolist()
    assert [list(m["box"]) for m in got] == want.mark_recs[:, :4].tolist() and [m["selected"] for m in got] == [bool(v) for v in want.mark_recs[:, 10]]
    assert [m["label"] for m in got] == want.mark_recs[:, 11].tolist() and [m["text"] for m in got] == [m["text"] for m in want.marks]
    assert [d["mark"] for d in pytuatara.image_to_data(form_synth, weights["dir"], "o", marks=(10, 64, 24, 128))] == want.item_mark.tolist()
    assert "mark" not in pytuatara.image_to_data(form_synth, weights["dir"], "o")[0]         # the call's setting is gone afterwards
    monkeypatch.setenv("TUATARA_MARKS", "1")                                                 # the C++ switch
    pytuatara.image_to_data(form_synth, weights["dir"], "o")
    assert [list(m["box"]) for m in pytuatara.last_call_marks()] == want.mark_recs[:, :4].tolist()
    monkeypatch.delenv("TUATARA_MARKS")
    with pytest.raises(RuntimeError, match="min_side in 8..64"):
        pytuatara.image_to_data(form_synth, weights["dir"], "o", marks=(7, 64, 24, 128))
    with pytest.raises(ValueError, match="regions"):
        pytuatara.image_to_data(form_synth, weights["dir"], "o", marks=True, regions=[{"rect": (5, 5, 200, 25)}])
    png = str(tmp_path / "page.png")
    Image.fromarray(form_synth).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--marks", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.split("\n") if ln]
    assert lines == [("[x] " if m["selected"] else "[ ] ") + " ".join(str(v) for v in m["box"]) + "\t" + m["text"] for m in want_bgr.marks]
    assert sum(ln.startswith("[x]") for ln in lines) == 1 and len(lines) == 6
    bad = subprocess.run([cli, "--marks", "7", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode == 1 and "8..64" in bad.stderr
    assert E.marks_from_page(form_synth)["marks"][:, :4].tolist() == want.mark_recs[:, :4].tolist()
