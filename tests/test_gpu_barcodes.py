"""GPU suite for barcodes (DESIGN.md "Barcodes"; tuatara_amd/csrc/barcodes.hip): barcode_scan_kernel and barcode_page_kernel through the stage call against
the host rule bit for bit on the pages of tests/barcodes_ref.py (every word-boundary offset, the page's edges, all four directions, 1-px modules, 8 and 9
codes on a line, 64 and 65 on a page, a 1300 x 1100 page of many bands); the hook's raw hits against the restatement; windows that are not dword-aligned;
page calls on the FUNSD page and on a synthetic page with drawn codes through the list, device, mixed-size, streamed and tiled entry points - items identical
to barcodes off, views equal to the host rule on the returned quads; batches asserted to hold no word; tables, marks and barcodes together on one ink pass;
local ink on a shaded label; deskew on a tilted label; the stage call after a poisoned scratch; the views with the layer off; every refusal.  Every test
here fails on the parent commit: Engine.set_barcodes / Engine.barcodes_page and their symbols are absent."""
import numpy as np
import pytest

from tests import barcodes_ref as R

pytestmark = pytest.mark.gpu

ARG = (8, 128, 3)


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads) that batches mixed sizes; barcodes OFF at rest: every test that turns them on turns them off again"""
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


class barcodes_on:
    def __init__(self, eng, arg=True):
        self.eng, self.arg = eng, arg

    def __enter__(self):
        self.eng.set_barcodes(self.arg)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_barcodes(False)


# (data, symbology, module, x, y, height, direction): cleared to white with a margin, then drawn, so the codes read whatever the page held there
CODES = [(b"INV-2024-0042", 1, 1, 20, 12, 24, 0), (b"TRACK 42", 2, 1, 300, 60, 20, 2), (b"0012345678", 1, 2, 20, 440, 30, 0), ("UP", 2, 2, 600, 150, 18, 3)]


def _codes_over(page, codes=CODES):
    for data, sym, module, x, y, height, d in codes:
        widths = R.text128(data) if sym == 1 else R.code39_symbols(data.decode() if isinstance(data, bytes) else data)
        n = sum(widths) * module
        if d in (0, 2):
            page[max(y - 4, 0):y + height + 4, max(x - 14, 0):x + n + 14] = 255
        else:
            page[max(y - 14, 0):y + n + 14, max(x - 4, 0):x + height + 4] = 255
        R.draw(page, widths, module, x, y, height, d)
    return page


def _data(codes=CODES):
    return sorted(d if isinstance(d, bytes) else d.encode() for d, *_ in codes)


@pytest.fixture(scope="module")
def label_synth():
    """a synthetic page of words with four drawn codes, one in each direction"""
    from tuatara_amd import synth
    return _codes_over(synth.synthetic_page(3, 512, 640, n_words=24))


@pytest.fixture(scope="module")
def big_label():
    from tuatara_amd import synth
    return _codes_over(synth.synthetic_page(7, 1300, 1100, n_words=60), [(b"BIG-PAGE-1", 1, 3, 40, 40, 40, 0), (b"987654", 1, 2, 700, 900, 30, 2),
                                                                           ("COL", 2, 2, 1000, 300, 30, 1)])


def _same(got, want, what=""):
    assert got["mode"] == want["mode"] and got["counts"] == want["counts"], (what, got["mode"], want["mode"], got["counts"], want["counts"])
    assert got["records"].shape == want["records"].shape and np.array_equal(got["records"], want["records"]), (what, got["records"][:, :12], want["records"][:, :12])
    assert np.array_equal(got["item_barcode"], want["item_barcode"]), what


def _shared_pages():
    pages = {"mixed": R.mixed_page()[:2], "edges": (R.edges_page(), None), "eight": (R.many_codes_page(8), None), "nine": (R.many_codes_page(9, per_row=9), None),
             "cap64": (R.many_codes_page(64), np.asarray([R.quad_box(10, 3, 20, 6)], np.float32)),
             "cap65": (R.many_codes_page(65), np.asarray([R.quad_box(10, 3, 20, 6)], np.float32))}
    for x0, x1 in R.OFFSET_RANGES:
        page = R.offsets_page(x0, x1)
        pages[f"offsets {x0}"] = (page, None)
        pages[f"offsets {x0} mirrored"] = (np.ascontiguousarray(page[:, ::-1]), None)
        pages[f"offsets {x0} transposed"] = (np.ascontiguousarray(page.transpose(1, 0, 2)), None)
        pages[f"offsets {x0} upwards"] = (np.ascontiguousarray(page.transpose(1, 0, 2)[::-1]), None)
    for s in range(4):
        pages[f"random {s}"] = R.random_page(s)
    for w in (1, 46, 63, 64, 65, 129):
        img = R.blank(20, w)
        img[np.random.RandomState(w).rand(20, w) < 0.3] = 0
        if w >= 46:
            R.draw(img, R.text128(b"w"), 1, w - 46, 4, 6)
        pages[f"width {w}"] = (img, None)
        pages[f"height {w}"] = (np.ascontiguousarray(img.transpose(1, 0, 2)), None)
    return pages


# ------------------------------------------------------------------------------------------------- 1. the kernels against the host rule
def test_stage_call_equals_the_host_rule(eng):
    from tuatara_amd import engine as E
    modes, found, dirs = set(), 0, set()
    for name, (img, quads) in _shared_pages().items():
        want, got = E.barcodes_from_page(img, quads, 4, 128, 3), eng.barcodes_page(img, quads, 4, 128, 3)
        _same(got, want, name)
        modes.add(got["mode"])
        found += len(got["barcodes"])
        dirs |= {b["direction"] for b in got["barcodes"]}
    assert modes == {1, -7} and found >= 4 * 131 + 64 + 16 and dirs == {0, 1, 2, 3}
    img, quads, boxes = R.mixed_page()
    r = eng.barcodes_page(img, quads)
    assert [b["box"] for b in r["barcodes"]] == [list(b) for b in boxes] and r["item_barcode"].tolist() == [0, 1, -1, 2, 3, 4, -1]
    _same(eng.barcodes_page(img, quads, 8, 128, 1), E.barcodes_from_page(img, quads, 8, 128, 1), "Code 128 alone")
    _same(eng.barcodes_page(img, quads, 8, 128, 2), E.barcodes_from_page(img, quads, 8, 128, 2), "Code 39 alone")


def _hits_equal(d, want, h, w, what=""):
    """the hook's raw hits and counters against the restatement's, line by line"""
    for kind, count, base in ((0, h, 0), (1, w, h)):
        for k in range(count):
            for rev in (0, 1):
                hs = want["hits"][(kind, k, rev)]
                assert d["line_counts"][base + k, rev, 0] == len(hs), (what, kind, k, rev)
                for s, (sym, p0, p1, text, flags, mod) in enumerate(hs):
                    r = d["hits"][base + k, rev, s]
                    assert r[:6].tolist() == [p0, p1, mod, flags, len(text), sym] and r[8:].tobytes() == text.ljust(48, b"\0"), (what, kind, k, rev, s)
    c = d["line_counts"].reshape(-1, 4).sum(axis=0).tolist()
    assert [c[2], c[3], c[0], c[1]] == want["counts"][1:5] == d["side"][2:6].tolist(), what


def test_a_page_of_many_bands_and_the_hooks_hits(eng):
    """1300 x 1100: 75 bands of lines; the hook's raw hits are the restatement's, and so are the host rule's"""
    from tuatara_amd import engine as E
    img = R.many_bands_page()
    want = R.barcodes_of_page(img)
    _same(eng.barcodes_page(img), E.barcodes_from_page(img))
    _same(eng.barcodes_page(img), want)
    assert sorted(b["data"] for b in want["barcodes"]) == sorted([b"BAND-0001-xyz", b"998877665544", b"TRACK-42", b"Z9", b"corner"])
    d = eng.barcodes_debug(img)
    _hits_equal(d, want, 1100, 1300)
    host = E.barcodes_from_page(img, raw=True)
    assert np.array_equal(d["line_counts"], host["line_counts"]) and np.array_equal(d["hits"], host["hits"])   # chain fields included
    for name in ("mixed", "nine", "cap65", "edges"):
        img = _shared_pages()[name][0]
        _hits_equal(eng.barcodes_debug(img, 4), R.barcodes_of_page(img, None, 4), *img.shape[:2], what=name)


@pytest.mark.parametrize("width", [512, 1024, 1536])
def test_decodes_that_fail_after_their_text_began(eng, width):
    """a cut-off Code 39 and an over-long Code 128 between two valid codes on one line, where a lane owns 1, 2 and 3 words, in all four directions: a failed
    decode leaves no byte in a slot - the next lane's hit keeps its text, and the hook's slots are zero beyond a line's count, as the host's are"""
    from tuatara_amd import engine as E
    page = R.partial_page(width)
    for img, d in ((page, 0), (page[:, ::-1], 2), (page.transpose(1, 0, 2), 1), (page.transpose(1, 0, 2)[::-1], 3)):
        img = np.ascontiguousarray(img)
        want, ref = E.barcodes_from_page(img, None, 4, raw=True), R.barcodes_of_page(img, None, 4)
        _same(want, ref, (width, d))
        got = eng.barcodes_page(img, None, 4)
        _same(got, want, (width, d))
        assert sorted((b["direction"], b["data"]) for b in got["barcodes"]) == [(d, b"A"), (d, b"A"), (d, b"B"), (d, b"B")]
        hook = eng.barcodes_debug(img, 4)
        _hits_equal(hook, ref, *img.shape[:2], what=(width, d))
        assert np.array_equal(hook["line_counts"], want["line_counts"]) and np.array_equal(hook["hits"], want["hits"])


def test_funsd_through_the_hook(eng, funsd):
    """the figures DESIGN.md states: 60288 candidates, 109 start patterns, no hit"""
    d = eng.barcodes_debug(funsd)
    assert d["side"][:8].tolist() == [1, 0, 60288, 109, 0, 0, 0, 0]


@pytest.mark.parametrize("offset,pad", [(3, 5), (1, 0), (4, 2), (2, 4)])
def test_a_window_that_is_not_dword_aligned(eng, offset, pad):
    from tuatara_amd import engine as E
    for img in (R.mixed_page()[0], R.random_page(4)[0], R.edges_page()):
        w = img.shape[1]
        want, got = E.barcodes_from_page(img, raw=True), eng.barcodes_debug(img, dev_offset=offset, dev_stride=3 * w + pad)
        assert np.array_equal(got["hits"], want["hits"]) and np.array_equal(got["line_counts"], want["line_counts"])
        assert got["side"][1] == len(want["records"]) and np.array_equal(got["side"][8:8 + 24 * len(want["records"])].reshape(-1, 24), want["records"])


def test_the_stage_call_whatever_the_engine_ran_before(eng, fresh):
    """after every fill of the poison hook, and after a larger page, the stage call's bytes are a fresh engine's"""
    small, quads = R.random_page(5)
    big = R.many_bands_page()
    want = fresh.barcodes_page(small, quads, 4)
    _same(want, R.barcodes_of_page(small, quads, 4))
    for pattern in (0, 1, 2):
        eng.barcodes_page(big)
        eng.poison_scratch(pattern)
        _same(eng.barcodes_page(small, quads, 4), want, pattern)
    eng.barcodes_page(R.many_codes_page(65), None, 4)                                    # a page beyond the cap before the small one, nothing in between
    _same(eng.barcodes_page(small, quads, 4), want)


# ------------------------------------------------------------------------------------------------- 2. page calls
def _items(res):
    return (list(res.texts), res.ids.tolist(), res.conf.tolist(), res.bbox.tolist(), res.quad.tolist())


def _views_equal_host(res, page, arg=ARG, host=None):
    from tuatara_amd import engine as E
    want = host(page, res.quad) if host else E.barcodes_from_page(page, res.quad if len(res) else None, *arg)
    assert res.barcode_mode == want["mode"]
    assert res.barcode_recs.shape == want["records"].shape and np.array_equal(res.barcode_recs, want["records"])
    assert res.item_barcode.shape == want["item_barcode"].shape and np.array_equal(res.item_barcode, want["item_barcode"])
    return want


def test_end_to_end(eng, funsd, label_synth):
    for name, page in (("funsd", funsd), ("synthetic label", label_synth)):
        off = eng.images_to_data([page], conf=True)[0]
        assert off.barcode_recs is None and off.item_barcode is None and off.barcodes == [] and off.barcode_mode == 0 and "barcode" not in off[0]
        with barcodes_on(eng):
            assert eng.barcodes == ARG
            on = eng.images_to_data([page], conf=True)[0]
        assert eng.barcodes is None
        assert len(on) >= 8 and _items(on) == _items(off), name                      # text, ids, conf, boxes, quads: every bit
        want = _views_equal_host(on, page)
        assert "barcode" in on[0] and len(on.barcodes) == len(want["records"])
        if name == "funsd":
            assert on.barcodes == []
        else:
            assert sorted(b["data"] for b in on.barcodes) == _data()
            assert sorted(b["direction"] for b in on.barcodes) == [0, 0, 2, 3] and {b["symbology"] for b in on.barcodes} == {"code128", "code39"}
            b = [b for b in on.barcodes if b["data"] == b"INV-2024-0042"][0]
            assert b["box"][:2] == [20, 12] and b["box"][3] == 35 and b["lines"] == 24 and b["module"] == 1.0 and not b["gs1"] and b["text"] == "INV-2024-0042"
        assert eng.images_to_data([page], conf=True)[0].barcode_recs is None          # off again


class wordless:
    """Batches without a single word: the engine's own knob `detector_only` drops the detector's boxes before anything goes to the recogniser, which leaves
    exactly the batch an empty detection leaves: N = 0, no packer, no upload, no recogniser pass."""
    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        assert self.eng.set_tuning("detector_only", 1) == 0
        return self.eng

    def __exit__(self, *a):
        assert self.eng.set_tuning("detector_only", 0) == 0


def _wordless_views(res, page, arg=ARG, host=None):
    assert len(res) == 0 and res.item_barcode.shape == (0,)
    return _views_equal_host(res, page, arg, host)


def test_a_label_and_no_text(eng, label_synth):
    """the layer runs for a batch without words - a label is a legitimate page - through the list, mixed-size, device and streamed entry points, behind a batch
    with words in the same slot, with marks on beside it, and under local ink; every call here asserts that its batch held no word"""
    from tests import ink_ref as I
    from tuatara_amd import engine as E
    from tuatara_amd.engine import DeviceBuffer
    page = _codes_over(R.blank(256, 256), [(b"LBL-1", 1, 1, 20, 20, 16, 0), ("Q7", 2, 1, 200, 60, 12, 1)])
    small = _codes_over(R.blank(250, 240), [(b"77", 1, 2, 30, 100, 10, 2)])             # (shares the 256 x 256 canvas: one mixed batch with `page`)
    blank = R.blank(256, 256)
    with wordless(eng):
        off = eng.images_to_data([page])[0]
        assert len(off) == 0 and off.barcode_recs is None and off.item_barcode is None and off.barcode_mode == 0
    with barcodes_on(eng):
        wordy = eng.images_to_data([label_synth])[0]                                  # a batch with words first: its side block and its items' barcodes lie in the slot
        assert len(wordy) >= 8 and len(wordy.barcode_recs) == 4
        with wordless(eng):
            res = eng.images_to_data([page])[0]
            want = _wordless_views(res, page)
            assert sorted(b["data"] for b in res.barcodes) == [b"LBL-1", b"Q7"] and len(want["records"]) == 2
            two = eng.images_to_data([page, blank])                                   # a uniform batch of two
            assert sum(len(r) for r in two) == 0
            _wordless_views(two[0], page)
            assert len(_wordless_views(two[1], blank)["records"]) == 0
            mixed = eng.images_to_data([page, small, label_synth])                    # sizes of their own: the page table, and a page whose words are dropped
            assert sum(len(r) for r in mixed) == 0
            _wordless_views(mixed[0], page)
            assert len(_wordless_views(mixed[1], small)["records"]) == 1
            assert len(_wordless_views(mixed[2], label_synth)["records"]) == 4
            eng.set_marks(True)                                                       # marks beside barcodes: one upload of the offsets, one ink pass
            try:
                n0 = eng.page_ink_passes()
                both = eng.images_to_data([page])[0]
                assert eng.page_ink_passes() == n0 + 1 and both.mark_mode == 1
                _wordless_views(both, page)
            finally:
                eng.set_marks(False)
            same = np.stack([page, blank, page])
            ub = DeviceBuffer(same.nbytes)
            ub.upload(same)
            try:
                dev = eng.pages_to_data_dev(ub, 3, 256, 256)
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
            ink = (I.RADIUS, I.DROP, I.DARK)
            shaded = I.shade(page, 0.35)
            eng.set_local_ink(ink)
            try:
                li = eng.images_to_data([shaded])[0]
            finally:
                eng.set_local_ink(False)
            got = _wordless_views(li, shaded, host=lambda p, q: E.barcodes_from_page_ink(p, None, ARG[0], ARG[2], local_ink=ink))
            assert got["records"][:, :6].tolist() == want["records"][:, :6].tolist() and li.ink == E.ink_from_page(shaded, *ink)["ink"]
        again = eng.images_to_data([label_synth])[0]                                  # and words again behind the wordless batches
        assert _items(again) == _items(wordy) and np.array_equal(again.barcode_recs, wordy.barcode_recs) and np.array_equal(again.item_barcode, wordy.item_barcode)


def test_mixed_sizes_device_pages_and_streams(eng, funsd, label_synth):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    small = np.ascontiguousarray(label_synth[:500, :630])
    pages = [funsd, label_synth, small]
    bufs, rows = [], []
    lst_off = eng.images_to_data(pages)                                               # every call's items with barcodes off: what barcodes on must leave bit for bit
    with barcodes_on(eng):
        lst = eng.images_to_data(pages)
        for p, s, g in zip(pages, lst_off, lst):
            assert _items(g) == _items(s)
            _views_equal_host(g, p)
        for k, p in enumerate([label_synth, small]):                                  # one canvas, two sizes; page 1 with an odd row stride
            h, w = p.shape[:2]
            stride = w * 3 + (7 if k == 1 else 0)
            host = np.full((h, stride), 0xAB, np.uint8)
            host[:, :w * 3] = np.ascontiguousarray(p).reshape(h, w * 3)
            b = DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
            rows.append((b, h, w, stride if k == 1 else 0))
        same = np.stack([label_synth] * 2)
        ub = DeviceBuffer(same.nbytes)
        ub.upload(same)
        bufs.append(ub)
        eng.set_barcodes(False)
        got_off, uni_off = eng.pages_to_data_dev_v(rows), eng.pages_to_data_dev(ub, 2, 512, 640)
        eng.set_barcodes(True)
        got = eng.pages_to_data_dev_v(rows)
        assert [_items(g) for g in got] == [_items(g) for g in got_off]
        assert len(_views_equal_host(got[0], label_synth)["records"]) == 4
        assert len(_views_equal_host(got[1], small)["records"]) >= 3
        uni = eng.pages_to_data_dev(ub, 2, 512, 640)
        for g, o in zip(uni, uni_off):
            assert _items(g) == _items(o)
            _views_equal_host(g, label_synth)
        streamed = []
        for push in (lambda: eng.stream_push_v(rows), lambda: eng.stream_push(ub, 2, 512, 640), lambda: eng.stream_push_v(rows[::-1])):
            r = push()
            if r:
                streamed.append(r)
        with pytest.raises(EngineError, match="streamed batches are in flight"):     # the setter and the stage call refuse while batches stream
            eng.set_barcodes(False)
        with pytest.raises(EngineError, match="streamed batches are in flight"):
            eng.barcodes_page(label_synth)
        while True:
            r = eng.stream_flush()
            if not r:
                break
            streamed.append(r)
        assert len(streamed) == 3
        for a, b in zip(streamed, [got, uni, got[::-1]]):
            for x, y in zip(a, b):
                assert _items(x) == _items(y) and x.barcode_mode == y.barcode_mode
                assert np.array_equal(x.barcode_recs, y.barcode_recs) and np.array_equal(x.item_barcode, y.item_barcode)
    for b in bufs:
        b.free()


def test_tiled_pages_read_the_page_at_its_own_scale(eng, big_label):
    eng.set_tiled(128)
    try:
        off = eng.images_to_data([big_label])[0]
        with barcodes_on(eng):
            on = eng.images_to_data([big_label])[0]
        assert on.tiles == 4 and _items(on) == _items(off)
        want = _views_equal_host(on, big_label)
        assert sorted(b["data"] for b in on.barcodes) == [b"987654", b"BIG-PAGE-1", b"COL"] and len(want["records"]) == 3
    finally:
        eng.set_tiled(0)


def test_tables_marks_and_barcodes_together(eng):
    """all three layers on: each one's views are what it gives alone, and the batch's ink pass is launched once - or twice when barcodes' `ink` differs"""
    from tests import deskew_ref as D
    from tests import marks_ref as M
    page = D.form_page(words=True)
    M.frame(page, 70, 112, 16, 2)
    _codes_over(page, [(b"FORM-9", 1, 1, 250, 150, 14, 0)])
    eng.set_tables((48, 128))
    try:
        tab = eng.images_to_data([page])[0]
    finally:
        eng.set_tables(False)
    eng.set_marks(True)
    try:
        mk = eng.images_to_data([page])[0]
    finally:
        eng.set_marks(False)
    with barcodes_on(eng):
        n0 = eng.page_ink_passes()
        bc = eng.images_to_data([page])[0]
        assert eng.page_ink_passes() == n0 + 1
        eng.set_tables((48, 128))
        eng.set_marks(True)
        try:
            n0 = eng.page_ink_passes()
            three = eng.images_to_data([page])[0]
            assert eng.page_ink_passes() == n0 + 1                                    # one pass, three readers
            eng.set_barcodes((8, 200, 3))
            n0 = eng.page_ink_passes()
            other = eng.images_to_data([page])[0]
            assert eng.page_ink_passes() == n0 + 2                                    # another threshold: barcodes form their own
            eng.set_marks(False)
            eng.set_barcodes(True)
            n0 = eng.page_ink_passes()
            two = eng.images_to_data([page])[0]
            assert eng.page_ink_passes() == n0 + 1                                    # tables and barcodes
        finally:
            eng.set_tables(False)
            eng.set_marks(False)
    assert [b["data"] for b in bc.barcodes] == [b"FORM-9"] and len(tab.table_rects) == 1 and len(mk.mark_recs) >= 1 and len(bc) >= 20
    for r in (three, two):
        assert _items(r) == _items(bc) and np.array_equal(r.barcode_recs, bc.barcode_recs) and np.array_equal(r.item_barcode, bc.item_barcode)
        for k in ("rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell"):
            assert np.array_equal(getattr(r, k), getattr(tab, k)), k
    assert np.array_equal(three.mark_recs, mk.mark_recs) and np.array_equal(other.mark_recs, mk.mark_recs)
    _views_equal_host(three, page)
    _views_equal_host(other, page, (8, 200, 3))


def test_local_ink_on_a_shaded_label_equals_the_fixed_rule_on_the_clean_one(eng, label_synth):
    from tests import ink_ref as I
    from tuatara_amd import engine as E
    shaded = I.shade(label_synth, 0.35)
    ink = (I.RADIUS, I.DROP, I.DARK)
    with barcodes_on(eng):
        clean = eng.images_to_data([label_synth])[0]
        eng.set_local_ink(ink)
        try:
            on = eng.images_to_data([shaded])[0]
        finally:
            eng.set_local_ink(False)
    _views_equal_host(on, shaded, host=lambda p, q: E.barcodes_from_page_ink(p, q, ARG[0], ARG[2], local_ink=ink))
    assert sorted(b["data"] for b in on.barcodes) == sorted(b["data"] for b in clean.barcodes) == _data()
    assert on.ink == E.ink_from_page(shaded, *ink)["ink"]


def test_deskew_reads_the_upright_page(eng):
    """a tilted label: the barcodes are the layer-off engine's host rule on the upright page the deskew rule forms, in its frame, and to_page leads back"""
    from tests import deskew_ref as D
    page = D.form_page(words=True)
    _codes_over(page, [(b"TILT-18", 1, 3, 250, 150, 40, 0)])
    tilted = D.tilt(page, 18)
    ref = D.deskew_ref(tilted)
    assert ref["skew"]["slope"] == 18
    off = eng.images_to_data([ref["image"]], conf=True)[0]
    eng.set_deskew(True)
    try:
        with barcodes_on(eng):
            on = eng.images_to_data([tilted], conf=True)[0]
    finally:
        eng.set_deskew(False)
    assert on.skew == ref["skew"] and _items(on) == _items(off)
    want = _views_equal_host(on, ref["image"])
    assert [b["data"] for b in on.barcodes] == [b"TILT-18"] and len(want["records"]) == 1
    back = on.to_page(np.asarray(on.barcode_recs[:, :2], np.float32))
    assert back.shape == (1, 2) and np.abs(back - D.tilt_points(np.asarray([(250, 150)], np.float64), 18, 480, 1000)).max() < 3.0


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals(eng, label_synth):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    for bad in ((3, 128, 3), (257, 128, 3), (8, 0, 3), (8, 256, 3), (8, 128, 0), (8, 128, 4)):
        with pytest.raises(EngineError, match="ttr_engine_set_barcodes: min_lines must be 0 .off., or min_lines must lie in 4..256"):
            eng.set_barcodes(bad)
        assert eng.barcodes is None
        with pytest.raises(EngineError, match="min_lines must lie in 4..256"):
            eng.barcodes_page(label_synth, None, *bad)
    q = np.asarray([R.quad_box(1, 1, 9, 9)] * 3, np.float32)
    q[2, 5] = -40000.0
    with pytest.raises(EngineError, match="quad 2 has a coordinate"):
        eng.barcodes_page(R.edges_page(), q)
    with barcodes_on(eng):                                                            # region calls leave the views empty
        out = eng.read_regions(label_synth, [{"rect": (20, 80, 160, 120)}])
        assert len(out) == 1 and "barcode" not in out[0]
    buf = DeviceBuffer(label_synth.nbytes)
    buf.upload(label_synth)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            with pytest.raises(EngineError, match="ttr_engine_set_barcodes: barcodes are read by one engine alone, and a communicator is attached"):
                eng.set_barcodes(True)
            assert eng.barcodes is None
        finally:
            comm.attach(False)
        with barcodes_on(eng):
            with pytest.raises(EngineError, match="ttr_engine_attach_comm: barcodes are read by one engine alone"):
                comm.attach(True)
            with pytest.raises(EngineError, match="latency mode does not support barcodes"):
                comm.pages_to_data_sharded(buf, 1, 512, 640)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- 4. callers
def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, label_synth, monkeypatch, tmp_path):
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
    with barcodes_on(eng_x4):                                                         # the callers' engine: plain crops
        want = eng_x4.images_to_data([label_synth])[0]
        want_bgr = eng_x4.images_to_data([np.ascontiguousarray(label_synth[:, :, ::-1])])[0]   # (the CLI feeds BGR)
    assert len(want.barcode_recs) == 4
    off = pytuatara.image_to_data(label_synth, weights["dir"], "o")
    assert pytuatara.last_call_barcodes() == []
    on = pytuatara.image_to_data(label_synth, weights["dir"], "o", barcodes=True)
    got = pytuatara.last_call_barcodes()
    assert "barcode" not in off[0] and [d["text"] for d in on] == [d["text"] for d in off] == list(want.texts)
    assert [d["barcode"] for d in on] == want.item_barcode.tolist()
    assert [list(b["box"]) for b in got] == want.barcode_recs[:, :4].tolist()
    for k in ("symbology", "direction", "text", "data", "lines", "module", "gs1"):
        assert [b[k] for b in got] == [b[k] for b in want.barcodes], k
    assert [d["barcode"] for d in pytuatara.image_to_data(label_synth, weights["dir"], "o", barcodes=(8, 128, 3))] == want.item_barcode.tolist()
    assert [b["symbology"] for b in (pytuatara.image_to_data(label_synth, weights["dir"], "o", barcodes=(8, 128, 2)), pytuatara.last_call_barcodes())[1]] == ["code39"] * 2
    assert "barcode" not in pytuatara.image_to_data(label_synth, weights["dir"], "o")[0]   # the call's setting is gone afterwards
    monkeypatch.setenv("TUATARA_BARCODES", "1")                                             # the C++ switch
    pytuatara.image_to_data(label_synth, weights["dir"], "o")
    assert [list(b["box"]) for b in pytuatara.last_call_barcodes()] == want.barcode_recs[:, :4].tolist()
    monkeypatch.delenv("TUATARA_BARCODES")
    with pytest.raises(RuntimeError, match="min_lines in 4..256"):
        pytuatara.image_to_data(label_synth, weights["dir"], "o", barcodes=(3, 128, 3))
    with pytest.raises(ValueError, match="regions"):
        pytuatara.image_to_data(label_synth, weights["dir"], "o", barcodes=True, regions=[{"rect": (5, 5, 200, 25)}])
    png = str(tmp_path / "page.png")
    Image.fromarray(label_synth).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--barcodes", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.split("\n") if ln]
    assert lines == [f"{b['symbology']} {b['direction']} " + " ".join(str(v) for v in b["box"]) + "\t" + b["text"] for b in want_bgr.barcodes]
    assert len(lines) == 4 and sum(ln.startswith("code39") for ln in lines) == 2
    bad = subprocess.run([cli, "--barcodes", "3", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode == 1 and "4..256" in bad.stderr
    assert E.barcodes_from_page(label_synth)["records"][:, :4].tolist() == want.barcode_recs[:, :4].tolist()
