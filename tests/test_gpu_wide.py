"""GPU suite for wide words (DESIGN.md "Wide words"): wide_cut_kernel against the host rule, region and page calls against crops made in numpy from
tests/wide_ref.py's piece coefficients and read by the stage calls, the joins, wide on with no wide word against wide off, lines and blocks, the streamed and
list forms, every refusal, and the callers.  Every test here fails on the parent commit: Engine.set_wide / Engine.wide_cuts and their symbols are absent."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests import rectify_ref as RR
from tests import regions_ref as GR
from tests import wide_ref as WR
from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


@pytest.fixture(scope="module")
def engines(weights):
    """rectified engines by (precision, lines + blocks), made on demand and kept for the module"""
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    made = {}

    def get(precision="f16x4", layout=False):
        key = (precision, layout)
        if key not in made:
            kw = dict(lines=1, blocks=1) if layout else {}
            made[key] = Engine(weights["dir"], precision=precision, crop_mode=CROP_RECTIFIED, **kw)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def pages(funsd):
    from tuatara_amd import synth
    return [funsd, synth.synthetic_page(71, 640, 512, n_words=24)]


def _bars(seed, h, w):
    """a page of dark bars on a light ground with some noise: gaps for the cuts to find, and texture everywhere else"""
    rng = np.random.default_rng(seed)
    img = rng.integers(200, 256, (h, w, 3), dtype=np.uint8)
    x = 3
    while x < w - 4:
        bw = int(rng.integers(3, 15))
        img[:, x:x + bw] = rng.integers(0, 120, (h, min(bw, w - x), 3), dtype=np.uint8)
        x += bw + int(rng.integers(2, 7))
    img[rng.integers(0, h, 40), rng.integers(0, w, 40)] = 0
    return img


# ------------------------------------------------------------------------------------------------- 1. the kernel against the host rule
@pytest.mark.parametrize("table", [False, True])
def test_wide_cuts_equals_the_host_rule(engines, table):
    """40 quads in one launch on a 64 x 1400 page: n in {2, 3, 5, 16} (the single interior cut; the full LDS rows and eight columns per thread), tilts 0, 7 and
    -30 degrees, two quads partly outside; n, cuts, profiles and coefficient rows bit for bit against the host rule and the numpy reference, through the
    uniform and the page-table form."""
    from tuatara_amd import engine as E
    eng = engines()
    img = _bars(1, 64, 1400)
    rng = np.random.default_rng(2)
    aspect = 2.0
    quads, want_n = [], []
    for i in range(38):
        n = (2, 3, 5, 16)[i % 4]
        deg = (0.0, 7.0, -30.0)[i % 3]
        h = float(rng.uniform(6, 12))
        length = (n - 0.5) * aspect * h
        quads.append(WR.quad_of(float(rng.uniform(0, 1400 - length * 0.8)), float(rng.uniform(4, 50)), length, h, deg))
        want_n.append(n)
    quads.append(WR.quad_of(-90.0, 20.0, 2.5 * aspect * 14.0, 14.0, 0.0))      # partly outside, left
    quads.append(WR.quad_of(1330.0, 40.0, 4.5 * aspect * 10.0, 10.0, 7.0))     # partly outside, right and below
    want_n += [3, 5]
    quads = np.stack(quads)
    assert len(quads) == 40 and not GR.inside(quads[38], 64, 1400) and not GR.inside(quads[39], 64, 1400)
    n, cuts, prof, coef = eng.wide_cuts(img, quads, aspect, table=table)
    assert n.tolist() == want_n and set(want_n) == {2, 3, 5, 16}
    for i, q in enumerate(quads):
        hn, frame = E.wide_plan(q, aspect)
        hq = E.wide_profile(img, frame, hn)
        hc = E.wide_cuts_from_profile(hq, hn)
        rn, rframe, rq, rcuts, rcoef = WR.word(img, q, aspect)
        assert n[i] == hn == rn, i
        assert np.array_equal(prof[i, :128 * hn], hq) and np.array_equal(hq, rq) and not prof[i, 128 * hn:].any(), i
        assert np.array_equal(cuts[i], hc) and np.array_equal(hc, rcuts), (i, cuts[i], hc)
        rows = np.stack([E.wide_piece_coef(frame, hc[j], hc[j + 1]) for j in range(hn)])
        assert np.array_equal(coef[i, :hn], rows) and np.array_equal(rows, rcoef) and not coef[i, hn:].any(), i
    assert any(len(set(np.diff(c[:k + 1]).tolist())) > 1 for c, k in zip(cuts, n))      # the cuts moved off the even split somewhere


def test_wide_cuts_one_piece_is_the_frame(engines):
    """n = 1 through the kernel: the cuts are {0, 128} and the coefficient row is region_coef's, kind 1"""
    eng = engines()
    img = _bars(3, 40, 300)
    quad = WR.quad_of(10.0, 5.0, 120.0, 30.0, 4.0)
    n, cuts, prof, coef = eng.wide_cuts(img, quad[None], 8.0)
    assert n.tolist() == [1] and cuts[0, :2].tolist() == [0, 128] and (cuts[0, 2:] == -1).all()
    assert np.array_equal(coef[0, 0], np.concatenate([[1], GR.region_fixed(quad), [0]])) and not coef[0, 1:].any()
    assert np.array_equal(prof[0, :128], WR.profile(img, WR.plan(quad, 8.0)[1], 1))


# ------------------------------------------------------------------------------------------------- 2. a region call
def _reference_rows(eng, img, quads, aspect, set_of=None, masks=None, rows_of=None, n_rows=None):
    """what the engine must return for these quads: per quad (n, cuts, coef), and the recogniser's rows of every piece - crops from the kind-1 sampler on
    wide_ref's piece coefficients, read by Engine.parseq_logits + logits_confidence in the engine's two passes: the batch's n_rows rows (quad i's first piece at
    row rows_of[i]; rows of words that are not listed are blank crops: a row's reading does not depend on its neighbours, the kernels picked depend on the row
    count), then the other pieces in (item, piece) order.  Returns (plans, piece rows per quad: lists of (ids, prob, conf))."""
    plans = [WR.word(img, q, aspect) for q in quads]
    rows_of = list(range(len(quads))) if rows_of is None else [int(r) for r in rows_of]
    n_rows = len(quads) if n_rows is None else n_rows
    first = np.zeros((n_rows, 32, 128, 3), np.uint8)
    first_set = np.full(n_rows, -1, np.int32)
    for i, r in enumerate(rows_of):
        first[r] = RR.sample(img, plans[i][4][0][1:7])
        first_set[r] = -1 if set_of is None else set_of[i]
    order = [(i, j) for i, p in enumerate(plans) for j in range(1, p[0])]
    passes = [(first, first_set)]
    if order:
        passes.append((np.stack([RR.sample(img, plans[i][4][j][1:7]) for i, j in order]), np.array([-1 if set_of is None else set_of[i] for i, _ in order], np.int32)))
    read = []
    for crops, so in passes:
        if masks is not None:
            lg, _ = eng.parseq_logits(crops, set_of=so, sets=masks)
            read.append(eng.logits_confidence(lg, set_of=so, sets=masks))
        else:
            lg, _ = eng.parseq_logits(crops)
            read.append(eng.logits_confidence(lg))
    rows = [[None] * p[0] for p in plans]
    for i, r in enumerate(rows_of):
        rows[i][0] = (read[0][0][r], read[0][1][r], read[0][2][r])
    for k, (i, j) in enumerate(order):
        rows[i][j] = (read[1][0][k], read[1][1][k], read[1][2][k])
    return plans, rows


def _check_item(texts_k, ids_k, prob_k, conf_k, pieces, plan, rows, piece_cuts_k, quad):
    """one item against its reference pieces: every piece's ids, prob and conf bit for bit; text the concatenation; conf the fp32 product from 1.0f; ids
    and prob the first piece's; the cuts and the piece quads the rule's"""
    from tuatara_amd.engine import decode_ids
    n, _, _, cuts, _ = plan
    p_ids, p_prob, p_conf, p_quad = pieces
    assert len(p_ids) == n
    assert np.array_equal(piece_cuts_k, cuts if n > 1 else np.array([0, 128] + [-1] * 15, np.int32))
    conf = np.float32(1.0)
    text = ""
    for j in range(n):
        assert p_ids[j].tobytes() == rows[j][0].tobytes(), j
        assert p_prob[j].tobytes() == rows[j][1].tobytes(), j
        assert np.float32(p_conf[j]).tobytes() == np.float32(rows[j][2]).tobytes(), j
        conf = np.float32(conf * np.float32(rows[j][2]))
        text += decode_ids(rows[j][0])
    assert texts_k == text
    assert np.asarray(ids_k, np.int32).tobytes() == rows[0][0].tobytes() and np.asarray(prob_k, np.float32).tobytes() == rows[0][1].tobytes()
    if n > 1:
        assert np.float32(conf_k).tobytes() == conf.tobytes()
        assert np.asarray(p_quad, np.float32).tobytes() == WR.piece_quads(quad, cuts, n).tobytes()
    else:
        assert np.float32(conf_k).tobytes() == np.float32(rows[0][2]).tobytes()
        assert np.asarray(p_quad, np.float32).ravel().tobytes() == np.asarray(quad, np.float32).tobytes()


@pytest.mark.parametrize("precision", ["f16x4", "f32"])
def test_region_call(engines, precision):
    """One 96 x 1400 page: two ordinary regions, wide ones with n = 2, 3 and 16, one at exactly max_aspect (n = 1); two of them under character sets of
    their own.  Every piece equals the stage calls on numpy crops bit for bit and obeys its region's mask."""
    from tuatara_amd.engine import charset_masks
    eng = engines(precision)
    img = _bars(4, 96, 1400)
    regions = [{"rect": (10, 5, 110, 35)},                                   # 100 x 30: ordinary
               {"rect": (20, 40, 320, 64), "set": 0},                         # 300 x 24: n = 2, digits
               {"quad": GR.tilted_quad(700.0, 50.0, 60.0, 20.0, -8.0)},       # ordinary, tilted
               {"rect": (400, 8, 800, 28), "set": 1},                         # 400 x 20: n = 3, capitals
               {"rect": (10, 80, 1390, 91)},                                  # 1380 x 11: n = 16
               {"rect": (900, 10, 1028, 26)}]                                 # 128 x 16: exactly max_aspect, n = 1
    charsets = [(DIGITS, None), (UPPER, None)]
    masks = charset_masks(charsets)
    from tuatara_amd.engine import region_quad
    quads = np.stack([region_quad(r["quad"] if "quad" in r else r["rect"]) for r in regions])
    set_of = [r.get("set", -1) for r in regions]
    eng.set_wide(8.0)
    try:
        assert eng.wide == 8.0
        got = eng.read_regions(img, regions, charsets)
    finally:
        eng.set_wide(0)
    plans, rows = _reference_rows(eng, img, quads, 8.0, set_of, masks)
    assert [p[0] for p in plans] == [1, 2, 1, 3, 16, 1]
    assert len(got) == len(regions)
    for k, it in enumerate(got):
        assert it["region"] == k and it["set"] == set_of[k] and np.asarray(it["quad"], np.float32).tobytes() == quads[k].tobytes()
        assert np.asarray(it["bbox"], np.float32).tobytes() == GR.region_bbox(quads[k]).tobytes()
        _check_item(it["text"], it["ids"], it["prob"], it["conf"], (it["piece_ids"], it["piece_prob"], it["piece_conf"], it["piece_quad"]), plans[k], rows[k],
                    it["piece_cuts"], quads[k])
        assert [p["text"] for p in it["pieces"]] and "".join(p["text"] for p in it["pieces"]) == it["text"]
        if set_of[k] >= 0:                                                    # every piece inside its region's mask
            for j in range(plans[k][0]):
                assert CR.allowed(masks[set_of[k]])[it["piece_ids"][j]].all(), (k, j)
    off = eng.read_regions(img, regions, charsets)                            # wide off: no pieces, and the ordinary regions read what they read with it on
    assert all("pieces" not in it for it in off)
    for k in (0, 2, 5):
        assert off[k]["ids"] == got[k]["ids"] and off[k]["text"] == got[k]["text"] and np.float32(off[k]["conf"]).tobytes() == np.float32(got[k]["conf"]).tobytes()


# ------------------------------------------------------------------------------------------------- 3. / 4. page calls
def _page(eng, img, wide):
    eng.set_wide(wide)
    try:
        return eng.images_to_data([img], conf=True)[0]
    finally:
        eng.set_wide(0)


def _same_items(a, b):
    assert a.texts == b.texts and a.ids.tobytes() == b.ids.tobytes() and a.prob.tobytes() == b.prob.tobytes() and a.conf.tobytes() == b.conf.tobytes()
    assert a.bbox.tobytes() == b.bbox.tobytes() and a.quad.tobytes() == b.quad.tobytes()


def test_page_call_with_wide_words(engines, pages):
    """set_wide(2.0) makes ordinary detected words wide: item count, order, bbox and quad equal wide off; every one-piece item equals wide off bit for bit;
    every wide item equals the stage calls on crops made from the page's pixels."""
    eng = engines()
    for img in pages:
        off = _page(eng, img, 0)
        on = _page(eng, img, 2.0)
        assert off.piece_first is None and on.piece_first is not None
        assert len(on) == len(off) > 0 and on.bbox.tobytes() == off.bbox.tobytes() and on.quad.tobytes() == off.quad.tobytes()
        n_of = np.array([WR.plan(q, 2.0)[0] for q in off.quad])
        wide = np.nonzero(n_of >= 2)[0]
        assert len(wide) >= 10, len(wide)
        assert on.piece_first.tolist() == np.concatenate([[0], np.cumsum(n_of)]).tolist()
        for k in np.nonzero(n_of == 1)[0]:
            assert on.texts[k] == off.texts[k] and on.ids[k].tobytes() == off.ids[k].tobytes() and on.prob[k].tobytes() == off.prob[k].tobytes(), k
            assert on.conf[k].tobytes() == off.conf[k].tobytes(), k
            a = int(on.piece_first[k])
            assert on.piece_ids[a].tobytes() == off.ids[k].tobytes() and on.piece_prob[a].tobytes() == off.prob[k].tobytes(), k
            assert on.piece_conf[a].tobytes() == off.conf[k].tobytes() and on.piece_quad[a].tobytes() == off.quad[k].tobytes(), k
            assert on.piece_cuts[k].tolist() == [0, 128] + [-1] * 15
        plans, rows = _reference_rows(eng, img, off.quad[wide], 2.0, rows_of=wide, n_rows=len(off))
        for r, k in enumerate(wide):
            a, b = int(on.piece_first[k]), int(on.piece_first[k + 1])
            _check_item(on.texts[k], on.ids[k], on.prob[k], on.conf[k], (on.piece_ids[a:b], on.piece_prob[a:b], on.piece_conf[a:b], on.piece_quad[a:b]),
                        plans[r], rows[r], on.piece_cuts[k], off.quad[k])
            d = on[int(k)]
            assert [p["text"] for p in d["pieces"]] == [on.pieces(int(k))[j]["text"] for j in range(b - a)] and "".join(p["text"] for p in d["pieces"]) == d["text"]
        _same_items(_page(eng, img, 0), off)                                  # and the engine is what it was


def test_wide_on_with_no_wide_word_is_wide_off(engines, pages):
    """set_wide(64.0): no detected word is that wide, so the whole result equals wide off bit for bit and piece_first is 0..count"""
    eng = engines()
    for img in pages:
        off = _page(eng, img, 0)
        on = _page(eng, img, 64.0)
        assert all(WR.plan(q, 64.0)[0] == 1 for q in off.quad)
        _same_items(on, off)
        assert on.piece_first.tolist() == list(range(len(off) + 1))
        assert on.piece_ids.tobytes() == off.ids.tobytes() and on.piece_prob.tobytes() == off.prob.tobytes() and on.piece_conf.tobytes() == off.conf.tobytes()
        assert on.piece_quad.tobytes() == off.quad.tobytes()


def test_lines_and_blocks_do_not_change(engines, pages):
    """lines = 1, blocks = 1 with set_wide(2.0): items and their quads do not change, so neither do the line and block outputs"""
    eng = engines(layout=True)
    for img in pages:
        off = _page(eng, img, 0)
        on = _page(eng, img, 2.0)
        assert on.piece_first is not None and int(on.piece_first[-1]) > len(on)
        assert off.line is not None and off.block is not None and len(off.lines) > 0 and len(off.blocks) > 0
        for f in ("line", "word", "order", "line_first", "line_bbox", "block", "line_block", "line_pos", "block_order", "block_first", "block_bbox"):
            assert getattr(on, f).tobytes() == getattr(off, f).tobytes(), f
        assert on.block_mode == off.block_mode
        assert [ln["items"] for ln in on.lines] == [ln["items"] for ln in off.lines] and [b["lines"] for b in on.blocks] == [b["lines"] for b in off.blocks]


# ------------------------------------------------------------------------------------------------- 6. streaming and the list form
def _same_pieces(a, b):
    _same_items(a, b)
    for f in ("piece_first", "piece_ids", "piece_prob", "piece_conf", "piece_quad", "piece_cuts"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_streamed_batches_and_the_list_form(engines):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    eng = engines()
    imgs = [synth.synthetic_page(80 + i, 512, 384, n_words=10) for i in range(3)]
    bufs = [DeviceBuffer(2 * 512 * 384 * 3), DeviceBuffer(512 * 384 * 3), DeviceBuffer(3 * 512 * 384 * 3)]
    eng.set_wide(2.0)
    try:
        bufs[0].upload(np.stack(imgs[:2]))
        bufs[1].upload(imgs[2])
        sync = eng.pages_to_data_dev(bufs[0], 2, 512, 384, conf=True) + eng.pages_to_data_dev(bufs[1], 1, 512, 384, conf=True)
        assert all(p.piece_first is not None and int(p.piece_first[-1]) > len(p) for p in sync)
        got = eng.stream_push(bufs[0], 2, 512, 384, conf=True)
        got += eng.stream_push(bufs[1], 1, 512, 384, conf=True)
        while True:
            more = eng.stream_flush(conf=True)
            if not more:
                break
            got += more
        assert len(got) == 3
        for a, b in zip(got, sync):
            _same_pieces(a, b)
        bufs[2].upload(np.stack(imgs))                                         # the list form runs same-sized images as one batch: against the call on that batch
        sync3 = eng.pages_to_data_dev(bufs[2], 3, 512, 384, conf=True)
        listed = eng.images_to_data(imgs, conf=True)
        assert len(listed) == 3 and eng.last_images_batches() == [3]
        for a, b in zip(listed, sync3):
            _same_pieces(a, b)
    finally:
        eng.set_wide(0)
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_every_refusal_by_name(engines, eng_x4, weights):
    from tuatara_amd import synth
    from tuatara_amd.engine import CROP_RECTIFIED, Comm, DeviceBuffer, Engine, EngineError
    eng = engines()
    img = synth.synthetic_page(85, 512, 384, n_words=6)

    def refused(e, match, value=8.0):
        before = e.wide
        with pytest.raises(EngineError, match=match):
            e.set_wide(value)
        assert e.wide == before

    for bad in (1.0, 1.99, 64.5, float("nan"), float("inf"), -8.0):
        refused(eng, "max_aspect", bad)
    refused(eng_x4, "crop_mode")                                              # crop_mode 0
    for kw, match in ((dict(orient=1), "orientation"), (dict(chars=1), "character boxes")):
        e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, **kw)
        try:
            refused(e, match)
        finally:
            e.close()
    eng.set_alternatives(3)
    try:
        refused(eng, "alternatives")
    finally:
        eng.set_alternatives(0)
    eng.set_lexicon(["abc", "de"], 1)
    try:
        refused(eng, "lexicon")
    finally:
        eng.set_lexicon(None)
    eng.set_pattern(r"\d+")
    try:
        refused(eng, "pattern")
    finally:
        eng.set_pattern(None)
    buf = DeviceBuffer(512 * 384 * 3)
    buf.upload(img)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            refused(eng, "communicator")
        finally:
            comm.attach(False)
        eng.stream_push(buf, 1, 512, 384)                                     # while batches stream: the setter and the stage call
        try:
            refused(eng, "streamed batches")
            with pytest.raises(EngineError, match="streamed batches"):
                eng.wide_cuts(img, WR.quad_of(5, 5, 200, 10)[None], 8.0)
        finally:
            while eng.stream_flush():
                pass
        # the other way round, with wide on
        eng.set_wide(4.0)
        try:
            with pytest.raises(EngineError, match="wide"):
                eng.set_alternatives(3)
            with pytest.raises(EngineError, match="wide"):
                eng.set_lexicon(["abc"], 1)
            with pytest.raises(EngineError, match="wide"):
                eng.set_pattern(r"\d+")
            with pytest.raises(EngineError, match="wide"):
                comm.attach(True)
            with pytest.raises(EngineError, match="wide"):
                comm.pages_to_data_sharded(buf, 1, 512, 384)
            with pytest.raises(EngineError, match="wide"):
                eng.read_regions(img, [{"rect": (5, 5, 200, 25)}], patterns=[r"\d+"])
            assert eng.wide == 4.0 and eng.alternatives == 0 and eng.lexicon_size == 0 and eng.pattern is None
            eng.stream_push(buf, 1, 512, 384)
            try:
                with pytest.raises(EngineError, match="streamed batches"):
                    eng.set_wide(0)
                assert eng.wide == 4.0
            finally:
                while eng.stream_flush():
                    pass
        finally:
            eng.set_wide(0)
        with pytest.raises(EngineError, match="max_aspect"):
            eng.wide_cuts(img, WR.quad_of(5, 5, 200, 10)[None], 1.0)
        with pytest.raises(EngineError, match="not finite"):
            eng.wide_cuts(img, np.full((1, 8), np.inf, np.float32), 8.0)
    finally:
        comm.close()
        buf.free()
    assert eng.wide == 0.0
    assert len(eng.image_to_data(img)) > 0                                    # and the engine still reads


# ------------------------------------------------------------------------------------------------- 8. callers
def test_pytuatara_and_ocr_cli(engines, weights, funsd, monkeypatch, tmp_path):
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    eng = engines()
    want = _page(eng, funsd, 2.0)
    got = pytuatara.image_to_data(funsd, weights["dir"], "o", wide=2.0, conf=True)
    assert len(got) == len(want) > 0 and "pieces" in got[0] and "quad" in got[0]
    assert sum(len(g["pieces"]) > 1 for g in got) >= 10
    for k, g in enumerate(got):
        w = want[k]
        assert g["text"] == w["text"] and list(g["bbox"]) == w["bbox"] and np.float32(g["conf"]).tobytes() == want.conf[k].tobytes()
        assert [(p["text"], np.float32(p["conf"]).tobytes()) for p in g["pieces"]] == [(p["text"], np.float32(p["conf"]).tobytes()) for p in w["pieces"]]
        assert np.asarray([p["quad"] for p in g["pieces"]], np.float32).tobytes() == np.asarray([p["quad"] for p in w["pieces"]], np.float32).tobytes()
    plain = pytuatara.image_to_data(funsd, weights["dir"], "o", rectify=True)          # the call's setting is gone afterwards
    assert "pieces" not in plain[0] and [p["text"] for p in plain] == _page(eng, funsd, 0).texts
    with pytest.raises(ValueError, match="wide"):
        pytuatara.image_to_data(funsd, weights["dir"], "o", wide=True, alts=3)
    # ocr_cli --wide 2: "bbox<TAB>conf<TAB>text", and one "<TAB>|conf text" line per piece under a wide item
    png = os.path.join(DATA, "funsd_0001129658.png")
    bgr = np.ascontiguousarray(funsd[:, :, ::-1])                                     # the CLI feeds BGR
    want = _page(eng, bgr, 2.0)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--wide", "2", png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    items = [ln.split("\t") for ln in lines if not ln.startswith("\t")]
    assert len(items) == len(want)
    for k, (bb, cf, text) in enumerate(items):
        assert [float(v) for v in bb.split()] == want.bbox[k].tolist() and text == want.texts[k] and abs(float(cf) - float(want.conf[k])) <= 1e-6
    assert sum(ln.startswith("\t|") for ln in lines) == sum(len(want.pieces(k)) for k in range(len(want)) if len(want.pieces(k)) > 1)
