"""GPU suite for curved words (DESIGN.md "Curved words"): curve_crop_kernel against the host rule and tests/curve_ref.py, a region call over hand-made arc
words against crops made in numpy and the oracle's reading of them, page calls on a synthetic arched page and the FUNSD page, curved off against the parent's
behaviour, lines and blocks, the list, `_v`, streamed and region entry points, every refusal, and the callers.  Every test here fails on the parent commit:
Engine.set_curved / Engine.curve_crops and their symbols are absent."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CC
from tests import curve_ref as CV
from tests import regions_ref as GR
from tests.conftest import ROOT

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
def arched():
    from tuatara_amd import synth
    return synth.synthetic_arched_page(1)[0]


def _arc_page(seed=0):
    """a 256 x 256 page of light noise holding one dark arc word (11 bars, sagitta two bar heights, tilted 10 degrees) -> (image, the word's quad)"""
    img, quad = CV.arc_word(11, 10.0, 20.0, 150.0, 10.0, True, True)
    rng = np.random.default_rng(seed)
    img = np.where(img > 128, rng.integers(240, 256, img.shape[:2], dtype=np.uint8)[..., None].repeat(3, 2), img).astype(np.uint8)
    return np.ascontiguousarray(img), quad


def _quads40(quad):
    """40 quads over a 256 x 256 page: the arc word's own quad, straight, tilted and arched-both-ways boxes about the page, four partly outside it"""
    rng = np.random.default_rng(9)
    out = [quad, CV.quad_of(128, 128, 160, 60, 10.0), CV.quad_of(128, 150, 170, 70, -170.0)]          # the last: the word upside down, so arched the other way
    for i in range(33):
        out.append(CV.quad_of(float(rng.uniform(60, 196)), float(rng.uniform(60, 196)), float(rng.uniform(40, 200)), float(rng.uniform(8, 80)), (0.0, 17.0, -30.0)[i % 3]))
    out += [CV.quad_of(10, 128, 160, 50, 0.0), CV.quad_of(250, 128, 160, 50, 5.0), CV.quad_of(128, 5, 150, 40, -8.0), CV.quad_of(128, 252, 150, 40, 3.0)]
    out = np.stack(out)
    assert len(out) == 40 and sum(not GR.inside(q, 256, 256) for q in out) >= 4
    return out


def _check_against_host(img, quads, got):
    from tuatara_amd import engine as E
    flag, hb, spine, knots, crops = got
    for i, q in enumerate(quads):
        h = E.curve_knots(img, E.curve_frame(q))
        assert flag[i] == h["flag"] and np.array_equal(hb[i], h["hb"]) and np.array_equal(spine[i], h["spine"]) and np.array_equal(knots[i], h["knots"]), i
        want = E.curve_crop(img, h["knots"]) if h["flag"] else GR.region_crop(img, q)
        assert np.array_equal(crops[i], want), i


# ------------------------------------------------------------------------------------------------- 1. the kernel against the host rule
@pytest.mark.parametrize("table", [False, True])
def test_curve_crops_equals_the_host_rule(engines, table):
    """40 quads in one launch over a 256 x 256 page, through the uniform and the page-table form: flag, half bands, spine rows, knot table and crop bit for
    bit against the host rule, and the host rule against the numpy reference; curved and straight words both occur."""
    eng = engines()
    img, quad = _arc_page()
    quads = _quads40(quad)
    got = eng.curve_crops(img, quads, table=table)
    _check_against_host(img, quads, got)
    assert got[0][0] == 1 and got[0][2] == 1 and 0 < int(got[0].sum()) < 40
    for i in (0, 1, 2, 36, 39):
        r = CV.word(img, quads[i])
        assert got[0][i] == r["flag"] and np.array_equal(got[1][i], r["hb"]) and np.array_equal(got[2][i], r["spine"]) and np.array_equal(got[3][i], r["table"]), i
        if r["flag"]:
            assert np.array_equal(got[4][i], CV.crop(img, r["table"])), i


def test_curve_crops_a_few_thousand_words(engines):
    """one launch of 3000 words: the 40 quads over and over, every word equal to its first occurrence"""
    eng = engines()
    img, quad = _arc_page()
    quads = np.tile(_quads40(quad), (75, 1))
    flag, hb, spine, knots, crops = eng.curve_crops(img, quads)
    assert len(flag) == 3000
    _check_against_host(img, quads[:40], (flag, hb, spine, knots, crops))
    for name, a in (("flag", flag), ("hb", hb), ("spine", spine), ("knots", knots), ("crops", crops)):
        a = a.reshape(75, 40, -1)
        assert (a == a[:1]).all(), name


# ------------------------------------------------------------------------------------------------- 2. a region call
def _oracle_agrees(eng, oracle_models, crops):
    """the engine's logits on these crops lie within 1e-3 of the CPU oracle's, and both read the same ids wherever the oracle's own choice is clear of that
    bar (its best class leads the second by more than 2e-3)"""
    from oracle import pipeline
    lg = np.asarray(eng.parseq_logits(crops)[0]).reshape(-1, 26, 95)
    o_lg = pipeline.parseq_logits(oracle_models[1], crops)
    assert np.abs(lg - o_lg).max() <= 1e-3, float(np.abs(lg - o_lg).max())
    top = np.sort(o_lg, -1)
    clear = top[..., -1] - top[..., -2] > 2e-3
    assert clear.any() and (lg.argmax(-1) == o_lg.argmax(-1))[clear].all()


def _arc_regions():
    """one 256 x 512 page holding two arc words (arched up, dark on light; arched down, light on dark) and a straight one -> (image, quads f32 [3, 8])"""
    a, qa = CV.arc_word(11, 10.0, 20.0, 150.0, 8.0, True, True)
    b, qb = CV.arc_word(8, 12.0, 18.0, 160.0, -12.0, False, False)
    img = np.concatenate([a, b], 1)
    qb = qb.copy()
    qb[0::2] += 256.0
    img[8:24, 40:200] = 20                                                     # a straight bar on the light half
    return np.ascontiguousarray(img), np.stack([qa, qb, GR.region_from_rect(36, 4, 204, 28)])


@pytest.mark.parametrize("precision", ["f16x4", "f32"])
def test_region_call(engines, oracle_models, precision):
    """Regions drawn round hand-made arc words, two of them under character sets of their own: the flags are the rule's, the crops the recogniser read are
    numpy's (through the stage call, which runs the same kernel), the logits on those crops lie within 1e-3 of the oracle's, and ids and texts are the
    oracle's masked reading of them."""
    from tuatara_amd.engine import charset_masks, decode_ids
    eng = engines(precision)
    img, quads = _arc_regions()
    regions = [{"quad": quads[0], "set": 0}, {"quad": quads[1]}, {"quad": quads[2], "set": 1}]
    charsets = [(DIGITS, None), (UPPER, None)]
    masks = charset_masks(charsets)
    set_of = np.array([0, -1, 1], np.int32)
    ref = [CV.word(img, q) for q in quads]
    assert [r["flag"] for r in ref] == [1, 1, 0]
    want_crops = np.stack([CV.crop(img, r["table"]) if r["flag"] else GR.region_crop(img, q) for r, q in zip(ref, quads)])
    assert np.array_equal(eng.curve_crops(img, quads)[4], want_crops)
    eng.set_curved(True)
    try:
        assert eng.curved
        got = eng.read_regions(img, regions, charsets)
    finally:
        eng.set_curved(False)
    _oracle_agrees(eng, oracle_models, want_crops)                            # the recogniser on those crops, no set: the oracle's logits and reading
    lg, _ = eng.parseq_logits(want_crops, set_of=set_of, sets=masks)          # ... and under the regions' sets: the stage calls' reading, bit for bit
    ids, prob, conf = eng.logits_confidence(lg, set_of=set_of, sets=masks)
    for k, it in enumerate(got):
        assert it["curved"] == ref[k]["flag"] and np.array_equal(it["spine_knots"], ref[k]["table"]), k
        assert np.asarray(it["outline"], np.float32).tobytes() == CV.outline(quads[k], ref[k]["flag"], ref[k]["table"]).tobytes(), k
        assert it["text"] == decode_ids(ids[k]), k
        if set_of[k] >= 0:
            assert CC.allowed(masks[set_of[k]])[np.asarray(it["ids"])].all(), k
        assert np.asarray(it["ids"], np.int32).tobytes() == ids[k].tobytes() and np.asarray(it["prob"], np.float32).tobytes() == prob[k].tobytes(), k
        assert np.float32(it["conf"]).tobytes() == np.float32(conf[k]).tobytes(), k
        assert np.asarray(it["quad"], np.float32).tobytes() == quads[k].tobytes() and np.asarray(it["bbox"], np.float32).tobytes() == GR.region_bbox(quads[k]).tobytes()
    off = eng.read_regions(img, regions, charsets)                            # curved off: no such keys, and the straight region reads what it read with it on
    assert all("curved" not in it and "outline" not in it for it in off)
    assert off[2]["ids"] == got[2]["ids"] and np.float32(off[2]["conf"]).tobytes() == np.float32(got[2]["conf"]).tobytes()


# ------------------------------------------------------------------------------------------------- 3. page calls
def _page(eng, img, on):
    eng.set_curved(on)
    try:
        return eng.images_to_data([img], conf=True)[0]
    finally:
        eng.set_curved(False)


def _same_items(a, b, rows=None):
    rows = range(len(a)) if rows is None else rows
    assert len(a) == len(b)
    for k in rows:
        assert a.texts[k] == b.texts[k] and a.ids[k].tobytes() == b.ids[k].tobytes() and a.prob[k].tobytes() == b.prob[k].tobytes(), k
        assert a.conf[k].tobytes() == b.conf[k].tobytes() and a.bbox[k].tobytes() == b.bbox[k].tobytes() and a.quad[k].tobytes() == b.quad[k].tobytes(), k


def _check_page(eng, img, off, on, oracle_models):
    from tuatara_amd.engine import decode_ids
    assert off.curved is None and on.curved is not None and len(on) == len(off) > 0
    assert on.bbox.tobytes() == off.bbox.tobytes() and on.quad.tobytes() == off.quad.tobytes()
    ref = [CV.word(img, q) for q in off.quad]
    assert on.curved.tolist() == [r["flag"] for r in ref]
    straight = [k for k, r in enumerate(ref) if not r["flag"]]
    _same_items(on, off, straight)                                           # items flagged 0: curved off, bit for bit
    for k, r in enumerate(ref):
        assert np.array_equal(on.spine_knots[k], r["table"]), k
        assert on.outline[k].tobytes() == CV.outline(off.quad[k], r["flag"], r["table"]).tobytes(), k
        d = on[k]
        assert d["curved"] == r["flag"] and np.asarray(d["outline"], np.float32).tobytes() == on.outline[k].tobytes()
    bent = [k for k, r in enumerate(ref) if r["flag"]]
    if bent:   # flagged items: the numpy reference's crops, read as the stage calls read them in a batch of the page's row count, and as the oracle reads them
        crops = np.stack([CV.crop(img, ref[k]["table"]) for k in bent])
        got = eng.curve_crops(img, off.quad[bent])
        assert np.array_equal(got[4], crops) and got[0].tolist() == [1] * len(bent)
        batch = np.zeros((len(off), 32, 128, 3), np.uint8)                    # (a row's reading does not depend on its neighbours; the kernels picked depend on the row count)
        batch[bent] = crops
        ids, prob, conf = eng.logits_confidence(eng.parseq_logits(batch)[0])
        for k in bent:
            assert on.ids[k].tobytes() == ids[k].tobytes() and on.prob[k].tobytes() == prob[k].tobytes() and on.conf[k].tobytes() == conf[k].tobytes(), k
            assert on.texts[k] == decode_ids(ids[k]), k
        _oracle_agrees(eng, oracle_models, crops)
    return bent


def test_page_call_on_an_arched_page(engines, arched, oracle_models):
    """a synthetic page of arched noise words and straight ones: at least two words are flagged; items flagged 0 equal curved off bit for bit; flagged items
    are read from the numpy reference's crops as the oracle reads them; outlines and knot tables are the rule's"""
    eng = engines()
    off = _page(eng, arched, False)
    on = _page(eng, arched, True)
    bent = _check_page(eng, arched, off, on, oracle_models)
    assert len(bent) >= 2 and len(bent) < len(on)
    _same_items(_page(eng, arched, False), off)                              # and the engine is what it was


def test_page_call_on_the_funsd_page(engines, funsd, oracle_models):
    eng = engines()
    off = _page(eng, funsd, False)
    on = _page(eng, funsd, True)
    _check_page(eng, funsd, off, on, oracle_models)


# ------------------------------------------------------------------------------------------------- 4. the off path
def test_curved_off_is_the_parents_result(engines, eng_x4, arched):
    """with curved off - never set, or set and cleared - a page's dicts carry the keys of before and the engine in crop_mode 0 refuses the setting and reads on"""
    from tuatara_amd.engine import EngineError
    eng = engines()
    a = eng.images_to_data([arched], conf=True)[0]
    eng.set_curved(True)
    eng.set_curved(False)
    b = eng.images_to_data([arched], conf=True)[0]
    _same_items(a, b)
    assert a.curved is None and b.curved is None and b.outline is None and b.spine_knots is None
    assert set(b[0].keys()) == {"text", "bbox", "ids", "quad", "conf", "char_conf"}
    before = eng_x4.image_to_data(arched)
    with pytest.raises(EngineError, match="crop_mode"):
        eng_x4.set_curved(True)
    assert not eng_x4.curved and eng_x4.image_to_data(arched) == before and set(before[0].keys()) == {"text", "bbox", "ids"}


# ------------------------------------------------------------------------------------------------- 5. compositions
def test_lines_and_blocks_do_not_change(engines, arched):
    eng = engines(layout=True)
    off = _page(eng, arched, False)
    on = _page(eng, arched, True)
    assert int(on.curved.sum()) >= 2 and off.line is not None and off.block is not None and len(off.lines) > 0 and len(off.blocks) > 0
    for f in ("line", "word", "order", "line_first", "line_bbox", "block", "line_block", "line_pos", "block_order", "block_first", "block_bbox"):
        assert getattr(on, f).tobytes() == getattr(off, f).tobytes(), f


def _same_curved(a, b):
    _same_items(a, b)
    for f in ("curved", "outline", "spine_knots"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_every_entry_point(engines):
    """the synchronous call, streamed batches with one page per batch, the list form and the `_v` form (pages of two sizes) give the same curved results"""
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    eng = engines()
    imgs = [synth.synthetic_arched_page(2 + i, 384, 512, n_words=4)[0] for i in range(2)]
    bufs = [DeviceBuffer(384 * 512 * 3) for _ in range(2)]
    eng.set_curved(True)
    try:
        for b, im in zip(bufs, imgs):
            b.upload(im)
        sync = [eng.pages_to_data_dev(b, 1, 384, 512, conf=True)[0] for b in bufs]
        assert all(p.curved is not None and int(p.curved.sum()) >= 1 for p in sync)
        got = []
        for b in bufs:
            got += eng.stream_push(b, 1, 384, 512, conf=True)
        while True:
            more = eng.stream_flush(conf=True)
            if not more:
                break
            got += more
        assert len(got) == 2
        for a, b in zip(got, sync):
            _same_curved(a, b)
        both = DeviceBuffer(2 * 384 * 512 * 3)                                # the list form runs same-sized images as one batch: against the call on that batch
        bufs.append(both)
        both.upload(np.stack(imgs))
        sync2 = eng.pages_to_data_dev(both, 2, 384, 512, conf=True)
        listed = eng.images_to_data(imgs, conf=True)
        assert len(listed) == 2 and eng.last_images_batches() == [2]
        for a, b in zip(listed, sync2):
            _same_curved(a, b)
        mixed = eng.pages_to_data_dev_v([(bufs[0], 384, 512, 0)], conf=True)  # the page-table form of the packer and of curve_crop_kernel
        assert len(mixed) == 1
        _same_curved(mixed[0], sync[0])
    finally:
        eng.set_curved(False)
        for b in bufs:
            b.free()


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_by_name(engines, eng_x4, weights, arched):
    from tuatara_amd.engine import CROP_RECTIFIED, Comm, DeviceBuffer, Engine, EngineError
    eng = engines()
    img = np.ascontiguousarray(arched[:384, :512])

    def refused(e, match):
        with pytest.raises(EngineError, match=match):
            e.set_curved(True)
        assert not e.curved

    refused(eng_x4, "crop_mode")
    for kw, match in ((dict(orient=1), "orientation"), (dict(chars=1), "character boxes")):
        e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, **kw)
        try:
            refused(e, match)
        finally:
            e.close()
    eng.set_wide(8.0)
    try:
        refused(eng, "wide")
    finally:
        eng.set_wide(0)
    assert eng.lib.ttr_engine_set_curved(eng.h, 2) == -1 and b"0 or 1" in eng.lib.ttr_last_error()
    buf = DeviceBuffer(384 * 512 * 3)
    buf.upload(img)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            refused(eng, "communicator")
        finally:
            comm.attach(False)
        eng.stream_push(buf, 1, 384, 512)
        try:
            refused(eng, "streamed batches")
            with pytest.raises(EngineError, match="streamed batches"):
                eng.curve_crops(img, CV.quad_of(100, 100, 150, 40)[None])
        finally:
            while eng.stream_flush():
                pass
        eng.set_curved(True)                                                  # the other way round
        try:
            with pytest.raises(EngineError, match="curved"):
                eng.set_wide(8.0)
            with pytest.raises(EngineError, match="curved"):
                comm.attach(True)
            with pytest.raises(EngineError, match="curved"):
                comm.pages_to_data_sharded(buf, 1, 384, 512)
            assert eng.curved and eng.wide == 0.0
            eng.set_alternatives(3)                                           # what acts on recogniser rows combines
            eng.set_alternatives(0)
            eng.stream_push(buf, 1, 384, 512)
            try:
                with pytest.raises(EngineError, match="streamed batches"):
                    eng.set_curved(False)
                assert eng.curved
            finally:
                while eng.stream_flush():
                    pass
        finally:
            eng.set_curved(False)
        with pytest.raises(EngineError, match="not finite"):
            eng.curve_crops(img, np.full((1, 8), np.inf, np.float32))
    finally:
        comm.close()
        buf.free()
    assert not eng.curved and len(eng.image_to_data(img)) > 0


# ------------------------------------------------------------------------------------------------- 7. callers
def test_pytuatara_and_ocr_cli(engines, weights, arched, monkeypatch, tmp_path):
    from PIL import Image
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    eng = engines()
    want = _page(eng, arched, True)
    got = pytuatara.image_to_data(arched, weights["dir"], "o", curved=True, conf=True)
    assert len(got) == len(want) > 0 and sum(g["curved"] for g in got) == int(want.curved.sum()) >= 2
    for k, g in enumerate(got):
        assert g["text"] == want.texts[k] and list(g["bbox"]) == want.bbox[k].tolist() and np.float32(g["conf"]).tobytes() == want.conf[k].tobytes()
        assert bool(g["curved"]) == bool(want.curved[k]) and np.asarray(g["outline"], np.float32).tobytes() == want.outline[k].tobytes()
    plain = pytuatara.image_to_data(arched, weights["dir"], "o", rectify=True)            # the call's setting is gone afterwards
    assert "curved" not in plain[0] and [p["text"] for p in plain] == _page(eng, arched, False).texts
    with pytest.raises(ValueError, match="curved"):
        pytuatara.image_to_data(arched, weights["dir"], "o", curved=True, wide=True)
    # ocr_cli --curved: "bbox<TAB>conf<TAB>text", and one "<TAB>~x y x y ..." line with the outline under a curved item
    png = str(tmp_path / "arched.png")
    Image.fromarray(arched).save(png)
    bgr = np.ascontiguousarray(arched[:, :, ::-1])                                      # the CLI feeds BGR
    want = _page(eng, bgr, True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--curved", png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    items = [ln.split("\t") for ln in lines if not ln.startswith("\t")]
    assert len(items) == len(want)
    for k, (bb, cf, text) in enumerate(items):
        assert [float(v) for v in bb.split()] == want.bbox[k].tolist() and text == want.texts[k] and abs(float(cf) - float(want.conf[k])) <= 1e-6
    outlines = [np.array([float(v) for v in ln[2:].split()], np.float32) for ln in lines if ln.startswith("\t~")]
    assert len(outlines) == int(want.curved.sum()) >= 2
    for o, k in zip(outlines, np.nonzero(want.curved)[0]):
        assert o.tobytes() == want.outline[k].ravel().tobytes()
