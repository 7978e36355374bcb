"""GPU suite for regions and per-row character sets (DESIGN.md "Regions and per-row character sets"): the decode kernel with rows of different sets
against float64, the recogniser with a row table against the same crops under each set alone (the uniform path, which tests/test_gpu_charset.py holds
to the masked oracle), the four places a token is chosen against each other, the region crops against numpy, the round trip of a page's own quads, the
page entry points and callers against each other, and the refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests import regions_ref as GR
from tests.conftest import DATA, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"


# ------------------------------------------------------------------------------------------------- 1. the decode kernel, rows of different sets
def _adversarial_logits(n, seed, blocked_of_row):
    """tests/test_gpu_charset.py's recipe restated, the blocked classes taken row by row: ties and +12 bumps on classes the ROW's mask blocks (kinds 7, 8)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    kind = rng.integers(0, 9, (n, 26))
    for i, p in zip(*np.nonzero(kind == 1)):                  # exact ties at the maximum: the first one wins
        t = rng.choice(95, rng.integers(2, 5), replace=False)
        x[i, p, t] = x[i, p].max() + 1.0
    for i, p in zip(*np.nonzero(kind == 2)):                  # all equal: id 0
        x[i, p] = np.float32(rng.normal())
    for i, p in zip(*np.nonzero(kind == 3)):                  # near one-hot
        x[i, p, rng.integers(0, 95)] += 40.0
    for i, p in zip(*np.nonzero(kind == 4)):                  # spreads up to +-1e30
        x[i, p] = rng.uniform(-1e30, 1e30, 95).astype(np.float32)
    for i, p in zip(*np.nonzero(kind == 5)):                  # an EOS (id 0) or a dropped id (88) at this position
        x[i, p, 0 if rng.random() < 0.5 else 88] += 12.0
    for i, p in zip(*np.nonzero(kind == 7)):                  # a blocked class ties with the maximum, in front of it or behind it
        if len(blocked_of_row[i]):
            x[i, p, rng.choice(blocked_of_row[i])] = x[i, p].max()
    for i, p in zip(*np.nonzero(kind == 8)):                  # a blocked class towers over the row
        if len(blocked_of_row[i]):
            x[i, p, rng.choice(blocked_of_row[i])] = x[i, p].max() + 12.0
    return x


def _check_decode(eng, x, masks, set_of, own):
    from tuatara_amd.engine import confidence_from_probs
    n = len(x)
    ids, prob, conf = eng.logits_confidence(x, set_of=set_of, sets=masks)
    r_ids, r_prob, r_conf, rows = GR.masked_decode_rows(x, masks, set_of, own)
    assert np.array_equal(ids, r_ids)
    rel = np.abs(prob.astype(np.float64) - r_prob) / r_prob
    print(f"n={n}: max relative |prob - float64| {rel.max():.2e}")
    assert rel.max() <= 2e-6
    assert (prob > 0).all() and (prob <= 1).all()
    for i in range(n):
        assert CR.allowed(rows[i])[ids[i]].all(), i                              # every id inside its own row's mask
        _, c = confidence_from_probs(ids[i], prob[i])
        assert c.tobytes() == conf[i:i + 1].tobytes(), (i, c, conf[i])
    for s in sorted(set(set_of)):                                                # every row: the bits of the masked call under that row's mask alone
        sel = np.nonzero(np.asarray(set_of) == s)[0]
        a_ids, a_prob, a_conf = eng.logits_confidence(x, mask=own if s < 0 else masks[s])
        assert ids[sel].tobytes() == a_ids[sel].tobytes() and prob[sel].tobytes() == a_prob[sel].tobytes() and conf[sel].tobytes() == a_conf[sel].tobytes(), s
    return ids


@pytest.mark.parametrize("n", [1, 7, 37])
def test_decode_kernel_rows_of_different_sets(eng_x4, n):
    from tuatara_amd.engine import charset_mask
    masks = np.stack([charset_mask(DIGITS), charset_mask("q"), charset_mask(None, "e"), charset_mask()])
    set_of = [i % 4 for i in range(n)]
    blocked = [np.nonzero(~CR.allowed(masks[s]))[0] for s in set_of]
    x = _adversarial_logits(n, 10 + n, blocked)
    ids = _check_decode(eng_x4, x, masks, set_of, CR.FULL)
    if n > 4:                                                                    # the masks had something to do, and differently from row to row
        assert any((~CR.allowed(masks[s])[x[i].argmax(-1)]).any() for i, s in enumerate(set_of))
        assert not np.array_equal(ids[0], x[0].argmax(-1)) or not np.array_equal(ids[4], x[4].argmax(-1))


def test_decode_kernel_a_row_under_the_engines_own_set(eng_x4):
    from tuatara_amd.engine import charset_mask
    masks = np.stack([charset_mask(DIGITS), charset_mask("q"), charset_mask(None, "e"), charset_mask()])
    n = 7
    set_of = [0, 1, -1, 3, 2, -1, 0]
    own = charset_mask(UPPER)
    blocked = [np.nonzero(~CR.allowed(own if s < 0 else masks[s]))[0] for s in set_of]
    x = _adversarial_logits(n, 99, blocked)
    assert np.array_equal(eng_x4.charset, CR.FULL)
    eng_x4.set_charset(UPPER)
    try:
        _check_decode(eng_x4, x, masks, set_of, own)
    finally:
        eng_x4.set_charset()
    # without an engine set, -1 is the full mask
    ids, prob, conf = eng_x4.logits_confidence(x, set_of=[-1] * n, sets=masks)
    p_ids, p_prob, p_conf = eng_x4.logits_confidence(x)
    assert ids.tobytes() == p_ids.tobytes() and prob.tobytes() == p_prob.tobytes() and conf.tobytes() == p_conf.tobytes()


# ------------------------------------------------------------------------------------------------- 2. the recogniser, 37 crops under three sets
SETS3 = ((DIGITS, None), (UPPER, None), (None, None))
_cache = {}


def _masks3():
    from tuatara_amd.engine import charset_mask
    return np.stack([charset_mask(a, d) for a, d in SETS3])


def _alone(eng, which, crops):
    """the 37 crops under each set alone through set_charset (the uniform, by-value path), once per engine: {set: (refined, AR, ids)}"""
    key = (which, "alone")
    if key not in _cache:
        runs = {}
        for s, (allow, deny) in enumerate(SETS3):
            eng.set_charset(allow, deny)
            try:
                runs[s] = eng.parseq_logits(crops, want_ar=True)
            finally:
                eng.set_charset()
        _cache[key] = runs
    return _cache[key]


@pytest.mark.parametrize("which", ["x4", "f32"])
def test_recogniser_rows_of_different_sets(which, eng_x4, eng_f32):
    from tuatara_amd.engine import decode_ids
    eng = eng_x4 if which == "x4" else eng_f32
    crops = CR.sweep_crops(21, 37)
    masks = _masks3()
    set_of = np.array([i % 3 for i in range(37)], np.int32)
    # the default early exit: refined logits and ids
    got, ids = eng.parseq_logits(crops, set_of=set_of, sets=masks)
    for s in range(3):
        eng.set_charset(*SETS3[s])
        try:
            a_got, a_ids = eng.parseq_logits(crops)
        finally:
            eng.set_charset()
        sel = set_of == s
        assert np.array_equal(got[sel], a_got[sel]) and np.array_equal(ids[sel], a_ids[sel]), s
    # the early exit off: the AR logits too, up to and including the row's own EOS
    try:
        assert eng.set_tuning("ar_early_exit", 0) == 0
        got0, ar0, ids0 = eng.parseq_logits(crops, want_ar=True, set_of=set_of, sets=masks)
        alone = _alone(eng, which + "-noexit", crops)
    finally:
        eng.set_tuning("ar_early_exit", 1)
    assert np.array_equal(got0, got) and np.array_equal(ids0, ids)                 # the exit changes nothing that is returned
    for s in range(3):
        a_got, a_ar, a_ids = alone[s]
        sel = np.nonzero(set_of == s)[0]
        assert np.array_equal(got0[sel], a_got[sel]) and np.array_equal(ids0[sel], a_ids[sel]), s
        choice, _, _ = CR.masked_decode(a_ar[sel], masks[s])
        up = CR.upto_first_eos(choice)
        assert np.array_equal(ar0[sel][up], a_ar[sel][up]), s
    for i in range(37):
        assert CR.allowed(masks[set_of[i]])[ids[i]].all(), i
    # the test bites
    _, plain = eng.parseq_logits(crops)
    differ = sum(decode_ids(p) != decode_ids(g) for p, g in zip(np.asarray(plain).reshape(-1, 26), np.asarray(ids).reshape(-1, 26)))
    print(f"{which}: {differ} of 37 rows read differently from the unconstrained engine")
    assert differ >= 10, differ


# ------------------------------------------------------------------------------------------------- 3. the four places agree
def test_every_place_a_token_is_chosen_agrees_under_a_row_table(eng_x4):
    crops = CR.sweep_crops(21, 37)
    masks = _masks3()
    set_of = np.array([i % 3 for i in range(37)], np.int32)
    runs = {}
    try:
        for key in (None, "embed_fold", "argmax_fold", "ar_host_check"):
            if key:
                assert eng_x4.set_tuning(key, 0) == 0
            runs[key] = eng_x4.parseq_logits(crops, want_ar=True, set_of=set_of, sets=masks)
            if key:
                assert eng_x4.set_tuning(key, 10 if key == "ar_host_check" else 1) == 0
    finally:
        for key, v in (("embed_fold", 1), ("argmax_fold", 1), ("ar_host_check", 10)):
            eng_x4.set_tuning(key, v)
    base = runs[None]
    for key, r in runs.items():
        for x, y in zip(r, base):
            assert np.array_equal(x, y), key


# ------------------------------------------------------------------------------------------------- 4. region crops
def _quads12(h, w):
    """upright; tilted by 7, -30 and 45 degrees; one sticking out of each image edge (the last of them also tilted); a few more; degenerate tl == tr"""
    return np.stack([
        GR.region_from_rect(40, 50, 240, 110), GR.region_from_rect(w // 2, h // 2, w // 2 + 128, h // 2 + 32),
        GR.tilted_quad(w * 0.4, h * 0.3, 220, 50, 7), GR.tilted_quad(w * 0.6, h * 0.5, 260, 64, -30), GR.tilted_quad(w * 0.3, h * 0.7, 180, 40, 45),
        GR.region_from_rect(-30, 100, 150, 150), GR.region_from_rect(w - 100, 200, w + 60, 250), GR.region_from_rect(300, -20, 500, 40),
        GR.tilted_quad(w * 0.5, h - 5.0, 240, 60, 12), GR.tilted_quad(w * 0.5, h * 0.5, 2.0 * w, 2.0 * h, 3),          # the last: larger than the page
        GR.tilted_quad(123.25, 77.75, 91.5, 17.125, -3.3),
        np.array([200, 300, 200, 300, 330, 340, 190, 345], np.float32)])                                               # degenerate: tl == tr


def test_region_crops_equal_numpy(eng_x4, funsd):
    from tuatara_amd import synth
    for img in (funsd, synth.synthetic_page(7, 1024, 768)):
        h, w = img.shape[:2]
        quads = _quads12(h, w)
        assert len(quads) == 12 and all(GR.quad_ok(q) for q in quads)
        assert sum(not GR.inside(q, h, w) for q in quads) >= 5
        crops = eng_x4.pack_regions(img, quads)
        ref = GR.region_crops(img, quads)
        for i in range(12):
            assert np.array_equal(crops[i], ref[i]), i
    assert len(eng_x4.pack_regions(funsd, np.zeros((0, 8), np.float32))) == 0


# ------------------------------------------------------------------------------------------------- 5. round trip
def test_round_trip_of_a_pages_own_quads(weights):
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    img = np.load(os.path.join(GOLDEN, "rotated_text.npz"))["image"]
    eng = Engine(weights["dir"], crop_mode=CROP_RECTIFIED)
    try:
        page = eng.images_to_data([img], conf=True)[0]
        quads = page.quad.copy()
        kind1 = np.array([not (q[1] == q[3] and q[0] == q[6]) for q in quads])      # fmod(angle, 90) != 0: the quad is tilted
        assert kind1.sum() >= 5, int(kind1.sum())
        back = eng.read_regions(img, [{"quad": q} for q in quads])
        assert len(back) == len(quads)
        for k, (q, r) in enumerate(zip(quads, back)):
            assert np.asarray(r["quad"], np.float32).tobytes() == q.tobytes() and r["region"] == k and r["set"] == -1
            assert np.asarray(r["bbox"], np.float32).tobytes() == GR.region_bbox(q).tobytes()
            if kind1[k]:
                assert r["ids"] == page.ids[k].tolist() and r["text"] == page.texts[k], k
                assert np.asarray(r["prob"], np.float32).tobytes() == page.prob[k].tobytes(), k
                assert np.float32(r["conf"]).tobytes() == page.conf[k].tobytes(), k
        again = eng.images_to_data([img], conf=True)[0]                               # the page call is what it was
        assert again.ids.tobytes() == page.ids.tobytes() and again.conf.tobytes() == page.conf.tobytes() and again.quad.tobytes() == page.quad.tobytes()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------- 6. pages
CHARSETS = [(DIGITS, None), (None, "e"), ("abcdefghij", None)]


def _items_equal(a, b):
    return (a["text"] == b["text"] and a["ids"] == b["ids"] and a["bbox"] == b["bbox"] and a["quad"] == b["quad"] and a["set"] == b["set"]
            and np.float32(a["conf"]).tobytes() == np.float32(b["conf"]).tobytes() and np.asarray(a["prob"], np.float32).tobytes() == np.asarray(b["prob"], np.float32).tobytes())


def test_pages_and_callers_agree(eng_x4, weights, funsd, monkeypatch, tmp_path):
    from tuatara_amd import build as B
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer, charset_mask, charset_masks
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ALLOWLIST", "TUATARA_BLOCKLIST", "TUATARA_ORIENT", "TUATARA_LINES", "TUATARA_CHARS", "TUATARA_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    p0 = synth.synthetic_page(61, 768, 1024)                                          # 768 x 1024
    p1 = np.ascontiguousarray(funsd[100:600, 30:730])                                 # 500 x 700
    wide = np.ascontiguousarray(synth.synthetic_page(62, 300, 416))                   # 300 x 400 inside rows of 416 pixels
    p2, p3 = wide[:, :400], synth.synthetic_page(63, 200, 320)                         # p3 gets no region
    imgs = [p0, p1, np.ascontiguousarray(p2), p3]
    # 14 regions dealt unevenly over pages 0, 1, 2 (page 3: none), interleaved, three sets and -1
    deal = [0, 1, 0, 2, 0, 0, 1, 2, 0, 1, 0, 2, 0, 1]
    regions = []
    rng = np.random.default_rng(4)
    for i, pg in enumerate(deal):
        h, w = imgs[pg].shape[:2]
        r = {"page": pg, "set": (i % 4) - 1}
        if i % 3 == 0:
            x0, y0 = int(rng.integers(0, w - 140)), int(rng.integers(0, h - 40))
            r["rect"] = (x0, y0, x0 + int(rng.integers(60, 140)), y0 + int(rng.integers(16, 40)))
        else:
            r["quad"] = GR.tilted_quad(float(rng.uniform(80, w - 80)), float(rng.uniform(30, h - 30)), float(rng.uniform(60, 200)), float(rng.uniform(16, 44)),
                                       float(rng.uniform(-40, 40)))
        regions.append(r)
    masks = charset_masks(CHARSETS)
    before = eng_x4.images_to_data(imgs[:2], conf=True)
    bufs = [DeviceBuffer(a.nbytes) for a in (p0, p1, wide, p3)]
    assert np.array_equal(eng_x4.charset, CR.FULL)
    try:
        eng_x4.set_charset(UPPER)                                                     # what -1 means in this test
        own = charset_mask(UPPER)
        for b, a in zip(bufs, (p0, p1, wide, p3)):
            b.upload(a)
        pages = [(bufs[0], 768, 1024), (bufs[1], 500, 700, 0), (bufs[2], 300, 400, 416 * 3), (bufs[3], 200, 320)]
        dev = eng_x4.read_regions(pages, regions, CHARSETS)
        assert [len(p) for p in dev] == [7, 4, 3, 0]
        for pg, items in enumerate(dev):                                               # the caller's order and sets
            mine = [i for i, d in enumerate(deal) if d == pg]
            assert [it["region"] for it in items] == mine and [it["set"] for it in items] == [regions[i]["set"] for i in mine]
        # the host-image form, page by page
        for pg in range(4):
            local = [dict(r, page=0) for r in regions if r["page"] == pg]
            host = eng_x4.read_regions(imgs[pg], local, CHARSETS)
            assert len(host) == len(dev[pg]) and all(_items_equal(a, b) for a, b in zip(host, dev[pg])), pg
        # the stage calls: ttr_parseq_logits_sets(ttr_pack_regions(...)) and the decode on its logits
        from tuatara_amd.engine import region_quad
        for pg in range(3):
            mine = [r for r in regions if r["page"] == pg]
            quads = np.stack([region_quad(r["quad"] if "quad" in r else r["rect"]) for r in mine])
            set_of = [r["set"] for r in mine]
            crops = eng_x4.pack_regions(imgs[pg], quads)
            assert np.array_equal(crops, GR.region_crops(imgs[pg], quads))
            lg, ids = eng_x4.parseq_logits(crops, set_of=set_of, sets=masks)
            d_ids, d_prob, d_conf = eng_x4.logits_confidence(lg, set_of=set_of, sets=masks)
            for k, it in enumerate(dev[pg]):
                assert it["ids"] == ids[k].tolist() == d_ids[k].tolist(), (pg, k)
                assert np.asarray(it["prob"], np.float32).tobytes() == d_prob[k].tobytes() and np.float32(it["conf"]).tobytes() == d_conf[k:k + 1].tobytes(), (pg, k)
                assert np.asarray(it["quad"], np.float32).tobytes() == quads[k].tobytes() and np.asarray(it["bbox"], np.float32).tobytes() == GR.region_bbox(quads[k]).tobytes()
                assert CR.allowed(own if set_of[k] < 0 else masks[set_of[k]])[ids[k]].all()
        # all regions under one mask: the call under set_charset with that mask, bit for bit (and no table travels)
        same = eng_x4.read_regions(pages, [dict(r, set=0) for r in regions], CHARSETS)
        eng_x4.set_charset(DIGITS)
        under = eng_x4.read_regions(pages, [dict(r, set=-1) for r in regions])
        assert all(_items_equal(dict(a, set=-1), b) for pa, pb in zip(same, under) for a, b in zip(pa, pb)) and sum(len(p) for p in same) == 14
    finally:
        eng_x4.set_charset()
        for b in bufs:
            b.free()
    # pytuatara regions= (a region without lists reads under the call's lists) and ocr_cli --regions, against the ctypes engine
    for pg in range(3):
        local = [r for r in regions if r["page"] == pg]
        want = [it for it in dev[pg]]
        spec = []
        for r in local:
            d = {"quad": list(map(float, r["quad"]))} if "quad" in r else {"rect": r["rect"]}
            if r["set"] >= 0:
                if CHARSETS[r["set"]][0]:
                    d["allowlist"] = CHARSETS[r["set"]][0]
                if CHARSETS[r["set"]][1]:
                    d["blocklist"] = CHARSETS[r["set"]][1]
            spec.append(d)
        got = pytuatara.image_to_data(imgs[pg], weights["dir"], "o", conf=True, allowlist=UPPER, regions=spec)
        assert [g["region"] for g in got] == list(range(len(local)))
        for g, w_ in zip(got, want):
            assert g["text"] == w_["text"] and list(g["bbox"]) == w_["bbox"] and np.float32(g["conf"]).tobytes() == np.float32(w_["conf"]).tobytes()
            assert np.asarray(g["quad"], np.float32).ravel().tobytes() == np.asarray(w_["quad"], np.float32).tobytes()
    assert pytuatara.image_to_data(p3, weights["dir"], "o", regions=[]) == []
    png = os.path.join(DATA, "funsd_0001129658.png")
    bgr = np.ascontiguousarray(funsd[:, :, ::-1])                                     # the CLI feeds BGR
    cli_regions = [{"rect": (60, 40, 260, 80), "set": 0}, {"quad": GR.tilted_quad(400, 300, 220, 40, -5), "set": 1}, {"rect": (100, 500, 300, 540), "set": -1}]
    want = eng_x4.read_regions(bgr, cli_regions, [(DIGITS, None), ("abcdefghij", "e")])
    f = tmp_path / "regions.txt"
    q = cli_regions[1]["quad"]
    f.write_text("# three fields\n60 40 260 80 " + DIGITS + "\n" + " ".join(repr(float(v)) for v in q) + " abcdefghij e   # tilted\n100 500 300 540\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--regions", str(f), png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln.split("\t") for ln in out.stdout.splitlines()]
    assert len(lines) == 3
    for (bb, cf, text), g in zip(lines, want):
        assert np.array([float(v) for v in bb.split()], np.float32).tobytes() == np.asarray(g["bbox"], np.float32).tobytes()      # (9 significant digits: the float itself)
        assert text == g["text"] and np.float32(float(cf)).tobytes() == np.float32(g["conf"]).tobytes()
    # the detecting entry points are what they were
    after = eng_x4.images_to_data(imgs[:2], conf=True)
    for x, y in zip(before, after):
        assert x.texts == y.texts and x.ids.tobytes() == y.ids.tobytes() and x.bbox.tobytes() == y.bbox.tobytes() and x.prob.tobytes() == y.prob.tobytes() and x.conf.tobytes() == y.conf.tobytes()
    assert len(before[0]) > 0


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_engine_usable(eng_x4, weights, funsd):
    from tuatara_amd.engine import Comm, DeviceBuffer, Engine, EngineError
    good = [{"rect": (60, 40, 260, 80), "set": 0}, {"quad": GR.tilted_quad(400, 300, 220, 40, -5), "set": -1}]
    sets = [(DIGITS, None)]
    want = eng_x4.read_regions(funsd, good, sets)
    h, w = funsd.shape[:2]

    def still_good(eng=eng_x4):
        got = eng.read_regions(funsd, good, sets)
        assert len(got) == 2 and all(_items_equal(a, b) for a, b in zip(got, want))

    nan_quad = GR.region_from_rect(1, 2, 30, 40)
    nan_quad[3] = np.nan
    for bad, kw, what in (([{"quad": nan_quad}], {}, "region 0 has a coordinate that is not finite"),
                          (good + [{"quad": GR.region_from_rect(1, 2, 30, 40) + np.float32(40000)}], {}, "region 2 has a coordinate .* 32768"),
                          ([dict(good[0], page=1)], {}, "region 0 names page 1"), ([dict(good[0], page=-1)], {}, "names page -1"),
                          ([dict(good[0], set=1)], {}, "names set 1"), ([dict(good[0], set=-2)], {}, "names set -2"),
                          (good, {"charsets": [np.array([0x7FE, 0, 0], np.uint32)]}, "bit 0")):
        with pytest.raises(EngineError, match=what):
            eng_x4.read_regions(funsd, bad, kw.get("charsets", sets))
        still_good()
    with pytest.raises(EngineError, match="set 0: bit 0"):
        eng_x4.logits_confidence(np.zeros((1, 26, 95), np.float32), set_of=[0], sets=np.array([[0x7FE, 0, 0]], np.uint32))
    with pytest.raises(EngineError, match="names set 3"):
        eng_x4.parseq_logits(np.zeros((2, 32, 128, 3), np.uint8), set_of=[0, 3], sets=np.array([[1, 0, 0]], np.uint32))
    still_good()
    # while batches stream
    buf = DeviceBuffer(funsd.nbytes)
    buf.upload(funsd)
    try:
        eng_x4.stream_push(buf, 1, h, w)
        for call in (lambda: eng_x4.read_regions(funsd, good, sets), lambda: eng_x4.read_regions([(buf, h, w)], good, sets),
                     lambda: eng_x4.pack_regions(funsd, np.zeros((1, 8), np.float32)), lambda: eng_x4.parseq_logits(np.zeros((1, 32, 128, 3), np.uint8), set_of=[-1]),
                     lambda: eng_x4.logits_confidence(np.zeros((1, 26, 95), np.float32), set_of=[-1])):
            with pytest.raises(EngineError, match="in flight"):
                call()
    finally:
        while eng_x4.stream_flush():
            pass
        buf.free()
    still_good()
    # a communicator
    comm = Comm(eng_x4, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        with pytest.raises(EngineError, match="communicator"):
            eng_x4.read_regions(funsd, good, sets)
        comm.attach(False)
    finally:
        comm.close()
    still_good()
    # the layers that read the detector's boxes, and strict_crops
    for kw, what in (({"orient": 1}, "orient"), ({"lines": 1}, "lines"), ({"chars": 1}, "chars"), ({"lines": 1, "blocks": 1}, "lines")):
        eng = Engine(weights["dir"], **kw)
        try:
            with pytest.raises(EngineError, match="the engine has " + what):
                eng.read_regions(funsd, good, sets)
            assert len(eng.image_to_data(funsd)) > 0
        finally:
            eng.close()
    strict = Engine(weights["dir"], strict_crops=True)
    try:
        outside = [good[0], {"quad": GR.region_from_rect(w - 50, 10, w + 1, 40)}]
        with pytest.raises(EngineError, match="region 1 has a corner outside page 0"):
            strict.read_regions(funsd, outside, sets)
        edge = [good[0], {"quad": GR.region_from_rect(w - 50, 0, w, 40), "set": 0}]           # on the edge is inside
        got = strict.read_regions(funsd, edge, sets)
        assert len(got) == 2 and _items_equal(got[0], want[0])
        assert len(eng_x4.read_regions(funsd, outside, sets)) == 2                            # without strict_crops: the border is replicated
    finally:
        strict.close()


def test_bf16_takes_full_masks_and_refuses_a_restricting_one(eng_bf16, funsd):
    from tuatara_amd.engine import EngineError
    regions = [{"rect": (60, 40, 260, 80), "set": 0}, {"quad": GR.tilted_quad(400, 300, 220, 40, -5), "set": -1}, {"rect": (100, 500, 300, 540), "set": 1}]
    full = [(None, None), ("", "")]
    got = eng_bf16.read_regions(funsd, regions, full)
    assert [g["set"] for g in got] == [0, -1, 1] and len(got) == 3
    plain = eng_bf16.read_regions(funsd, [dict(r, set=-1) for r in regions])
    assert [g["ids"] for g in got] == [p["ids"] for p in plain]
    for sets in ([(DIGITS, None), (None, None)], [(None, None), (None, "|")]):
        with pytest.raises(EngineError, match="bf16"):
            eng_bf16.read_regions(funsd, regions, sets)
    with pytest.raises(EngineError, match="bf16"):
        eng_bf16.logits_confidence(np.zeros((1, 26, 95), np.float32), set_of=[0], sets=np.array([[0x7FF, 0, 0]], np.uint32))
    again = eng_bf16.read_regions(funsd, regions, full)
    assert [g["ids"] for g in again] == [g["ids"] for g in got]


# ------------------------------------------------------------------------------------------------- 8. more rows than one recogniser group
def test_a_call_of_4097_regions_equals_its_two_groups(eng_x4):
    """The recogniser takes more than 4096 rows in even groups (4097 = 2049 + 2048), and each group's row masks, alternatives and lexicon matches must
    start where its crops do.  A crop's outputs do not depend on its batch (test_x4_parseq_batch_invariance) and a group has the row count of the matching
    call of its own, so the one call equals the two calls on regions[:2049] and regions[2049:] bit for bit, row for row."""
    n, cut, classes = 4097, 2049, 1021                                          # 1021: prime, so the positions' cycle and the sets' meet in every combination
    rng = np.random.default_rng(97)
    img = rng.integers(0, 256, (96, 640, 3), dtype=np.uint8)
    regions = []
    for i in range(n):
        c = i % classes                                                          # the position class: regions c, c + 1021, ... share a rectangle, not a set
        x0, y0 = (c * 37) % 500, (c * 11) % 60
        regions.append({"rect": (x0, y0, x0 + 48 + c % 90, y0 + 14 + c % 21), "set": i % 4 - 1})
    charsets = [(DIGITS, None), (UPPER, None), ("abcdefghijklmnopqrstuvwxyz", None)]
    alphabets = [DIGITS, UPPER, "abcdefghijklmnopqrstuvwxyz", DIGITS + UPPER + "abcdefghijklmnopqrstuvwxyz"]
    words = sorted({"".join(rng.choice(list(alphabets[k % 4]), int(rng.integers(1, 9)))) for k in range(80)})[:64]
    assert len(words) >= 48
    eng_x4.set_alternatives(3)
    eng_x4.set_lexicon(words, 2)
    try:
        whole = eng_x4.read_regions(img, regions, charsets)
        halves = eng_x4.read_regions(img, regions[:cut], charsets) + eng_x4.read_regions(img, regions[cut:], charsets)
    finally:
        eng_x4.set_lexicon(None)
        eng_x4.set_alternatives(0)
    assert len(whole) == len(halves) == n
    for i, (a, b) in enumerate(zip(whole, halves)):
        assert a["ids"] == b["ids"] and a["text"] == b["text"] and a["set"] == b["set"] == i % 4 - 1, i
        for k in ("prob", "conf"):
            assert np.asarray(a[k], np.float32).tobytes() == np.asarray(b[k], np.float32).tobytes(), (i, k)
        for k in ("alt_ids", "alt_prob", "lex_idx", "lex_logp"):
            assert a[k].tobytes() == b[k].tobytes(), (i, k)
    # the test bites: the sets matter, and both side blocks hold something
    assert any(whole[c]["ids"] != whole[c + classes]["ids"] for c in range(classes))        # one rectangle, two sets, two readings
    assert whole[0]["alt_ids"].shape == (26, 3) and any((r["alt_ids"][:, 1:] >= 0).any() for r in whole)
    assert whole[0]["lex_idx"].shape == (2,) and any((r["lex_idx"] >= 0).any() for r in whole)
