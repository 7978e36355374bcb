"""-m gpu: history invariance of the f16x4 engine - a call's result must not depend on what the same engine ran earlier.

Every device buffer of the engine is a grow-only DevBuf that the next call, of whatever shape, runs in again; kernels pad in registers and read ragged tails; two
float buffers are written once per capacity instead of per call (the unpacked detector head's zero padding channels, the decoder's K/V cache).  A read of memory
the call did not write gives plausible numbers, so no float64 bar sees it: here every stage is compared BIT FOR BIT (raw bytes; no tolerance anywhere) with its
clean answer - the result on a newly created engine whose scratch buffers were zeroed (poison_scratch(0)) -

  poison tests   after ttr_dbg_poison_scratch filled every scratch buffer, to its full capacity, with quiet NaNs (pattern 1) and with large finite values
                 (pattern 2: fmaxf, comparisons and masked selects swallow a NaN);
  history tests  on a second engine after a real history: large before small, B = 3 before B = 1, all-255 before all-0, unpacked / packed / unpacked head
                 layouts, streamed batches on both workspace sets, a flood map before a sparse one, 128 long words before five, K = 8 before K = 2, ...;
  the control    with the two write-once buffers poisoned as well, the detector's 96 x 160 heat map must DIFFER: the poison reaches memory the kernels read.

Each probe is first held to run-to-run identity on its clean engine.  Engines are the module's own (the session fixtures of conftest.py carry the history of
whatever file ran before).  Clean engines are shared where that cannot hide anything: the integer stages and the decode stages on one engine, the detector on one
fresh engine per canvas size (a canvas size fixes the head tensors' layout, so nothing a probe leaves behind can sit where another probe's padding is), the
recogniser on one fresh engine per model and one more per probe that follows a larger batch on the long-word model (the K/V cache is the one buffer whose
history the engine keeps on purpose).  Before every probe on a shared clean engine its scratch buffers are zeroed again.  profiles/history.md has the wall times."""
import time

import numpy as np
import pytest

from tests import parity_rules as R

pytestmark = pytest.mark.gpu

TIMES = []            # (what, seconds): engine constructions and clean-answer fixtures, printed with the last test


def _engine(wdir, **kw):
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    t0 = time.perf_counter()
    e = Engine(wdir, "f16x4", **kw)
    e.poison_scratch(0)
    TIMES.append((f"Engine({', '.join(f'{k}={v}' for k, v in kw.items())})", time.perf_counter() - t0))
    return e


def same(a, b) -> bool:
    """equality of raw outputs: arrays by dtype, shape and bytes (a NaN equals only the same NaN); containers member by member; everything else by =="""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) == type(b) and a == b


def page_fields(pr):
    """every field of a PageResult (no field of it is a time)"""
    return {k: getattr(pr, k) for k in type(pr).__slots__ if k != "lex_words"}


def assert_same(got, clean, what):
    if isinstance(clean, dict) and isinstance(got, dict):
        bad = [k for k in clean if k not in got or not same(got[k], clean[k])]
        assert not bad and got.keys() == clean.keys(), f"{what}: fields that differ from the clean answer: {bad}"
    else:
        if isinstance(clean, np.ndarray) and isinstance(got, np.ndarray) and clean.shape == got.shape and clean.dtype.kind == "f":
            d = np.flatnonzero(clean.ravel().view(np.uint32) != got.ravel().view(np.uint32))
            assert d.size == 0, f"{what}: {d.size} of {clean.size} values differ from the clean answer, first at {np.unravel_index(d[0], clean.shape)}: {got.ravel()[d[0]]!r} against {clean.ravel()[d[0]]!r}"
        assert same(got, clean), f"{what}: differs from the clean answer"


def twice(f, what):
    """the probe's clean answer, behind its run-to-run identity on the clean engine"""
    a, b = f(), f()
    assert_same(b, a, f"{what}: second run on the clean engine")
    return a


# ------------------------------------------------------------------ inputs
CANVASES = [(32, 32), (64, 96), (96, 160), (64, 128)]       # 96 x 160: unpacked head (W / 2 no multiple of 32); 64 x 128: packed; 32 x 32: one 16 x 16 map


def canvas(h, w, B, fill, seed=0):
    if fill == "random":
        return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    return np.full((B, h, w, 3), {"255": 255, "0": 0}[fill], np.uint8)


def flood_map():
    """tests/test_gpu_post.py: a noise-only link map floods the page into one component"""
    from tests.golden.make_golden import synthetic_heatmap
    return np.stack([synthetic_heatmap(3)[..., 0], np.random.default_rng(0).normal(0, 0.01, (256, 192)).astype(np.float32)], -1)


def ramp_map():
    ramp = np.zeros((64, 64, 2), np.float32)
    ramp[..., 0] = np.linspace(0, 0.2, 64)[None, :]
    ramp[..., 1] = np.linspace(0, 0.1, 64)[:, None]
    return ramp


def dots_map(n, H=256, W=192):
    """n separate 4 x 4 blobs on a grid: n candidates"""
    t = np.zeros((H, W), np.float32)
    per_row = W // 8
    for i in range(n):
        y, x = 2 + 8 * (i // per_row), 2 + 8 * (i % per_row)
        t[y:y + 4, x:x + 4] = 1.0
    heat = np.stack([t, np.zeros_like(t)], -1)
    heat[0, 0, 1] = 1.0
    return heat


def post_maps():
    from tests.golden.make_golden import synthetic_heatmap
    return {"synthetic0": synthetic_heatmap(0), "flood": flood_map(), "sparse": synthetic_heatmap(5, 128, 96), "ramp": ramp_map(),
            "256x192": synthetic_heatmap(7, 256, 192), "96x112": synthetic_heatmap(123, 96, 112), "dots600": dots_map(600), "dots3": dots_map(3)}


def small_page(funsd):
    """a 206 x 275 window of the FUNSD page: of a few fixed windows the one with the most ink"""
    wins = [funsd[y:y + 206, x:x + 275] for y, x in ((0, 0), (100, 200), (300, 100), (500, 300), (700, 150))]
    return np.ascontiguousarray(max(wins, key=lambda w: int((w < 128).sum())))


def noise_crops(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 32, 128, 3), dtype=np.uint8)


def lexicon_words(n, seed=2):
    rng = np.random.default_rng(seed)
    return ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 9)))) for _ in range(n)]


# ------------------------------------------------------------------ engines and clean answers
@pytest.fixture(scope="module")
def wdir(weights):
    return weights["dir"]


@pytest.fixture(scope="module")
def clean(wdir):
    """the shared clean engine of the integer, decode and recogniser stages"""
    e = _engine(wdir)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hist(wdir):
    """the engine that is poisoned and given histories"""
    e = _engine(wdir)
    yield e
    e.close()


@pytest.fixture(scope="module")
def det_clean(wdir):
    """the detector's clean heat maps, one fresh engine per canvas size: {(h, w, B, fill): heat [B, h/2, w/2, 2]}"""
    t0 = time.perf_counter()
    out = {}
    for h, w in CANVASES + [(128, 160)]:
        e = _engine(wdir)
        try:
            for B in (1, 3):
                for fill in ("random", "255", "0"):
                    e.poison_scratch(0)
                    out[(h, w, B, fill)] = twice(lambda: e.craft_taps(canvas(h, w, B, fill))[0], f"detector {h} x {w}, B = {B}, {fill}")
        finally:
            e.close()
    TIMES.append(("det_clean (5 engines, 30 probes x 2)", time.perf_counter() - t0))
    return out


def heat_of(e, h, w, B, fill):
    return e.craft_taps(canvas(h, w, B, fill))[0]


@pytest.fixture(scope="module")
def post_clean(clean, funsd):
    t0 = time.perf_counter()
    out = {}
    for name, hm in post_maps().items():
        clean.poison_scratch(0)
        out["ccl " + name] = twice(lambda: clean.ccl_boxes(hm), "ccl_boxes " + name)
    img = np.random.default_rng(33 * 7 + 700).integers(0, 256, (33, 700, 3), dtype=np.uint8)
    clean.poison_scratch(0)
    out["resize"] = twice(lambda: clean.resize_canvas(img), "resize_canvas 33 x 700")
    rects = np.array([[50, 40, 60, 20, 0], [100, 75, 16, 6, -90], [198, 10, 30, 30, 30]], np.float32)
    page = np.random.default_rng(3).integers(0, 256, (300, 420, 3), dtype=np.uint8)
    clean.poison_scratch(0)
    out["pack"] = twice(lambda: clean.pack_crops(page, rects, 1.0), "pack_crops")
    clean.poison_scratch(0)
    out["pack_rect"] = twice(lambda: clean.pack_crops_rectified(page, rects, 1.0), "pack_crops_rectified")
    out["_inputs"] = (img, page, rects)
    assert len(out["ccl flood"]) == 1 and len(out["ccl ramp"]) <= 1 and len(out["ccl dots600"]) == 600 and len(out["ccl dots3"]) == 3
    TIMES.append(("post_clean", time.perf_counter() - t0))
    return out


@pytest.fixture(scope="module")
def rec_clean(clean):
    """the default model's clean recogniser answers: parseq_logits(want_ar) at N = 1, 3, 5 (decoder rows 26, 78, 130 against 128-row panels) and the decode
    stages on the N = 5 logits"""
    t0 = time.perf_counter()
    out = {}
    crops = noise_crops(5)
    for n in (1, 3, 5):
        clean.poison_scratch(0)
        out[f"parseq {n}"] = twice(lambda: clean.parseq_logits(crops[:n], want_ar=True), f"parseq_logits N = {n}")
    logits = out["parseq 5"][0]
    clean.poison_scratch(0)
    out["conf"] = twice(lambda: clean.logits_confidence(logits), "logits_confidence")
    for k in (2, 8):
        clean.poison_scratch(0)
        out[f"alts {k}"] = twice(lambda: clean.logits_alternatives(logits, k), f"logits_alternatives k = {k}")
    clean.set_lexicon(lexicon_words(5), 1)
    clean.poison_scratch(0)
    out["lex 5"] = twice(lambda: clean.logits_lexicon(logits), "logits_lexicon V = 5, M = 1")
    clean.set_lexicon(None)
    out["_crops"], out["_logits"] = crops, logits
    TIMES.append(("rec_clean", time.perf_counter() - t0))
    return out


# ------------------------------------------------------------------ the hook itself
def test_poison_fills_allocated_scratch_and_refuses_while_streaming(hist):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    hist.craft_taps(canvas(64, 96, 1, "random"))
    a = hist.poison_scratch(1)
    hist.parseq_logits(noise_crops(2))
    b = hist.poison_scratch(2)
    assert 0 < a < b                                            # the recogniser's workspaces joined the detector's
    with pytest.raises(EngineError, match="pattern must be"):
        hist.poison_scratch(3)
    buf = DeviceBuffer(64 * 96 * 3)
    buf.upload(canvas(64, 96, 1, "255"))
    assert hist.stream_push(buf, 1, 64, 96) == []
    with pytest.raises(EngineError, match="streamed batches are in flight"):
        hist.poison_scratch(1)
    assert len(hist.stream_flush()) == 1 and hist.stream_flush() == []
    buf.free()


# ------------------------------------------------------------------ poison tests
@pytest.mark.parametrize("pattern", [1, 2])
@pytest.mark.parametrize("hw", CANVASES)
def test_detector_after_poison(hist, det_clean, hw, pattern):
    h, w = hw
    for B in (1, 3):
        for fill in ("random", "255"):
            hist.poison_scratch(pattern)
            assert_same(heat_of(hist, h, w, B, fill), det_clean[(h, w, B, fill)], f"detector {h} x {w}, B = {B}, {fill} after poison {pattern}")


@pytest.mark.parametrize("pattern", [1, 2])
def test_integer_stages_after_poison(hist, post_clean, pattern):
    img, page, rects = post_clean["_inputs"]
    maps = post_maps()
    for name, f in [("resize", lambda: hist.resize_canvas(img)), ("ccl synthetic0", lambda: hist.ccl_boxes(maps["synthetic0"])),
                    ("ccl flood", lambda: hist.ccl_boxes(maps["flood"])), ("pack", lambda: hist.pack_crops(page, rects, 1.0)),
                    ("pack_rect", lambda: hist.pack_crops_rectified(page, rects, 1.0))]:
        hist.poison_scratch(pattern)
        assert_same(f(), post_clean[name], f"{name} after poison {pattern}")


@pytest.mark.parametrize("pattern", [1, 2])
def test_recogniser_and_decode_stages_after_poison(hist, rec_clean, pattern):
    crops, logits = rec_clean["_crops"], rec_clean["_logits"]
    for n in (1, 3, 5):
        hist.poison_scratch(pattern)
        assert_same(hist.parseq_logits(crops[:n], want_ar=True), rec_clean[f"parseq {n}"], f"parseq_logits N = {n} after poison {pattern}")
    hist.poison_scratch(pattern)
    assert_same(hist.logits_confidence(logits), rec_clean["conf"], f"logits_confidence after poison {pattern}")
    hist.poison_scratch(pattern)
    assert_same(hist.logits_alternatives(logits, 2), rec_clean["alts 2"], f"logits_alternatives after poison {pattern}")
    hist.set_lexicon(lexicon_words(5), 1)
    try:
        hist.poison_scratch(pattern)
        assert_same(hist.logits_lexicon(logits), rec_clean["lex 5"], f"logits_lexicon after poison {pattern}")
    finally:
        hist.set_lexicon(None)


@pytest.fixture(scope="module")
def page_clean(clean, funsd):
    page = small_page(funsd)
    clean.poison_scratch(0)
    got = twice(lambda: clean.image_to_data(page, conf=True), "image_to_data 206 x 275")
    print(f"image_to_data 206 x 275: {len(got)} words")
    return page, got


@pytest.mark.parametrize("pattern", [1, 2])
def test_image_to_data_after_poison(hist, page_clean, pattern):
    page, want = page_clean
    hist.poison_scratch(pattern)
    assert_same(hist.image_to_data(page, conf=True), want, f"image_to_data after poison {pattern}")


# ------------------------------------------------------------------ history tests: detector
def test_detector_large_then_small(hist, det_clean):
    heat_of(hist, 128, 256, 3, "255")
    assert_same(heat_of(hist, 64, 96, 1, "random"), det_clean[(64, 96, 1, "random")], "64 x 96 behind three all-255 pages of 128 x 256")


def test_detector_small_large_small(hist, det_clean):
    for h, w in ((32, 32), (128, 256), (32, 32), (96, 160), (128, 160), (96, 160)):
        heat = heat_of(hist, h, w, 1, "random")
        if (h, w) != (128, 256):                                # (the large page in between is history only)
            assert_same(heat, det_clean[(h, w, 1, "random")], f"{h} x {w} in small / large / small")


def test_detector_three_pages_then_one(hist, det_clean):
    for h, w in CANVASES:
        assert_same(heat_of(hist, h, w, 3, "random"), det_clean[(h, w, 3, "random")], f"{h} x {w}, B = 3")
        assert_same(heat_of(hist, h, w, 1, "random"), det_clean[(h, w, 1, "random")], f"{h} x {w}, B = 1 behind B = 3")


def test_detector_white_then_black(hist, det_clean):
    for h, w in CANVASES:
        heat_of(hist, h, w, 3, "255")
        assert_same(heat_of(hist, h, w, 1, "0"), det_clean[(h, w, 1, "0")], f"{h} x {w}: all-0 behind all-255")
        assert_same(heat_of(hist, h, w, 3, "0"), det_clean[(h, w, 3, "0")], f"{h} x {w}: three all-0 pages behind all-255")


def test_detector_unpacked_packed_unpacked(hist, det_clean):
    """128 x 160 (unpacked head), 64 x 128 (packed), 96 x 160 (unpacked, in buffers at least as large as it needs: no capacity change re-zeroes them)"""
    assert_same(heat_of(hist, 128, 160, 3, "random"), det_clean[(128, 160, 3, "random")], "128 x 160 (unpacked)")
    assert_same(heat_of(hist, 64, 128, 3, "255"), det_clean[(64, 128, 3, "255")], "64 x 128 (packed) behind it")
    assert_same(heat_of(hist, 96, 160, 1, "random"), det_clean[(96, 160, 1, "random")], "96 x 160 (unpacked) behind both")
    assert_same(heat_of(hist, 96, 160, 3, "255"), det_clean[(96, 160, 3, "255")], "96 x 160, B = 3, all-255 behind all three")
    # the same change of layout with NaNs in what the packed page leaves behind: stale finite values in the padding channels meet zero weights and move no
    # heat map (the bug tests/test_gpu_craft_layers.py once found looked like that), NaNs do
    for h, w, B in ((64, 128, 3), (96, 160, 1), (64, 128, 1), (32, 32, 1), (64, 96, 3)):
        assert_same(heat_of(hist, h, w, B, "random"), det_clean[(h, w, B, "random")], f"{h} x {w}, B = {B} across a change of layout")
        hist.poison_scratch(1)


def test_detector_after_streamed_batches_on_both_workspace_sets(wdir, det_clean):
    """three streamed batches of three pages in launch groups of one page on two detector lanes: the groups alternate between the two workspace sets; then the
    same small page lands on set 0 again, and - a batch of two groups - on both"""
    from tuatara_amd.engine import DeviceBuffer
    c = _engine(wdir, craft_group=1)                           # the clean answer of the page path: the same launch groups, one lane, nothing before them
    try:
        buf = DeviceBuffer(3 * 64 * 96 * 3)
        buf.upload(canvas(64, 96, 3, "random"))

        def pages_heat():
            c.pages_to_data_dev(buf, 3, 64, 96)
            return c.last_heat(3, 64, 96)
        want_pages = twice(pages_heat, "three 64 x 96 pages, one per launch group")
        buf.free()
    finally:
        c.close()
    e = _engine(wdir, craft_lanes=2, craft_group=1)
    try:
        bufs = []
        for j, (h, w, fill) in enumerate([(128, 160, "255"), (64, 96, "255"), (64, 96, "random")]):
            buf = DeviceBuffer(3 * h * w * 3)
            buf.upload(canvas(h, w, 3, fill))
            bufs.append(buf)
            e.stream_push(buf, 3, h, w)
        while e.stream_flush():
            pass
        assert_same(heat_of(e, 64, 96, 1, "random"), det_clean[(64, 96, 1, "random")], "64 x 96 behind three streamed batches")
        e.pages_to_data_dev(bufs[2], 3, 64, 96)                 # one page per group: pages 0 and 2 on set 0, page 1 on set 1
        assert_same(e.last_heat(3, 64, 96), want_pages, "three 64 x 96 pages, one per launch group, on alternating workspace sets")
        for b in bufs:
            b.free()
    finally:
        e.close()


# ------------------------------------------------------------------ history tests: post-processing
def test_ccl_histories(hist, post_clean):
    maps = post_maps()
    for chain in (("flood", "sparse", "ramp"), ("256x192", "96x112"), ("dots600", "dots3"), ("flood", "dots3", "synthetic0")):
        for name in chain:
            assert_same(hist.ccl_boxes(maps[name]), post_clean["ccl " + name], f"ccl_boxes {name} in {' -> '.join(chain)}")
    assert hist.set_tuning("gpu_calipers", 2) == 0              # the hulls' pool too small: the host's calipers read rows_packed
    try:
        for name in ("flood", "sparse", "dots3"):
            assert_same(hist.ccl_boxes(maps[name]), post_clean["ccl " + name], f"ccl_boxes {name} on the host-calipers path behind a flood map")
    finally:
        hist.set_tuning("gpu_calipers", 1)


# ------------------------------------------------------------------ history tests: recogniser
@pytest.fixture(scope="module")
def long_dir(tmp_path_factory):
    from tuatara_amd import weights as W
    d = str(tmp_path_factory.mktemp("weights_long_history"))
    W.make_synthetic_weights(d, seed=0, structured=True, max_len=30)
    return d


def first_eos(ids):
    ids = np.asarray(ids).reshape(-1, 26)
    return np.where((ids == 0).any(1), (ids == 0).argmax(1), 26)


@pytest.mark.parametrize("exits", [1, 0])
def test_long_words_then_few(long_dir, exits):
    """128 long-word crops write all 26 K/V slots of every row, 17 of them with no EOS; then 5 of them alone, and the 5 crops whose words end first: refined
    logits, AR logits and ids against fresh engines that never saw the 128.  exits = 0: the same with ar_crop_exit / ar_early_exit off."""
    kw = {} if exits else dict(ar_crop_exit=0, ar_early_exit=0)
    crops = R.long_word_crops()
    e = _engine(long_dir, **kw)
    try:
        full = twice(lambda: e.parseq_logits(crops, want_ar=True), "128 long-word crops")
        eos = first_eos(full[2])
        assert (eos == 26).sum() >= 8 and eos.min() <= 1          # words that never end, and words that end at once
        late = np.argsort(-eos, kind="stable")[:5]
        early = np.argsort(eos, kind="stable")[:5]
        assert int((np.abs(full[1]).max((0, 2)) > 0).sum()) == 26  # the loop ran to its last step
        for name, sel in (("the 5 longest", late), ("the 5 that end first", early)):
            f = _engine(long_dir, **kw)
            try:
                want = twice(lambda: f.parseq_logits(crops[sel], want_ar=True), f"{name} on a fresh engine")
            finally:
                f.close()
            assert_same(e.parseq_logits(crops[sel], want_ar=True), want, f"{name} behind the 128 (exits = {exits})")
            e.parseq_logits(crops, want_ar=True)                    # the 128 again in front of the next five
    finally:
        e.close()


def test_recogniser_large_then_small(hist, rec_clean):
    crops = rec_clean["_crops"]
    big = hist.parseq_logits(noise_crops(300, seed=9))
    assert big[0].shape == (300, 26, 95)
    assert_same(hist.parseq_logits(crops[:3], want_ar=True), rec_clean["parseq 3"], "N = 3 behind N = 300")
    assert hist.set_tuning("enc_chunk", 2) == 0
    try:
        assert_same(hist.parseq_logits(crops, want_ar=True), rec_clean["parseq 5"], "N = 5 in encoder groups of 2")
    finally:
        hist.set_tuning("enc_chunk", 0)
    assert_same(hist.parseq_logits(crops, want_ar=True), rec_clean["parseq 5"], "N = 5 in one group behind groups of 2")
    assert_same(hist.parseq_logits(crops[:1], want_ar=True), rec_clean["parseq 1"], "N = 1 behind N = 5")


def test_decode_stages_large_then_small(hist, rec_clean):
    logits = rec_clean["_logits"]
    many = np.random.default_rng(4).normal(0, 3, (200, 26, 95)).astype(np.float32)
    hist.logits_alternatives(many, 8)
    assert_same(hist.logits_alternatives(logits, 8), rec_clean["alts 8"], "alternatives K = 8 behind 200 rows")
    assert_same(hist.logits_alternatives(logits, 2), rec_clean["alts 2"], "alternatives K = 2 behind K = 8")
    hist.logits_confidence(many)
    assert_same(hist.logits_confidence(logits), rec_clean["conf"], "logits_confidence behind 200 rows")
    hist.set_lexicon(lexicon_words(5000, seed=7), 8)
    try:
        idx, _ = hist.logits_lexicon(many)
        assert idx.shape == (200, 8)
        hist.set_lexicon(lexicon_words(5), 1)
        assert_same(hist.logits_lexicon(logits), rec_clean["lex 5"], "lexicon V = 5, M = 1 behind V = 5000, M = 8")
    finally:
        hist.set_lexicon(None)


# ------------------------------------------------------------------ history tests: pages
LAYERS = dict(crop_mode=1, mixed_batches=1, lines=1, blocks=1, chars=1, tables=True, deskew=True, alts=3)


def pages_dev(e, imgs):
    from tuatara_amd.engine import DeviceBuffer
    h, w = imgs[0].shape[:2]
    buf = DeviceBuffer(len(imgs) * h * w * 3)
    buf.upload(np.stack(imgs))
    try:
        return [page_fields(p) for p in e.pages_to_data_dev(buf, len(imgs), h, w, conf=True)]
    finally:
        buf.free()


def test_layered_pages_large_then_small(wdir, funsd):
    """conf, lines, blocks, chars, tables, deskew and alternatives on: the FUNSD page, then a 206 x 275 page, against a clean engine configured alike - every
    field of the result"""
    small = small_page(funsd)
    c = _engine(wdir, **LAYERS)
    try:
        want = twice(lambda: pages_dev(c, [small]), "layered 206 x 275 page")
    finally:
        c.close()
    e = _engine(wdir, **LAYERS)
    try:
        big = pages_dev(e, [funsd])
        assert len(big[0]["texts"]) > len(want[0]["texts"]) >= 1
        got = pages_dev(e, [small])
        for k in want[0]:
            assert same(got[0][k], want[0][k]), f"layered 206 x 275 page behind the FUNSD page: field {k} differs from the clean answer"
        for pattern in (1, 2):
            e.poison_scratch(pattern)
            assert_same(pages_dev(e, [small])[0], want[0], f"layered 206 x 275 page after poison {pattern}")
    finally:
        e.close()


def streamed_single(e, buf, h, w):
    """one batch of one page through stream_push and the flushes that empty the pipeline -> its pages' fields"""
    got = [e.stream_push(buf, 1, h, w, conf=True)]
    while True:
        r = e.stream_flush(conf=True)
        if not r:
            break
        got.append(r)
    return [page_fields(p) for p in got[-1]]


def test_mixed_batch_tiled_page_and_streams_then_a_single_page(wdir, funsd):
    """one engine (mixed batches, canvas 256): a mixed-size batch, a tiled page, streamed batches of 1, 2 and 3 in front of the probe batch - then the single
    small page each time, against a clean engine configured alike"""
    from tuatara_amd.engine import DeviceBuffer
    small = small_page(funsd)
    kw = dict(mixed_batches=1, canvas_size=256)
    c = _engine(wdir, **kw)
    try:
        want = twice(lambda: [page_fields(p) for p in c.images_to_data([small], conf=True)], "single page through images_to_data")
        want_dev = twice(lambda: pages_dev(c, [small]), "single page through pages_to_data_dev")
        h, w = small.shape[:2]
        probe = DeviceBuffer(h * w * 3)
        probe.upload(small)
        want_stream = twice(lambda: streamed_single(c, probe, h, w), "single page through stream_push")
        assert len(want_stream) == 1 and len(want_stream[0]["texts"]) >= 1
    finally:
        c.close()
    e = _engine(wdir, **kw)
    try:
        mixed = [np.ascontiguousarray(funsd[:250, :250]), np.ascontiguousarray(funsd[100:340, 200:456]), np.ascontiguousarray(funsd[:256, :230])]
        assert len(e.images_to_data(mixed, conf=True)) == 3
        assert_same([page_fields(p) for p in e.images_to_data([small], conf=True)], want, "single page behind a mixed-size batch")
        e.set_tiled(64)
        tiled = e.images_to_data([np.ascontiguousarray(funsd[:448, :640])], conf=True)
        assert tiled[0].tiles > 1
        e.set_tiled(False)
        assert_same([page_fields(p) for p in e.images_to_data([small], conf=True)], want, "single page behind a tiled page")
        assert_same(pages_dev(e, [small]), want_dev, "single page (device) behind a tiled page")
        other = DeviceBuffer(3 * h * w * 3)
        other.upload(np.stack([np.ascontiguousarray(funsd[y:y + h, x:x + w]) for y, x in ((0, 0), (400, 300), (600, 100))]))
        for before in (1, 2, 3):                                 # the probe batch lands on slot parity `before` % 2
            for j in range(before):
                e.stream_push(other, 3 - (j % 2), h, w)
            assert_same(streamed_single(e, probe, h, w), want_stream, f"streamed single page behind {before} streamed batches")
        probe.free()
        other.free()
    finally:
        e.close()


# ------------------------------------------------------------------ the positive control
def test_control_poisoned_padding_channels_change_the_heat_map(wdir, det_clean):
    """with the write-once buffers poisoned too, the unpacked head reads NaN padding channels: the 96 x 160 heat map must differ from the clean one, or the
    poison reaches nothing the kernels read (the detector only: no CCL runs on this map)"""
    from tuatara_amd.engine import EngineError
    e = _engine(wdir, range_guard=0)                             # (the guard would refuse the NaNs by name: the control wants them to reach the heat map)
    try:
        assert_same(heat_of(e, 96, 160, 1, "random"), det_clean[(96, 160, 1, "random")], "the throw-away engine before the poison")
        e.poison_scratch(1, also_kept_once=True)
        try:
            heat = heat_of(e, 96, 160, 1, "random")
        except EngineError:
            heat = None
        assert heat is None or not same(heat, det_clean[(96, 160, 1, "random")]), "poisoned padding channels left the heat map unchanged: they are never read"
    finally:
        e.close()


def test_wall_times_of_the_shared_parts():
    for what, s in TIMES:
        print(f"history: {what}: {s:.2f} s")
