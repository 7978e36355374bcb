"""-m gpu: mixed-size batches (DESIGN.md "Mixed-size batches") - pages of different sizes and row strides that share one detector canvas travel
as one batch.  The table kernels against their uniform twins byte for byte (resize_pad_pages_kernel, pack_crops_pages_kernel,
pack_crops_rect_pages_kernel through the stage calls), then every entry point: the list form with ttr_config.mixed_batches = 1, the device
entry points ttr_pages_to_data_dev_v / ttr_stream_push_v, strided windows, the opt-ins, failures, the flag off, pytuatara.  The bar throughout:
a page's result is its single-image call's."""
import math
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_images import _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# six sizes that share the 192 x 256 canvas of an engine with canvas_size = 256 (tests/test_mixed_cpu.py): identity, general, general, general,
# the exact 2 x 2 area path, general - with the FUNSD window each is cut from (y, x)
SIZES_256 = [(192, 256, 60, 40), (206, 275, 300, 200), (300, 400, 80, 60), (297, 395, 420, 300), (384, 512, 100, 120), (380, 509, 560, 200)]
# heat-map rects (cx, cy, w, h, angle) on the 96 x 128 map of that canvas: axis-aligned, tilted, leaving the image (clamped), empty after the clamp
RECTS = np.array([[40, 30, 30, 10, 0], [60, 50, 36, 9, 17], [125, 90, 20, 12, 0], [200, 150, 10, 6, 0]], np.float32)


def _engine(weights, **kw):
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    return Engine(weights["dir"], **kw)


@pytest.fixture(scope="module")
def eng_mixed(weights):
    return _engine(weights, mixed_batches=1)


@pytest.fixture(scope="module")
def eng256(weights):
    return _engine(weights, canvas_size=256, mixed_batches=1)


@pytest.fixture(scope="module")
def pages256(funsd):
    """the six sizes as windows of FUNSD; page 3 stays a row-strided view into the page, the others are copied out"""
    out = []
    for k, (h, w, y, x) in enumerate(SIZES_256):
        v = funsd[y:y + h, x:x + w]
        out.append(v if k == 3 else np.ascontiguousarray(v))
    assert out[3].strides[0] == funsd.shape[1] * 3
    return out


@pytest.fixture(scope="module")
def pages7(funsd):
    """two canvases at the default canvas_size: four pages on 1024 x 768 (FUNSD 1000 x 754, its 180 degree turn, two synthetic 1024 x 768) and three
    FUNSD crops of 206 x 275, 200 x 270 and 193 x 257 on 224 x 288, interleaved"""
    from tuatara_amd import synth
    f = funsd
    big = [f, np.ascontiguousarray(f[::-1, ::-1]), synth.synthetic_page(200, 1024, 768, n_words=22), synth.synthetic_page(201, 1024, 768, n_words=22)]
    small = [np.ascontiguousarray(f[300:506, 200:475]), np.ascontiguousarray(f[500:700, 100:370]), np.ascontiguousarray(f[40:233, 300:557])]
    return [small[0], big[0], big[2], small[1], big[1], small[2], big[3]]


def _single(eng, image):
    """ttr_image_to_data's raw result (for Engine._quads, and for _take_many's PageResult, which keeps every array)"""
    import ctypes as C
    from tuatara_amd.engine import _u8
    image = np.ascontiguousarray(image, dtype=np.uint8)
    arr = (C.c_void_p * 1)()
    eng._check(eng.lib.ttr_image_to_data(eng.h, _u8(image), image.shape[0], image.shape[1], image.shape[1] * 3, arr))
    return arr


def _with_quads(eng, arr, n):
    """n raw results -> (their pages with conf, their quads f32 [count, 8] per page)"""
    quads = [eng._quads(arr[i], eng.lib.ttr_result_count(arr[i])) for i in range(n)]
    return [list(m) for m in eng._take_many(arr, n, True)], quads


def _list_with_quads(eng, pages):
    import ctypes as C
    from tuatara_amd.engine import _host_images
    ptrs, hs, ws, st, keep = _host_images(pages)
    out = (C.c_void_p * len(keep))()
    assert eng.lib.ttr_images_to_data(eng.h, ptrs, hs, ws, st, len(keep), out) == 0, eng.lib.ttr_last_error()
    return _with_quads(eng, out, len(keep))


@pytest.fixture(scope="module")
def singles7(eng_mixed, pages7):
    return [_with_quads(eng_mixed, _single(eng_mixed, p), 1)[0][0] for p in pages7]


@pytest.fixture(scope="module")
def single_quads7(eng_mixed, pages7):
    return [_with_quads(eng_mixed, _single(eng_mixed, p), 1)[1][0] for p in pages7]


def _equal(a, b):
    """text and bbox (test_gpu_images._same) and ids"""
    return _same(a, b) and [x["ids"] for x in a] == [x["ids"] for x in b]


def _conf_close(a, b):
    """conf between entry points that form different batches (DESIGN.md "Recognition confidence", "Batch composition"): the refined logits move by
    at most 1.1e-5 with the batch's composition, a position's log-probability then by at most twice that, and conf is a product of at
    most 27 probabilities: |d log conf| <= 27 * 2 * 1.1e-5"""
    return all(abs(math.log(x["conf"]) - math.log(y["conf"])) <= 27 * 2 * 1.1e-5 for x, y in zip(a, b))


# ---------------------------------------------------------------- 1, 2: the table kernels, byte for byte
def test_canvas_bytes_equal_the_uniform_kernel(eng256, pages256):
    for order in (list(range(6)), list(range(5, -1, -1))):
        pages = [pages256[k] for k in order]
        assert {eng256.canvas_geometry(*p.shape[:2])[:2] for p in pages} == {(192, 256)}
        canv, ratios = eng256.resize_canvas_batch(pages)
        assert canv.shape == (6, 192, 256, 3)
        for k, p in enumerate(pages):
            one, ratio = eng256.resize_canvas(p)
            assert np.array_equal(canv[k], one), f"page {order[k]} {p.shape}"            # padding included
            assert np.float32(ratios[k]) == np.float32(ratio) == np.float32(eng256.canvas_geometry(*p.shape[:2])[2])
    th, tw = int(380 * ratios[0]), int(509 * ratios[0])                                   # (the reversed order's first page: the zero padding exists)
    assert (th, tw) != (192, 256) and not canv[0, th:].any() and not canv[0, :, tw:].any() and canv[0, :th, :tw].any()


@pytest.mark.parametrize("crop_mode", [0, 1])
@pytest.mark.parametrize("turn", [0, 1])
def test_crop_bytes_equal_the_uniform_kernels(eng256, pages256, crop_mode, turn):
    n_pages, n_rects = len(pages256), len(RECTS)
    # rect-major order: consecutive crops come from different pages
    rects = np.concatenate([RECTS for _ in range(n_pages)]).reshape(n_pages, n_rects, 5).transpose(1, 0, 2).reshape(-1, 5)
    page_of = np.tile(np.arange(n_pages, dtype=np.int32), n_rects)
    crops, quads = eng256.pack_crops_batch(pages256, rects, page_of, crop_mode, turn)
    for pg, p in enumerate(pages256):
        ratio = eng256.canvas_geometry(*p.shape[:2])[2]
        c1, q1 = eng256.pack_crops_oriented(np.ascontiguousarray(p), RECTS, ratio, crop_mode, turn)
        sel = np.nonzero(page_of == pg)[0]
        assert np.array_equal(crops[sel], c1), f"page {pg} {p.shape}"
        assert np.array_equal(quads[sel], q1), f"page {pg} {p.shape}"
        assert c1[0].any() and c1[1].any() and c1[2].any() and not c1[3].any()            # three real crops, the fourth empty after the clamp
    from tuatara_amd.engine import EngineError
    with pytest.raises(EngineError, match="page_of"):
        eng256.pack_crops_batch(pages256, RECTS, [0, 1, 6, 0], crop_mode, turn)


# ---------------------------------------------------------------- 3, 8: the list form
def test_list_batches_by_canvas_and_equals_the_single_calls(eng_mixed, eng_x4, pages7, singles7, single_quads7):
    got, quads = _list_with_quads(eng_mixed, pages7)
    assert eng_mixed.last_images_batches() == [4, 3]                                     # two canvases: 1024 x 768 first, then 224 x 288
    assert len(got) == len(pages7)
    for i, (g, s) in enumerate(zip(got, singles7)):
        assert _same(g, s), f"image {i} {pages7[i].shape}"
        assert np.array_equal(quads[i], single_quads7[i]), f"image {i}: quad"
    assert sum(len(g) for g in got) > 150
    # the same list on an engine without the flag: five sizes, five batches
    eng_x4.images_to_data(pages7, keep=False)
    assert len(eng_x4.last_images_batches()) == 5 and sorted(eng_x4.last_images_batches()) == [1, 1, 1, 2, 2]
    # small batches: every bucket cut at images_batch
    assert eng_mixed.set_tuning(b"images_batch", 2) == 0
    try:
        again = eng_mixed.images_to_data(pages7)
        assert eng_mixed.last_images_batches() == [2, 2, 2, 1]
    finally:
        eng_mixed.set_tuning(b"images_batch", 32)
    for g, s in zip(again, singles7):
        assert _same(g, s)
    assert _same(eng_mixed.image_to_data(pages7[1]), singles7[1])                        # nothing left in flight


def test_off_means_off(eng_x4, pages7):
    got = eng_x4.images_to_data(pages7)
    b = eng_x4.last_images_batches()
    assert sum(b) == 7 and len(b) == 5 and b[:2] == [2, 2]                               # size buckets, the 1024 x 768 canvases first
    for g, p in zip(got, pages7):
        assert _same(g, eng_x4.image_to_data(p))


# ---------------------------------------------------------------- 4: through the three resize paths
def test_list_through_the_resize_paths(eng256, pages256):
    singles = [eng256.image_to_data(np.ascontiguousarray(p)) for p in pages256]
    got = eng256.images_to_data(pages256)
    assert eng256.last_images_batches() == [6]
    for i, (g, s) in enumerate(zip(got, singles)):
        assert _equal(g, s), f"image {i} {pages256[i].shape}"
    counts = [len(s) for s in singles]
    assert sum(counts) > 0
    assert counts[0] > 0 and counts[4] > 0 and max(counts[1], counts[2], counts[3], counts[5]) > 0, counts   # identity, 2 x 2 area, general


# ---------------------------------------------------------------- 5: the device entry points
def test_device_entry_points(eng_mixed, funsd, pages7):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    small = [pages7[0], pages7[3], pages7[5]]                                            # 206 x 275, 200 x 270, 193 x 257: one canvas
    singles = [eng_mixed.image_to_data(p, conf=True) for p in small]
    assert all(len(s) > 0 for s in singles)
    bufs, pages = [], []
    for k, p in enumerate(small):
        h, w = p.shape[:2]
        stride = w * 3 + (13 if k == 1 else 0)                                           # page 1: a padded row stride
        host = np.full((h, stride), 0xAB, np.uint8)
        host[:, :w * 3] = p.reshape(h, w * 3)
        b = DeviceBuffer(host.nbytes)
        b.upload(host)
        bufs.append(b)
        pages.append((b, h, w, stride if k == 1 else 0))
    got = eng_mixed.pages_to_data_dev_v(pages, conf=True)
    for g, s in zip(got, singles):
        assert _equal(g, s) and _conf_close(g, s)
    # a window into the middle of a larger device image
    big = DeviceBuffer(funsd.nbytes)
    big.upload(funsd)
    y, x, h, w = 300, 200, 206, 275
    window = [(big.ptr + (y * funsd.shape[1] + x) * 3, h, w, funsd.shape[1] * 3)]
    win = eng_mixed.pages_to_data_dev_v(window, conf=True)
    assert [list(m) for m in win] == [eng_mixed.image_to_data(np.ascontiguousarray(funsd[y:y + h, x:x + w]), conf=True)] and len(win[0]) > 0
    # streamed, interleaved with a uniform batch: every batch equals its synchronous result
    two = np.stack([pages7[2], pages7[6]])                                               # two 1024 x 768 pages
    ub = DeviceBuffer(two.nbytes)
    ub.upload(two)
    sync = [eng_mixed.pages_to_data_dev_v(pages, conf=True), eng_mixed.pages_to_data_dev(ub, 2, 1024, 768, conf=True), win,
            eng_mixed.pages_to_data_dev_v(pages[::-1], conf=True)]
    streamed = []
    for push in (lambda: eng_mixed.stream_push_v(pages, conf=True), lambda: eng_mixed.stream_push(ub, 2, 1024, 768, conf=True),
                 lambda: eng_mixed.stream_push_v(window, conf=True), lambda: eng_mixed.stream_push_v(pages[::-1], conf=True)):
        r = push()
        if r:
            streamed.append(r)
    while True:
        r = eng_mixed.stream_flush(conf=True)
        if not r:
            break
        streamed.append(r)
    assert len(streamed) == 4
    for k, (a, b) in enumerate(zip(streamed, sync)):
        assert [list(m) for m in a] == [list(m) for m in b], f"batch {k}"
    # two canvases in one batch: refused, naming the page and both canvases; the engine works afterwards
    with pytest.raises(EngineError, match=r"page 1 \(1024 x 768\) has canvas 1024 x 768, page 0 \(206 x 275\) has canvas 224 x 288"):
        eng_mixed.pages_to_data_dev_v([pages[0], (ub, 1024, 768, 0)])
    with pytest.raises(EngineError, match="Error reading image"):
        eng_mixed.pages_to_data_dev_v([pages[0], (bufs[1], 200, 270, 100)])              # a stride shorter than a row
    with pytest.raises(EngineError, match="mixed-size batch: page 1"):
        eng_mixed.stream_push_v([pages[0], (ub, 1024, 768, 0)])
    assert eng_mixed.stream_flush() == []                                                # the refused push left nothing in flight
    again = eng_mixed.pages_to_data_dev_v(pages, conf=True)
    assert [list(m) for m in again] == [list(m) for m in sync[0]]
    for b in bufs + [big, ub]:
        b.free()


# ---------------------------------------------------------------- 6: the opt-ins ride along
@pytest.mark.parametrize("name,cfg", [("rectified", dict(crop_mode=1)), ("flip", dict(orient=1)), ("blocks", dict(lines=1, blocks=1)), ("chars", dict(chars=1))])
def test_opt_ins_ride_along(weights, pages7, name, cfg):
    eng = _engine(weights, mixed_batches=1, **cfg)
    got = eng.images_to_data(pages7, conf=True)
    assert eng.last_images_batches() == [4, 3]
    total = 0
    for i, (g, p) in enumerate(zip(got, pages7)):
        s = eng._take_many(_single(eng, p), 1, True)[0]
        assert _equal(list(g), list(s)) and _conf_close(list(g), list(s)), f"{name}: image {i}"
        for key in ("quad", "orient", "line", "word", "order", "line_first", "line_bbox", "block", "line_block", "line_pos", "block_order", "block_first", "block_bbox",
                    "char_first", "char_quad", "char_bbox", "char_cuts", "char_mode", "char_profile"):
            a, b = getattr(g, key), getattr(s, key)
            assert (a is None) == (b is None), (name, key)
            if a is not None:
                assert np.array_equal(a, b), f"{name}: image {i}: {key}"
        assert (g.page_orient, g.block_mode) == (s.page_orient, s.block_mode)
        total += len(s)
    assert total > 150
    present = {"rectified": "quad", "flip": "orient", "blocks": "block_order", "chars": "char_quad"}[name]
    assert getattr(got[1], present) is not None and len(getattr(got[1], present)) > 0


# ---------------------------------------------------------------- 7: failures stay alone
def test_failures_stay_alone(eng_mixed, pages7, singles7):
    from tuatara_amd.engine import EngineError
    with pytest.raises(EngineError, match="3 dimensions"):                               # (the wrapper's check, as without the flag)
        eng_mixed.images_to_data([pages7[0], np.zeros((10, 10), np.uint8), pages7[3]])
    thin = np.full((2, 3000, 3), 255, np.uint8)                                          # 2 rows * (1024 / 3000) < 1 row
    got = eng_mixed.images_to_data([pages7[0], thin, pages7[3], pages7[1]])
    assert eng_mixed.last_images_batches() == [1, 2]                                     # the thin image never reached a bucket
    msg = eng_mixed.last_images_error
    assert msg and "1 of 4 images failed (indices 1)" in msg and "image too thin to resize" in msg, msg
    assert got[1] == []
    assert _same(got[0], singles7[0]) and _same(got[2], singles7[3]) and _same(got[3], singles7[1])
    # an unreadable entry (NULL) between canvas-mates, through the C ABI
    import ctypes as C
    a, b = pages7[0], pages7[3]
    ptrs = (C.c_void_p * 3)(a.ctypes.data, None, b.ctypes.data)
    hs, ws = (C.c_int32 * 3)(a.shape[0], 206, b.shape[0]), (C.c_int32 * 3)(a.shape[1], 275, b.shape[1])
    out = (C.c_void_p * 3)()
    rc = eng_mixed.lib.ttr_images_to_data(eng_mixed.h, ptrs, hs, ws, None, 3, out)
    msg = eng_mixed.lib.ttr_last_error().decode()
    assert rc == 1 and "1 of 3 images failed (indices 1)" in msg and "Error reading image" in msg, (rc, msg)
    res = eng_mixed._take_many(out, 3)
    assert _same(res[0], singles7[0]) and res[1] == [] and _same(res[2], singles7[3])
    assert eng_mixed.last_images_batches() == [2]


# ---------------------------------------------------------------- 9: pytuatara
def test_pytuatara_mixed_batches_keyword(weights, pages7, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    monkeypatch.delenv("TUATARA_PRECISION", raising=False)
    monkeypatch.delenv("TUATARA_MIXED_BATCHES", raising=False)
    pages = [pages7[0], pages7[3], np.ascontiguousarray(pages7[0][::-1, ::-1])]          # two sizes, one canvas
    plain = pytuatara.images_to_data(pages, weights["dir"], "../outputs")
    mixed = pytuatara.images_to_data(pages, weights["dir"], "../outputs", mixed_batches=True)
    assert len(mixed) == 3 and sum(len(m) for m in mixed) > 0
    for m, p in zip(mixed, plain):
        assert _same(m, p)
