"""GPU suite for the rectified crop mode (crop_mode = TTR_CROP_RECTIFIED; DESIGN.md "Rectified crops"): the packer
(post_ops.hip: pack_crops_rect_kernel) against the numpy restatement tests/rectify_ref.py bit for bit, the end-to-end path against
the CPU oracle, every entry point against the single-page call, and the default mode left as it is."""
import os
import sys

import numpy as np
import pytest

from tests import rectify_ref as R
from tests.conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng_rect(weights):
    """the default precision (f16x4) with rectified crops"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    return Engine(weights["dir"], crop_mode=CROP_RECTIFIED)


@pytest.fixture(scope="module")
def rotated_pages():
    from tuatara_amd import synth
    return [synth.synthetic_rotated_page(s, 512, 512, n_words=10, max_deg=30.0)[0] for s in (11, 12)]


@pytest.fixture(scope="module")
def rotated_text():
    return np.load(os.path.join(GOLDEN, "rotated_text.npz"))["image"]


def _check_crops(eng, img, rects, ratio):
    crops, quads = eng.pack_crops_rectified(img, rects, ratio)
    from oracle import post
    boxes = post.adjust_result_coordinates(rects, 1.0 / ratio, 1.0 / ratio)
    kinds = []
    for i, b in enumerate(boxes):
        ref, q, k = R.zero_or_crop(img, b)
        assert np.array_equal(crops[i], ref), (i, b, k)
        assert np.array_equal(quads[i], q), (i, b)
        kinds.append(k)
    return kinds


def test_pack_crops_rectified_equals_numpy(eng_rect, oracle_models, rotated_pages):
    from oracle import pipeline
    kinds = []
    # detected boxes of rotated pages
    for page in rotated_pages:
        d = pipeline.detect(oracle_models[0], page)
        assert len(d["det"]) >= 8
        kinds += _check_crops(eng_rect, page, d["det"], d["ratio"])
    # boxes touching every image edge (clamp), 1-px-thin boxes, on a colour page (heat-map units: x2 -> image pixels)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)
    rects = np.array([[0, 40, 40, 12, 20], [210, 75, 30, 10, -35], [100, 0, 50, 8, 12.5], [100, 150, 50, 8, -7], [0, 0, 30, 30, 45],
                      [210, 150, 25, 6, 60], [105, 75, 60, 0.5, 17], [105, 75, 0.5, 40, 3], [50, 100, 40, 0.5, 0], [80, 30, 20, 10, 90],
                      [150, 120, 70, 14, -80], [60, 60, 3, 2, 33]], np.float32)
    kinds += _check_crops(eng_rect, img, rects, 1.0)
    assert 0 in kinds and 1 in kinds
    # the mode of the engine does not matter to the stage entry point, and ttr_pack_crops is unchanged on axis-aligned boxes
    upright = rects[np.abs(np.fmod(rects[:, 4], 90.0)) == 0]
    c0, _ = eng_rect.pack_crops(img, upright, 1.0)
    c1, _ = eng_rect.pack_crops_rectified(img, upright, 1.0)
    assert np.array_equal(c0, c1)


def _end_to_end(eng0, eng1, oracle_models, img, min_skew=None):
    from oracle import pipeline, post
    got0, got1 = eng0.image_to_data(img), eng1.image_to_data(img)
    assert set(got0[0]) == {"text", "bbox", "ids"} and set(got1[0]) == {"text", "bbox", "ids", "quad"}
    assert np.array_equal(np.array([g["bbox"] for g in got1]), np.array([g["bbox"] for g in got0]))
    d = pipeline.detect(oracle_models[0], img)
    crops, quads, kinds, keep = R.crops(img, d["boxes"])
    assert len(keep) == len(got1)
    assert np.array_equal(np.array([g["bbox"] for g in got1]), np.array([post.tesseract_bbox(d["boxes"][i]) for i in keep]))
    assert np.array_equal(np.array([g["quad"] for g in got1], np.float32), quads)
    eng_crops, _ = eng1.pack_crops_rectified(img, d["det"][keep], d["ratio"])
    assert np.array_equal(eng_crops, crops)
    ref_logits = pipeline.parseq_logits(oracle_models[1], crops)
    lg, ids = eng1.parseq_logits(crops)
    assert float(np.abs(lg - ref_logits).max()) < 1e-3
    texts, ref_ids = post.decode_logits(ref_logits)
    assert [g["text"] for g in got1] == texts
    assert np.array_equal(np.array([g["ids"] for g in got1]), ref_ids)
    if min_skew is not None:
        assert max(abs(R.skew_degrees(q)) for q, k in zip(quads, kinds) if k == 1) >= min_skew
    return got0, got1


def test_end_to_end_rotated_pages(eng_x4, eng_rect, oracle_models, rotated_pages, rotated_text):
    _end_to_end(eng_x4, eng_rect, oracle_models, rotated_pages[0], min_skew=10.0)
    _end_to_end(eng_x4, eng_rect, oracle_models, rotated_text, min_skew=10.0)


def test_axis_aligned_items_unchanged_on_funsd(eng_x4, eng_rect, funsd, funsd_oracle):
    from oracle import post
    got0, got1 = eng_x4.image_to_data(funsd), eng_rect.image_to_data(funsd)
    keep = [b for b in funsd_oracle["boxes"] if post.crop_resize(funsd_oracle["swapped"], b, True) is not None]
    assert len(keep) == len(got0) == len(got1) > 20
    upright = 0
    for b, g0, g1 in zip(keep, got0, got1):
        assert g0["bbox"] == g1["bbox"]
        if R.deskew(b)[0] == 0:
            assert (g0["text"], g0["ids"]) == (g1["text"], g1["ids"])
            upright += 1
    assert upright > 20


def test_every_entry_point_equals_the_single_page_call(eng_rect, rotated_pages):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    small = synth.synthetic_rotated_page(13, 384, 448, n_words=6, max_deg=25.0)[0]
    pages = rotated_pages + [small]
    single = [eng_rect.image_to_data(p) for p in pages]
    assert all(len(s) > 0 for s in single)
    many = eng_rect.images_to_data(pages)                                 # mixed sizes
    assert [list(m) for m in many] == single
    buf = DeviceBuffer(2 * 512 * 512 * 3)
    buf.upload(np.stack(rotated_pages))
    assert [list(m) for m in eng_rect.pages_to_data_dev(buf, 2, 512, 512)] == single[:2]
    streamed = []
    for k in range(2):                                                      # one page per batch: the streamed pipeline's two slots
        streamed += eng_rect.stream_push(buf.ptr + k * 512 * 512 * 3, 1, 512, 512)
    while True:
        r = eng_rect.stream_flush()
        if not r:
            break
        streamed += r
    assert [list(m) for m in streamed] == single[:2]


def test_strict_crops_fail_alike(weights, rotated_pages):
    from tuatara_amd.engine import CROP_RECTIFIED, Engine, EngineError
    edge = rotated_pages[1].copy()
    edge[0:14, 0:80] = np.random.default_rng(0).integers(0, 2, (14, 80, 1), dtype=np.uint8) * 255   # ink on the border: the box leaves the image
    s0 = Engine(weights["dir"], strict_crops=True)
    s1 = Engine(weights["dir"], strict_crops=True, crop_mode=CROP_RECTIFIED)
    for e in (s0, s1):
        with pytest.raises(EngineError, match="leaves the image"):
            e.image_to_data(edge)
    a, b = s0.image_to_data(rotated_pages[1]), s1.image_to_data(rotated_pages[1])
    assert [g["bbox"] for g in a] == [g["bbox"] for g in b] and len(a) > 0
    s0.close(); s1.close()


def test_pytuatara_rectify_keyword(weights, rotated_pages, eng_rect, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    monkeypatch.delenv("TUATARA_PRECISION", raising=False)
    monkeypatch.delenv("TUATARA_CROP_MODE", raising=False)
    page = rotated_pages[0]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    rect = pytuatara.image_to_data(page, weights["dir"], "o", rectify=True)
    assert set(plain[0]) == {"text", "bbox"} and set(rect[0]) == {"text", "bbox", "quad"}
    want = eng_rect.image_to_data(page)
    assert [(r["text"], list(r["bbox"]), [list(p) for p in r["quad"]]) for r in rect] == [(g["text"], g["bbox"], g["quad"]) for g in want]
    many = pytuatara.images_to_data([page], weights["dir"], "o", rectify=True)
    assert many == [rect]
    with pytest.raises(TypeError):
        pytuatara.image_to_data(page, weights["dir"], "o", True)               # keyword-only
