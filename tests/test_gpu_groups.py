"""GPU suite: the f16x4 engine's launch groups at their boundary (DESIGN.md "Launch groups").  The default path runs CRAFT in groups of 16 pages of 1024 x 768
(its widest tensor: 1 610 612 736 bytes of the 2^31 - 1 that 32-bit buffer offsets address); with enc_chunk lifted the encoder runs one group of up to 2730 crops
(2560 crops: a hidden activation of 2 013 265 920 bytes; the default stays 1280 + 1280, profiles/groups.md).  Group size is scheduling only: every result must
equal, bit for bit, what the smaller groups of before give - the reference here is the engine itself under craft_group = 8 / enc_chunk = 1280, computed once per
module."""
import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

H, W = 1024, 768
ONE = 4096                           # enc_chunk that lifts the default cap of 1820 crops: the window alone decides


def _run(eng, ptr, n, h, w):
    """One batch through the engine -> (heat maps, [(bbox, ids, text) per word] per page, pages per CRAFT group)."""
    res = eng.pages_to_data_dev(ptr, n, h, w)
    heat = eng.last_heat(n, h, w)
    words = [[(tuple(x["bbox"]), tuple(int(v) for v in x["ids"]), x["text"]) for x in pg] for pg in res]
    return heat, words, eng.last_groups()[0]


@pytest.fixture(scope="module")
def big_pages():
    from tuatara_amd import synth
    return np.stack([synth.synthetic_page(300 + i, H, W, n_words=24) for i in range(21)])


@pytest.fixture(scope="module")
def crops(big_pages):
    """2740 crops of 32 x 128 cut from the pages on a grid (172 of the 192 windows of each page): 2560 and 2600 of them are one encoder group, all 2740 two."""
    t = big_pages[:16].reshape(16, H // 32, 32, W // 128, 128, 3).transpose(0, 1, 3, 2, 4, 5).reshape(16, 192, 32, 128, 3)
    return np.ascontiguousarray(t[:, :172].reshape(-1, 32, 128, 3)[:2740])


@pytest.fixture(scope="module")
def chunked(eng_x4, crops):
    """The recogniser under enc_chunk = 1280 (the encoder groups of before: 3 x 914 here), once: logits and ids of all 2740 crops."""
    try:
        eng_x4.set_tuning("enc_chunk", 1280)
        lg, ids = eng_x4.parseq_logits(crops)
        assert eng_x4.last_groups()[1] == 914
    finally:
        eng_x4.set_tuning("enc_chunk", 0)
    return lg, ids


def test_16_pages_in_one_group_equal_two_groups_of_8(eng_x4, big_pages):
    from tuatara_amd.engine import DeviceBuffer
    buf = DeviceBuffer(big_pages[:16].nbytes)
    buf.upload(big_pages[:16])
    try:
        heat16, words16, g16 = _run(eng_x4, buf, 16, H, W)
        eng_x4.set_tuning("craft_group", 8)
        heat8, words8, g8 = _run(eng_x4, buf, 16, H, W)
    finally:
        eng_x4.set_tuning("craft_group", 16)
        buf.free()
    assert (g16, g8) == (16, 8)
    assert sum(len(p) for p in words16) > 20 * 16
    assert np.isfinite(heat16).all() and float(np.abs(heat16).max()) > 0.1
    assert np.array_equal(heat16, heat8)
    assert words16 == words8


def test_21_pages_in_one_group_at_the_window(eng_x4, big_pages):
    """The largest group the key reaches: craft_group = 32 runs 21 pages of 1024 x 768 as ONE group, slice1.7 / slice1.10's tensors at 2 113 929 216 bytes, 33 MB
    below 2^31 - where an offset advanced past the last tile would wrap.  It must equal the default's 16 + 5."""
    from tuatara_amd.engine import DeviceBuffer
    buf = DeviceBuffer(big_pages.nbytes)
    buf.upload(big_pages)
    try:
        heat_d, words_d, g_d = _run(eng_x4, buf, 21, H, W)
        eng_x4.set_tuning("craft_group", 32)
        heat21, words21, g21 = _run(eng_x4, buf, 21, H, W)
    finally:
        eng_x4.set_tuning("craft_group", 16)
        buf.free()
    assert (g_d, g21) == (16, 21)
    assert np.isfinite(heat21).all() and sum(len(p) for p in words21) > 20 * 21
    assert np.array_equal(heat21, heat_d)
    assert words21 == words_d


@pytest.mark.parametrize("n,group", [(20, 16), (24, 8)])
def test_ragged_and_evened_groups_equal_single_pages(eng_x4, n, group):
    """20 small pages run as 16 + 4, 24 as 8 + 8 + 8: each must give what its pages give one by one."""
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    h, w = 256, 192
    pages = np.stack([synth.synthetic_page(500 + i, h, w, n_words=6, scale=1) for i in range(n)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    try:
        heat, words, g = _run(eng_x4, buf, n, h, w)
        assert g == group
        assert sum(len(p) for p in words) > n
        for i in range(n):
            h1, w1, _ = _run(eng_x4, buf.ptr + i * h * w * 3, 1, h, w)
            assert np.array_equal(h1[0], heat[i]), i
            assert w1[0] == words[i], i
    finally:
        buf.free()


def _recognise(eng, crops, enc_chunk):
    try:
        eng.set_tuning("enc_chunk", enc_chunk)
        lg, ids = eng.parseq_logits(crops)
        return lg, ids, eng.last_groups()[1]
    finally:
        eng.set_tuning("enc_chunk", 0)


def test_2560_crops_in_one_encoder_group(eng_x4, crops, chunked):
    lg, ids, g = _recognise(eng_x4, crops[:2560], ONE)
    assert g == 2560
    assert np.isfinite(lg).all() and float(np.abs(lg).max()) > 1.0
    assert np.array_equal(lg, chunked[0][:2560])
    assert np.array_equal(ids, chunked[1][:2560])
    for chunk in (1280, 0):                 # the chunked schedule on the same 2560 (2 x 1280: the benchmark's pass), by the key and by default
        lg2, ids2, g2 = _recognise(eng_x4, crops[:2560], chunk)
        assert g2 == 1280
        assert np.array_equal(lg, lg2) and np.array_equal(ids, ids2)


def test_2600_crops_equal_the_chunked_result(eng_x4, crops, chunked):
    """(2600 crops are still one group: 2730 fit the window.)"""
    lg, ids, g = _recognise(eng_x4, crops[:2600], ONE)
    assert g == 2600
    assert np.array_equal(lg, chunked[0][:2600])
    assert np.array_equal(ids, chunked[1][:2600])


def test_2730_crops_in_one_group_at_the_window(eng_x4, crops, chunked):
    """The largest encoder group: 2730 crops put the MLP hidden at 2 146 959 360 bytes, 0.5 MB below 2^31."""
    lg, ids, g = _recognise(eng_x4, crops[:2730], ONE)
    assert g == 2730
    assert np.array_equal(lg, chunked[0][:2730])
    assert np.array_equal(ids, chunked[1][:2730])


def test_2740_crops_in_two_even_groups(eng_x4, crops, chunked):
    """Past 2730 crops the hidden activation leaves the window: two even groups of 1370."""
    lg, ids, g = _recognise(eng_x4, crops, ONE)
    assert g == 1370
    assert np.array_equal(lg, chunked[0])
    assert np.array_equal(ids, chunked[1])


def test_22_pages_are_refused_before_anything_runs(eng_x4):
    """The detector's forward pass handed 22 pages of 1024 x 768 directly (no grouping in front of it): slice1.7's output would be 2 214 592 512 bytes.  The pass
    refuses in its own prelude, naming the layer, before its first kernel is enqueued (the canvas upload of the debug entry point is all that ran): the records
    of the pass before are still the engine's.  The layer launchers' own refusals of such a tensor (conv3p_check, gemm2_check) cannot be reached behind that prelude
    and are held on the host, at these shapes, by tests/test_groups_cpu.py::test_launchers_refuse_a_tensor_past_the_window."""
    from tuatara_amd.engine import EngineError
    _, recs = eng_x4.craft_taps(np.full((1, 64, 64, 3), 255, np.uint8))
    count = eng_x4.lib.ttr_dbg_craft_tap_count(eng_x4.h)
    assert count == len(recs) > 20
    with pytest.raises(EngineError, match=r"slice1\.7: 22 pages of 1024 x 768 .* past the 2 GiB window"):
        eng_x4.craft_taps(np.zeros((22, H, W, 3), np.uint8))
    assert eng_x4.lib.ttr_dbg_craft_tap_count(eng_x4.h) == count
