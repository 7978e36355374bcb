"""GPU suite for the side-block records of the opt-in page layers (tuatara_amd/csrc/engine.h: SideCopy): a layer arms its record for the batches it runs in and
the next batch of the slot disarms it.  One engine reads the synthetic form as three one-page batches per call - pipeline slots 0, 1, 0 - with a layer on, then
off, then on again: the third call equals the first field for field, and the call in between carries nothing of the layer.  Everything is exact."""
import numpy as np
import pytest

from tests.test_gpu_marks import SPOTS, _boxes_over

pytestmark = pytest.mark.gpu

TABLE_FIELDS = ("rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell", "cell_texts")
MARK_FIELDS = ("mark_recs", "item_mark")
ALT_FIELDS = ("alt_ids", "alt_prob")


@pytest.fixture(scope="module")
def eng(weights):
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED)
    assert e.set_tuning(b"images_batch", 1) == 0           # every page a batch of its own: three pages take slots 0, 1, 0
    yield e
    e.close()


@pytest.fixture(scope="module")
def form_synth():
    from tuatara_amd import synth
    return _boxes_over(synth.synthetic_page(3, 512, 640, n_words=24), SPOTS)


def _same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _assert_same(got, want, what):
    for f in type(want).__slots__:
        assert _same_value(getattr(got, f), getattr(want, f)), (what, f)


def _three(eng, page):
    """the page as three batches of one call; the three results agree with each other"""
    res = eng.images_to_data([page] * 3)
    assert eng.last_images_batches() == [1, 1, 1] and len(res[0]) >= 8
    for k in (1, 2):
        _assert_same(res[k], res[0], f"slot {k & 1}")
    return res[0]


def test_tables_and_marks_on_off_on(eng, form_synth):
    def both(on):
        eng.set_tables((48, 128) if on else False)
        eng.set_marks(on)
    try:
        both(True)
        first = _three(eng, form_synth)
        assert first.table_mode != 0 and first.rulings is not None and first.mark_mode == 1 and len(first.mark_recs) == 6 and first.item_mark.shape == (len(first),)
        both(False)
        off = _three(eng, form_synth)
        assert off.table_mode == 0 and off.mark_mode == 0 and off.tables == [] and off.marks == []
        for f in TABLE_FIELDS + MARK_FIELDS:
            assert getattr(off, f) is None, f
        assert list(off.texts) == list(first.texts) and np.array_equal(off.ids, first.ids) and np.array_equal(off.quad, first.quad)
        both(True)
        _assert_same(_three(eng, form_synth), first, "on again")
    finally:
        both(False)


def test_alternatives_on_off_on(eng, form_synth):
    try:
        eng.set_alternatives(2)
        first = _three(eng, form_synth)
        assert first.alt_ids.shape == (len(first), 26, 2) and np.array_equal(first.alt_ids[:, :, 0], first.ids)
        eng.set_alternatives(0)
        off = _three(eng, form_synth)
        for f in ALT_FIELDS:
            assert getattr(off, f) is None, f
        assert list(off.texts) == list(first.texts) and np.array_equal(off.ids, first.ids)
        eng.set_alternatives(2)
        _assert_same(_three(eng, form_synth), first, "on again")
    finally:
        eng.set_alternatives(0)
