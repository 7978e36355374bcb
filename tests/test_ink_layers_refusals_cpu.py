"""The refusals of the host entry points of the layers that read ink - ttr_{tables,marks,barcodes,deskew}_from_page and their _ink forms - word for word: a bad
image, a bad layer argument, a bad ink argument, a bad quad, and - the _ink forms - a bad layer argument together with a bad ink argument (the layer's check
fires first, with 128 in the place of the ink).  The strings are literals: the entry points share their checks, and a shared check must not change a text."""
import numpy as np
import pytest

from tuatara_amd import engine as E

IMG = np.full((40, 50, 3), 255, np.uint8)
QUAD = np.array([[1, 1, 9, 1, 9, 9, 1, 9]], np.float32)
BAD_QUAD = np.array([[1, 1, np.inf, 1, 9, 9, 1, 9]], np.float32)
BAD_LOCAL = (65, 38, 2)
INK_TEXT = "radius must lie in 1..64, drop in 1..255 and polarity in 0..2, got 65, 38 and 2"
QUAD_TEXT = "quad 0 has a coordinate that is not finite or has |x| >= 32768"

# layer -> (the fixed form's call (image, quads, layer argument, ink, row_stride), the local form's (..., local_ink, ...), a bad layer argument, its text with
# {ink} where the ink stands)
LAYERS = {
    "tables": (lambda im, q, a, ink, rs: E.tables_from_page(im, q, a, ink, rs), lambda im, q, a, li, rs: E.tables_from_page_ink(im, q, a, li, rs), 48, 5,
               "min_len must lie in 16..4096 and ink in 1..255, got {arg} and {ink}"),
    "marks": (lambda im, q, a, ink, rs: E.marks_from_page(im, q, a, 64, 24, ink, rs), lambda im, q, a, li, rs: E.marks_from_page_ink(im, q, a, 64, 24, li, rs), 10, 5,
              "min_side must lie in 8..64, max_side in min_side..128, fill and ink in 1..255, got {arg}, 64, 24 and {ink}"),
    "barcodes": (lambda im, q, a, ink, rs: E.barcodes_from_page(im, q, a, ink, 3, rs), lambda im, q, a, li, rs: E.barcodes_from_page_ink(im, q, a, 3, li, rs), 8, 2,
                 "min_lines must lie in 4..256, ink in 1..255 and symbologies in 1..3, got {arg}, {ink} and 3"),
    "deskew": (lambda im, q, a, ink, rs: E.deskew_from_page(im, a, 288, ink, rs), lambda im, q, a, li, rs: E.deskew_from_page_ink(im, a, 288, li, rs), 64, 200,
               "max_slope must lie in 1..128, gain in 256..65535 and ink in 1..255, got {arg}, 288 and {ink}"),
}


def _refused(call, text):
    with pytest.raises(E.EngineError) as ex:
        call()
    assert str(ex.value) == text
    assert E.load().ttr_last_error().decode("latin1") == text


@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_the_fixed_forms(layer):
    fixed, _, good, bad, text = LAYERS[layer]
    what = f"ttr_{layer}_from_page: "
    assert fixed(IMG, QUAD, good, 128, 0) is not None
    _refused(lambda: fixed(IMG, QUAD, good, 128, 1), what + "bad image size")
    _refused(lambda: fixed(IMG, QUAD, bad, 128, 0), what + text.format(arg=bad, ink=128))
    _refused(lambda: fixed(IMG, QUAD, good, 0, 0), what + text.format(arg=good, ink=0))
    _refused(lambda: fixed(IMG, QUAD, good, 256, 1), what + "bad image size")                    # the image before the layer's ranges
    if layer != "deskew":
        _refused(lambda: fixed(IMG, BAD_QUAD, good, 128, 0), what + QUAD_TEXT)
        _refused(lambda: fixed(IMG, BAD_QUAD, bad, 128, 0), what + text.format(arg=bad, ink=128))   # the layer's ranges before the quads


@pytest.mark.parametrize("layer", sorted(LAYERS))
def test_the_local_forms(layer):
    _, local, good, bad, text = LAYERS[layer]
    what = f"ttr_{layer}_from_page_ink: "
    assert local(IMG, QUAD, good, True, 0) is not None
    _refused(lambda: local(IMG, QUAD, good, True, 1), what + "bad image size")
    _refused(lambda: local(IMG, QUAD, bad, True, 0), what + text.format(arg=bad, ink=128))
    _refused(lambda: local(IMG, QUAD, good, BAD_LOCAL, 0), what + INK_TEXT)
    _refused(lambda: local(IMG, QUAD, good, False, 0), what + "radius must lie in 1..64, drop in 1..255 and polarity in 0..2, got 0, 38 and 2")
    _refused(lambda: local(IMG, QUAD, bad, BAD_LOCAL, 0), what + text.format(arg=bad, ink=128))  # the layer first, the ink rule second
    if layer != "deskew":
        _refused(lambda: local(IMG, BAD_QUAD, good, True, 0), what + QUAD_TEXT)
        _refused(lambda: local(IMG, BAD_QUAD, good, BAD_LOCAL, 0), what + QUAD_TEXT)             # the quads before the ink rule
