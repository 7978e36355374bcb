"""CPU suite for mixed-size batches (DESIGN.md "Mixed-size batches"): the canvas rule that decides which pages may share a batch, against a
numpy-float32 restatement; the new C ABI is exported and bound; ttr_config.mixed_batches is validated.  No GPU compute here."""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from tuatara_amd import build, engine
    build.build_all()
    return engine.load()


def canvas_ref(h, w, canvas_size=1024, mag_ratio=1.0):
    """canvas_geometry (geometry.cpp) restated in numpy float32: -> (h32, w32, ratio, target_h, target_w)"""
    f = np.float32
    target = f(mag_ratio) * f(max(h, w))
    if target > f(canvas_size):
        target = f(canvas_size)
    ratio = f(target / f(max(h, w)))
    th, tw = int(f(h) * ratio), int(f(w) * ratio)
    up = lambda v: v + (32 - v % 32) if v % 32 else v
    return up(th), up(tw), ratio, th, tw


# (h, w) -> (H, W) at canvas 1024, and the ratio where it is exact
CANVAS_1024 = [((1000, 754), (1024, 768), None), ((1024, 768), (1024, 768), 1.0),
               ((206, 275), (224, 288), 1.0), ((200, 270), (224, 288), 1.0), ((193, 257), (224, 288), 1.0), ((224, 288), (224, 288), 1.0),
               ((2000, 1508), (1024, 800), None), ((1997, 1500), (1024, 800), None), ((2048, 1536), (1024, 768), 0.5)]
# the six sizes of the GPU suite at canvas 256: identity, the general fixed-point path, the exact 2 x 2 area path
CANVAS_256 = [((192, 256), 1.0), ((206, 275), 0.9309), ((300, 400), 0.64), ((297, 395), 0.6481), ((384, 512), 0.5), ((380, 509), 0.5029)]


def test_canvas_geometry_at_1024(lib):
    for (h, w), (H, W), ratio in CANVAS_1024:
        oh, ow, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_float()
        assert lib.ttr_canvas_geometry(None, h, w, ctypes.byref(oh), ctypes.byref(ow), ctypes.byref(r)) == 0     # no engine: the default config
        ref = canvas_ref(h, w)
        assert (oh.value, ow.value) == (H, W) == ref[:2], (h, w)
        assert np.float32(r.value) == ref[2], (h, w)
        if ratio is not None:
            assert r.value == ratio
    # 1000 x 754 is not enlarged (mag_ratio 1): ratio 1, padded to the canvas 1024 x 768 shares with the 1024 x 768 pages
    assert canvas_ref(1000, 754)[2:] == (1.0, 1000, 754)


def test_canvas_geometry_at_256(lib):
    from tuatara_amd import engine
    for (h, w), ratio in CANVAS_256:
        got = engine.canvas_geometry(h, w, 256, 1.0)
        ref = canvas_ref(h, w, 256)
        assert got[:2] == (192, 256) == ref[:2], (h, w)
        assert np.float32(got[2]) == ref[2] and abs(got[2] - ratio) < 5e-5, (h, w, got[2])
        assert got[3:] == ref[3:], (h, w)
    # the three resize paths: identity, exact 2 x 2 decimation, general
    assert engine.canvas_geometry(192, 256, 256)[2:] == (1.0, 192, 256)
    assert engine.canvas_geometry(384, 512, 256)[2:] == (0.5, 192, 256)
    g = engine.canvas_geometry(380, 509, 256)
    assert g[2] != 0.5 and 380 / g[3] != 2.0 and (g[3], g[4]) != (380, 509)


def test_canvas_geometry_refuses_what_the_engine_refuses(lib):
    H, W, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_float()
    assert lib.ttr_canvas_geometry(None, 0, 10, ctypes.byref(H), ctypes.byref(W), ctypes.byref(r)) == -1
    assert b"Error reading image" in lib.ttr_last_error()
    assert lib.ttr_canvas_geometry(None, 2, 3000, ctypes.byref(H), ctypes.byref(W), ctypes.byref(r)) == -1     # 2 * (1024 / 3000) < 1 row
    assert b"image too thin to resize" in lib.ttr_last_error()


def test_new_symbols_are_exported_and_bound(lib):
    from tuatara_amd import engine
    raw = ctypes.CDLL(engine.lib_path())
    bound = {n for n, _, _ in engine.SYMBOLS}
    for name in ("ttr_canvas_geometry", "ttr_pages_to_data_dev_v", "ttr_stream_push_v", "ttr_last_images_batches", "ttr_resize_canvas_batch",
                 "ttr_pack_crops_batch", "ttr_dbg_canvas_geometry"):
        assert hasattr(raw, name), name
        assert name in bound, name
    cfg = engine.Config()
    lib.ttr_config_default(ctypes.byref(cfg))
    assert cfg.mixed_batches == 0                                   # off by default
    assert engine.Config._fields_[-1][0] == "mixed_batches"         # appended last: every earlier field keeps its offset
    assert ctypes.sizeof(engine.Page) == 24
    hdr = open(os.path.join(ROOT, "include", "tuatara_hip.h")).read()
    assert hdr.index("int blocks;") < hdr.index("int mixed_batches;") < hdr.index("} ttr_config;")


def test_mixed_batches_must_be_0_or_1(lib, tmp_path):
    """the config is checked before anything touches a device: the message is the same with and without a GPU"""
    from tuatara_amd.engine import Engine, EngineError
    with pytest.raises(EngineError, match="mixed_batches must be 0 or 1"):
        Engine(str(tmp_path), mixed_batches=2)
    with pytest.raises(EngineError, match="mixed_batches must be 0 or 1"):
        Engine(str(tmp_path), mixed_batches=-1)
