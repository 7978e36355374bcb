"""GPU suite for the recognition confidence (DESIGN.md "Recognition confidence"): decode_conf_kernel against float64 on adversarial logits,
the engine's probabilities against the ones the reference computes and discards (the oracle's orc_softmax_argmax), every entry point -
multi-rank gathers and the sharded mode included - against the plain call on the same pages bit for bit, no change to what the engine returned before,
and the callers (pytuatara, ocr_cli --conf)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

CONF_KEYS = {"conf", "char_conf"}


@pytest.fixture(scope="module")
def eng_rect(weights):
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    return Engine(weights["dir"], crop_mode=CROP_RECTIFIED)


@pytest.fixture(scope="module")
def pages():
    from tuatara_amd import synth
    return [synth.synthetic_page(60 + i, 1024, 768, n_words=14 + 6 * i) for i in range(2)]


def _adversarial_logits(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    kind = rng.integers(0, 7, (n, 26))
    for i, p in zip(*np.nonzero(kind == 1)):                  # exact ties at the maximum: the first one wins
        t = rng.choice(95, rng.integers(2, 5), replace=False)
        x[i, p, t] = x[i, p].max() + 1.0
    for i, p in zip(*np.nonzero(kind == 2)):                  # all equal: prob = 1/95, id 0
        x[i, p] = np.float32(rng.normal())
    for i, p in zip(*np.nonzero(kind == 3)):                  # near one-hot
        x[i, p, rng.integers(0, 95)] += 40.0
    for i, p in zip(*np.nonzero(kind == 4)):                  # spreads up to +-1e30
        x[i, p] = rng.uniform(-1e30, 1e30, 95).astype(np.float32)
    for i, p in zip(*np.nonzero(kind == 5)):                  # an EOS (id 0) or a dropped id (88) at this position
        x[i, p, 0 if rng.random() < 0.5 else 88] += 12.0
    return x


def _softmax_max64(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return 1.0 / np.exp(x - m).sum(-1)


def test_kernel_against_float64(eng_x4):
    from tuatara_amd.engine import confidence_from_probs
    for n, seed in ((1, 1), (37, 2), (4100, 3)):
        x = _adversarial_logits(n, seed)
        ids, prob, conf = eng_x4.logits_confidence(x)
        assert np.array_equal(ids, np.argmax(x, -1)), n                      # numpy's argmax: the first maximal index
        p64 = _softmax_max64(x)
        rel = np.abs(prob.astype(np.float64) - p64) / p64
        print(f"n={n}: max relative |prob - float64| {rel.max():.2e}, rows with prob 1/95: {int((np.abs(p64 - 1 / 95) < 1e-12).sum())}")
        assert rel.max() <= 2e-6, n
        assert (prob > 0).all() and (prob <= 1).all()
        for i in range(n):
            _, c = confidence_from_probs(ids[i], prob[i])
            assert c.tobytes() == conf[i:i + 1].tobytes(), (n, i, c, conf[i])
    assert (ids == 0).any() and (ids == 88).any()


def _oracle_probs(logits):
    from oracle import post
    import ctypes as C
    logits = np.ascontiguousarray(logits, np.float32)
    N = len(logits)
    ids = np.zeros((N, 26), np.int64)
    probs = np.zeros((N, 26), np.float32)
    post.lib().orc_softmax_argmax(logits.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(N * 26), C.c_int(95),
                                  ids.ctypes.data_as(C.POINTER(C.c_int64)), probs.ctypes.data_as(C.POINTER(C.c_float)))
    return ids, probs


def _upto_eos(ids):
    e = np.where((ids == 0).any(-1), (ids == 0).argmax(-1), 25)
    return np.arange(26)[None, :] <= e[:, None]


def _parity(eng, res, crops, ref_logits):
    """the engine's prob / conf of one page (res: PageResult) against the oracle's discarded probabilities"""
    from tuatara_amd.engine import confidence_from_probs
    assert len(res) == len(crops) > 0
    lg, _ = eng.parseq_logits(crops)
    dx = np.abs(lg.astype(np.float64) - ref_logits).max(-1)                   # [N, 26]: max_c |dx_c| per position
    o_ids, o_prob = _oracle_probs(ref_logits)
    mask = _upto_eos(o_ids) & (res.ids == o_ids)
    dlog = np.abs(np.log(res.prob.astype(np.float64)) - np.log(o_prob.astype(np.float64)))
    assert mask.sum() > 0.9 * _upto_eos(o_ids).sum()
    assert (dlog[mask] <= 2 * dx[mask] + 4e-6).all(), float((dlog - 2 * dx)[mask].max())
    assert dlog[mask].max() < 2e-3
    words = 0
    for i in range(len(res)):
        if not np.array_equal(res.ids[i], o_ids[i]):
            continue
        _, oc = confidence_from_probs(o_ids[i], o_prob[i])
        assert abs(np.log(float(res.conf[i])) - np.log(float(oc))) <= 2e-3 * (len(res.texts[i]) + 1), i
        words += 1
    assert words > 0.9 * len(res)
    return float(dlog[mask].max()), words


def test_parity_with_the_references_discarded_probabilities(eng_x4, oracle_models, funsd, funsd_oracle, pages):
    from oracle import pipeline
    res = eng_x4.images_to_data([funsd], conf=True)[0]
    d, w = _parity(eng_x4, res, funsd_oracle["crops"], funsd_oracle["logits"])
    print(f"FUNSD: {w} words, max |dlog p| up to EOS {d:.2e}")
    for pg in pages:
        o = pipeline.image_to_data(*oracle_models, pg, debug=True)
        res = eng_x4.images_to_data([pg], conf=True)[0]
        d, w = _parity(eng_x4, res, o["crops"], o["logits"])
        print(f"synthetic page: {w} words, max |dlog p| up to EOS {d:.2e}")


def _check_items(items, res=None):
    from tuatara_amd.engine import confidence_from_probs
    for j, d in enumerate(items):
        assert len(d["char_conf"]) == len(d["text"]) and 0 < d["conf"] <= 1, d
        if res is not None:
            cc, c = confidence_from_probs(res.ids[j], res.prob[j])
            assert float(c) == d["conf"] and cc.tolist() == d["char_conf"]


def test_every_entry_point_equals_the_single_page_call(eng_x4, eng_rect, pages):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    small = synth.synthetic_page(71, 384, 448, n_words=6)
    for eng in (eng_x4, eng_rect):
        single = [eng.image_to_data(p, conf=True) for p in pages + [small]]
        assert all(len(s) > 0 for s in single)
        for s in single:
            _check_items(s)
        many = eng.images_to_data(pages + [small], conf=True)                   # mixed sizes
        assert [list(m) for m in many] == single
        for m in many:
            _check_items(list(m), m)
        buf = DeviceBuffer(2 * 1024 * 768 * 3)
        buf.upload(np.stack(pages))
        dev = eng.pages_to_data_dev(buf, 2, 1024, 768, conf=True)
        assert [list(m) for m in dev] == single[:2]
        streamed = []
        for k in range(2):                                                      # one page per batch: the streamed pipeline's two slots
            streamed += eng.stream_push(buf.ptr + k * 1024 * 768 * 3, 1, 1024, 768, conf=True)
        while True:
            r = eng.stream_flush(conf=True)
            if not r:
                break
            streamed += r
        assert [list(m) for m in streamed] == single[:2]
        buf.free()
    assert set(eng_rect.image_to_data(pages[0], conf=True)[0]) == {"text", "bbox", "ids", "quad"} | CONF_KEYS


def test_no_behaviour_change(eng_x4, funsd, pages):
    from tuatara_amd.engine import DeviceBuffer
    for img in [funsd] + pages:
        plain, withc = eng_x4.image_to_data(img), eng_x4.image_to_data(img, conf=True)
        assert len(plain) > 0 and all(set(d) == {"text", "bbox", "ids"} for d in plain)
        assert [{k: v for k, v in d.items() if k not in CONF_KEYS} for d in withc] == plain
        _check_items(withc)
    many = eng_x4.images_to_data(pages)
    assert all(set(d) == {"text", "bbox", "ids"} for m in many for d in m)
    buf = DeviceBuffer(2 * 1024 * 768 * 3)
    buf.upload(np.stack(pages))
    a, b = eng_x4.pages_to_data_dev(buf, 2, 1024, 768), eng_x4.pages_to_data_dev(buf, 2, 1024, 768, conf=True)
    assert all(set(d) == {"text", "bbox", "ids"} for m in a for d in m)
    for x, y in zip(a, b):
        assert np.array_equal(x.ids, y.ids) and np.array_equal(x.bbox, y.bbox) and x.texts == y.texts
        assert np.array_equal(x.conf, y.conf) and np.array_equal(x.prob, y.prob)
    buf.free()


@pytest.mark.parametrize("which", ["bf16", "f32"])
def test_other_precisions_are_self_consistent(which, eng_bf16, eng_f32, pages):
    eng = eng_bf16 if which == "bf16" else eng_f32
    for pg in pages:
        res = eng.images_to_data([pg], conf=True)[0]
        canvas, ratio = eng.resize_canvas(pg)
        crops, _ = eng.pack_crops(pg, eng.ccl_boxes(eng.craft_heatmap(canvas)), ratio)
        assert len(crops) == len(res) > 0
        lg, ids = eng.parseq_logits(crops)
        assert np.array_equal(ids, res.ids)
        rel = np.abs(res.prob.astype(np.float64) - _softmax_max64(lg)) / _softmax_max64(lg)
        print(f"{which}: {len(res)} words, max relative |prob - float64 softmax of its own logits| {rel.max():.2e}")
        assert rel.max() <= 2e-6
        _check_items(list(res), res)


# ------------------------------------------------------------------------------------------------- multi-rank (tests/test_gpu_dist.py's pattern)
WORLD1 = r'''
import sys
import numpy as np
sys.path.insert(0, {root!r})
from tuatara_amd import synth
from tuatara_amd.engine import Comm, DeviceBuffer, Engine
assert "torch" not in sys.modules
eng = Engine({wdir!r})
pages = np.stack([synth.synthetic_page(80 + i, 1024, 768, n_words=10 + 5 * i) for i in range(2)])
buf = DeviceBuffer(pages.nbytes); buf.upload(pages)
single = [list(r) for r in eng.pages_to_data_dev(buf, 2, 1024, 768, conf=True)]   # the same batch without a communicator
comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
comm.attach(True)
res = eng.pages_to_data_dev(buf, 2, 1024, 768, conf=True)
assert [list(r) for r in res] == single
counts, ids = comm.last_gathered()
conf, prob = comm.last_gathered_conf()
assert np.array_equal(ids, np.concatenate([r.ids for r in res]))
assert np.array_equal(conf, np.concatenate([r.conf for r in res])) and np.array_equal(prob, np.concatenate([r.prob for r in res]))
got = 0
def check(prev):
    global got
    assert [list(r) for r in prev] == single
    c, p = comm.last_gathered_conf()
    assert np.array_equal(c, np.concatenate([r.conf for r in prev])) and np.array_equal(p, np.concatenate([r.prob for r in prev]))
    got += 1
for k in range(3):                                                                # streamed batches: the gather rides every pass
    prev = eng.stream_push(buf, 2, 1024, 768, conf=True)
    if prev:
        check(prev)
while True:
    prev = eng.stream_flush(conf=True)
    if not prev:
        break
    check(prev)
assert got == 3
comm.attach(False)
lat = comm.pages_to_data_sharded(buf, 2, 1024, 768, conf=True)
assert [list(r) for r in lat] == single
comm.close()
print("OK", sum(len(s) for s in single))
'''

RANK2 = r'''
import sys
import numpy as np
sys.path.insert(0, {root!r})
from tuatara_amd import synth
from tuatara_amd.engine import Comm, DeviceBuffer, Engine
rank, world, port = int(sys.argv[1]), 2, int(sys.argv[2])
eng = Engine({wdir!r})
comm = Comm(eng, rank, world, "127.0.0.1", port, transport="socket")
mine = np.stack([synth.synthetic_page(90 + 3 * rank + i, 1024, 768, n_words=6 + 7 * rank + 3 * i) for i in range(3)])
other = np.stack([synth.synthetic_page(90 + 3 * (1 - rank) + i, 1024, 768, n_words=6 + 7 * (1 - rank) + 3 * i) for i in range(3)])
buf = DeviceBuffer(mine.nbytes); buf.upload(mine)
obuf = DeviceBuffer(other.nbytes); obuf.upload(other)
solo_mine = eng.pages_to_data_dev(buf, 3, 1024, 768, conf=True)
solo_other = eng.pages_to_data_dev(obuf, 3, 1024, 768, conf=True)
by_rank = [solo_mine, solo_other] if rank == 0 else [solo_other, solo_mine]
assert sum(len(p) for p in by_rank[0]) != sum(len(p) for p in by_rank[1])       # ragged totals: the payload is padded to the larger one
comm.attach(True)
checked = 0
def check(res):
    global checked
    assert [list(p) for p in res] == [list(p) for p in solo_mine]
    counts, ids = comm.last_gathered()
    conf, prob = comm.last_gathered_conf()
    assert np.array_equal(ids, np.concatenate([p.ids for r in by_rank for p in r]))
    assert np.array_equal(conf, np.concatenate([p.conf for r in by_rank for p in r]))
    assert np.array_equal(prob, np.concatenate([p.prob for r in by_rank for p in r]))
    checked += 1
check(eng.pages_to_data_dev(buf, 3, 1024, 768, conf=True))                       # synchronous batch
for k in range(2):                                                                # streamed batches
    res = eng.stream_push(buf, 3, 1024, 768, conf=True)
    if res:
        check(res)
while True:
    res = eng.stream_flush(conf=True)
    if not res:
        break
    check(res)
assert checked == 3
comm.attach(False)
lat = comm.pages_to_data_sharded(obuf if rank == 0 else None, 3 if rank == 0 else 0, 1024, 768, conf=True)
if rank == 0:
    assert [list(p) for p in lat] == [list(p) for p in solo_other]
comm.close()
print("OK rank", rank)
'''


def test_world_one_over_rccl(weights):
    code = WORLD1.format(root=ROOT, wdir=weights["dir"])
    env = dict(os.environ, TUATARA_PRELOAD_TORCH="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, (out.stdout[-1000:], out.stderr[-3000:])


def test_world_two_over_the_socket_transport(weights):
    from tuatara_amd.launch import free_port
    port = free_port()
    code = RANK2.format(root=ROOT, wdir=weights["dir"])
    env = dict(os.environ, TUATARA_PRELOAD_TORCH="0", TUATARA_COMM_TIMEOUT="240")
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(2)]
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=900)
            outs.append((p.returncode, o, e))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (rc, o, e) in enumerate(outs):
        assert rc == 0 and f"OK rank {r}" in o, (r, rc, o[-800:], e[-3000:])


# ------------------------------------------------------------------------------------------------- callers
def test_pytuatara_conf_keyword(weights, pages, eng_x4, eng_rect, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    monkeypatch.delenv("TUATARA_PRECISION", raising=False)
    monkeypatch.delenv("TUATARA_CROP_MODE", raising=False)
    page = pages[0]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    withc = pytuatara.image_to_data(page, weights["dir"], "o", conf=True)
    assert set(plain[0]) == {"text", "bbox"} and set(withc[0]) == {"text", "bbox"} | CONF_KEYS
    want = eng_x4.image_to_data(page, conf=True)
    assert [(r["text"], list(r["bbox"]), r["conf"], list(r["char_conf"])) for r in withc] == [(g["text"], g["bbox"], g["conf"], g["char_conf"]) for g in want]
    both = pytuatara.image_to_data(page, weights["dir"], "o", rectify=True, conf=True)
    assert set(both[0]) == {"text", "bbox", "quad"} | CONF_KEYS
    want = eng_rect.image_to_data(page, conf=True)
    assert [(r["text"], list(r["bbox"]), [list(p) for p in r["quad"]], r["conf"], list(r["char_conf"])) for r in both] == \
        [(g["text"], g["bbox"], g["quad"], g["conf"], g["char_conf"]) for g in want]
    assert pytuatara.images_to_data([page], weights["dir"], "o", conf=True) == [withc]
    assert pytuatara.images_to_data([page], weights["dir"], "o", rectify=True, conf=True) == [both]
    with pytest.raises(TypeError):
        pytuatara.image_to_data(page, weights["dir"], "o", False, True)          # keyword-only


def test_ocr_cli_conf_lines_match_the_python_dicts(weights, funsd, eng_x4, tmp_path):
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if k not in ("TUATARA_PRECISION", "TUATARA_CROP_MODE")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--conf", png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln.split("\t") for ln in out.stdout.splitlines()]
    want = eng_x4.image_to_data(np.ascontiguousarray(funsd[:, :, ::-1]), conf=True)     # the CLI feeds BGR
    assert len(lines) == len(want) > 20
    for (bb, conf, text), g in zip(lines, want):
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"]
        assert conf == f"{g['conf']:.6f}"
