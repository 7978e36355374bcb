"""Profile target for patterns (DESIGN.md "Patterns"): what a pattern costs, and that the default path costs what it cost.
    python tools/prof_pattern.py default      # no pattern: pages/s of 32 pages per call and single-page p50 (runs on a build without the feature too)
    python tools/prof_pattern.py              # no pattern and the engine pattern .{0,25}, alternated in one process, three rounds
    python tools/prof_pattern.py decode       # decode_pat_kernel beside decode_conf_kernel on the same 1280 crops' logits (wall clock of the stage calls;
                                              # under rocprofv3 --kernel-trace --stats the kernel table gives the kernels' own times)
    python tools/prof_pattern.py regions      # 320 region crops under three patterns in one call against three passes of one pattern each
Page workload: 32 synthetic 1024 x 768 pages (f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four timed calls per round;
single-page p50: 30 synchronous calls on the first page.  .{0,25} restricts nothing but the length (and id 88), so words end where they ended and the
difference to no pattern is the cost of the mechanism: the AR argmax as its own launch and the serial decode."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tuatara_amd import synth, weights as W                               # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                      # noqa: E402

ROUNDS = 3
LENGTH_ONLY = r".{0,25}"
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)


def use(pattern):
    if pattern is not None or hasattr(eng, "set_pattern"):
        eng.set_pattern(pattern)


def page_run(buf, calls=4):
    res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    t0 = time.perf_counter()
    for _ in range(calls):
        res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    dt = time.perf_counter() - t0
    return res, calls * 32 / dt, eng.last_stage_ms()


def p50(one, iters=30):
    lat = []
    for _ in range(iters):
        t0 = time.perf_counter()
        eng.pages_to_data_dev(one, 1, 1024, 768)
        lat.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(lat))


if mode in ("all", "default"):
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    one = DeviceBuffer(pages[0].nbytes)
    one.upload(pages[0])
    for rnd in range(ROUNDS):
        for pattern in ([None] if mode == "default" else [None, LENGTH_ONLY]):
            use(pattern)
            res, rate, ms = page_run(buf)
            lens = [len(t) for r in res for t in r.texts]
            print(f"round {rnd} pattern={pattern}: {len(lens)} words per call, mean length {np.mean(lens):.2f}, longest {max(lens)}, recogniser stage {ms['parseq']:.3f} ms "
                  f"(last call), {rate:.1f} pages/s over 4 synchronous calls, single-page p50 {p50(one):.3f} ms")
    use(None)

if mode == "decode":
    n = 1280
    x = np.random.default_rng(7).normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    x[:, :, 0] += np.linspace(-6.0, 6.0, 26)[None, :]                     # words end somewhere in the middle
    none = np.full(n, -1, np.int32)
    cases = {"decode_conf_kernel (logits_confidence)": lambda: eng.logits_confidence(x),
             "decode_pat_kernel, no row has a pattern": lambda: eng.logits_decode_patterns(x, None, none),
             "decode_pat_kernel, .{0,25} on every row": lambda: eng.logits_decode_patterns(x, [LENGTH_ONLY], np.zeros(n, np.int32)),
             r"decode_pat_kernel, \d+\.\d{2} on every row": lambda: eng.logits_decode_patterns(x, [r"\d+\.\d{2}"], np.zeros(n, np.int32))}
    for name, fn in cases.items():
        fn()
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: {n} crops, stage call (upload 12.6 MB, kernel, download) min {min(ts):.3f} ms, median {np.median(ts):.3f} ms")

if mode == "regions":
    page = synth.synthetic_page(3, 1024, 768, n_words=28)
    rng = np.random.default_rng(5)
    regions = []
    for _ in range(320):
        x0, y0 = int(rng.integers(0, 768 - 140)), int(rng.integers(0, 1024 - 40))
        regions.append({"rect": (x0, y0, x0 + int(rng.integers(60, 140)), y0 + int(rng.integers(16, 40)))})
    pats = [r"\d{2}/\d{2}/\d{4}", r"[A-Z]{2}\d{2,6}", r"\d+\.\d{2}"]
    of = [pats[i % 3] for i in range(320)]
    buf = DeviceBuffer(page.nbytes)
    buf.upload(page)
    dev = [(buf, 1024, 768)]

    def one_call():
        return eng.read_regions(dev, regions, patterns=of)

    def three_passes():
        return [eng.read_regions(dev, [r for r, p in zip(regions, of) if p == P], patterns=[P] * sum(p == P for p in of)) for P in pats]

    for name, fn in (("one call, three patterns", one_call), ("three passes, one pattern each", three_passes)):
        fn()
        for rnd in range(ROUNDS):
            ts = []
            for _ in range(10):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            print(f"round {rnd} {name}: 320 regions, min {min(ts):.3f} ms, median {np.median(ts):.3f} ms")
