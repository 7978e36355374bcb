"""Profile target for character sets (DESIGN.md "Character sets"): what a set costs, and that it adds no launch.
    python tools/prof_charset.py                                                                  # pages/s and single-page p50: no set, digits, A-Z, alternated
    python tools/prof_charset.py default                                                          # the no-set figures only (runs on a build without the feature too)
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_charset.py steps <none|digits|upper>   # kernel table of a fixed number of AR steps
Page workload: 32 synthetic 1024 x 768 pages (f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four timed calls
per round; single-page p50: 30 synchronous calls on the first page.  A set changes when words end, so the AR step count - and with it the
recogniser's time - depends on the data: the rates under a set are a report, not a bar.
Steps workload: the recogniser alone on the 40 crops of one grid page, five calls with the AR early exit switched off (ar_early_exit = 0): every
call runs all 25 steps whatever the tokens are, so the kernel table's launch counts must be the same with and without a set."""
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
SETS = {"none": (None, None), "digits": ("0123456789", None), "upper": ("ABCDEFGHIJKLMNOPQRSTUVWXYZ", None)}
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)


def use(name):
    if name != "none" or hasattr(eng, "set_charset"):
        eng.set_charset(*SETS[name])


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
    names = ["none"] if mode == "default" else list(SETS)
    for rnd in range(ROUNDS):
        for name in names:
            use(name)
            res, rate, ms = page_run(buf)
            lens = [len(t) for r in res for t in r.texts]
            print(f"round {rnd} set={name}: {len(lens)} words per call, mean length {np.mean(lens):.2f}, longest {max(lens)}, recogniser stage {ms['parseq']:.3f} ms "
                  f"(last call), {rate:.1f} pages/s over 4 synchronous calls, single-page p50 {p50(one):.3f} ms")
    use("none")

if mode == "steps":
    name = sys.argv[2] if len(sys.argv) > 2 else "none"
    crops = np.random.default_rng(7).integers(0, 256, (40, 32, 128, 3), dtype=np.uint8)
    assert eng.set_tuning("ar_early_exit", 0) == 0
    use(name)
    eng.set_profiling(2)
    for _ in range(5):
        _, ids = eng.parseq_logits(crops)
    prof = eng.get_profile()
    eng.set_profiling(0)
    print(f"set={name}: 5 calls x 40 crops, all 25 AR steps; timed matrix launches: recogniser {prof['parseq']['launches']}, AR steps {prof['parseq_ar']['launches']}; "
          f"distinct ids {len(np.unique(ids))}")
