"""Profile target for character boxes (DESIGN.md "Character boxes"): what `chars = 1` costs.
    python tools/prof_chars.py                                                                  # stage times and pages/s, chars off / on alternated; the stage call on FUNSD-like counts
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_chars.py pages <0|1>    # kernel table of the page workload, chars off / on
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_chars.py stage        # char_cut_kernel on 72 words of one plane (a FUNSD-like crop count)
Page workload: 32 synthetic 1024 x 768 pages (config 5, f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four
timed calls per round; without arguments chars off and chars on alternate for ROUNDS rounds in this one process.  With chars on the kernel
table holds char_cut_kernel (one launch per batch) and the per-slot copy of the region planes shows among the memory copies (a
device-to-device copy of 32 x 512 x 384 x 4 bytes; --memory-copy-trace in a run of its own lists it).  Stage workload: ttr_char_cuts on one
512 x 512 random plane and 72 words, timed as a whole call (upload of the plane included)."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import chars_ref as R                                          # noqa: E402
from tuatara_amd import synth, weights as W                               # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine, chars_from_map       # noqa: E402

ROUNDS = 3
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)


def page_run(eng, buf, calls=4):
    res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    t0 = time.perf_counter()
    for _ in range(calls):
        res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    dt = time.perf_counter() - t0
    return res, calls * 32 / dt, eng.last_stage_ms()


if mode in ("all", "pages"):
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    which = [int(sys.argv[2])] if mode == "pages" else [0, 1]
    engs = {k: Engine(d, chars=k) for k in which}
    for rnd in range(ROUNDS if mode == "all" else 1):
        for k in which:
            res, rate, ms = page_run(engs[k], buf)
            words = sum(len(r) for r in res)
            extra = f", {sum(int(r.char_first[-1]) for r in res if len(r))} characters, {sum(int((r.char_mode == 1).sum()) for r in res if len(r))} words cut at valleys" if k else ""
            print(f"round {rnd} chars={k}: {words} words per call{extra}, pack {ms['pack']:.3f} ms, recogniser stage {ms['parseq']:.3f} ms (last call), "
                  f"{rate:.1f} pages/s over 4 synchronous calls, host_us {engs[k].last_host_us()}")

if mode in ("all", "stage"):
    eng = Engine(d)
    T = R.random_map(9, 512, 512)
    quads, turns, nchars = R.random_words(10, 72, 512, 512, 1.0)
    eng.char_cuts(T, 1.0, 0.4, quads, turns, nchars)
    t0 = time.perf_counter()
    for _ in range(8):
        cuts, modes, prof = eng.char_cuts(T, 1.0, 0.4, quads, turns, nchars)
    dt = (time.perf_counter() - t0) / 8
    print(f"stage: ttr_char_cuts on 72 words of a 512 x 512 plane: {dt * 1e3:.3f} ms per call (upload of the plane, kernel, download), {int((modes == 1).sum())} words cut at valleys")
    if mode == "all":
        t0 = time.perf_counter()
        chars_from_map(T, 1.0, 0.4, quads, turns, nchars)
        print(f"host rule on the same 72 words: {(time.perf_counter() - t0) * 1e6:.1f} us")
