"""Profile target for text lines (DESIGN.md "Text lines"): what `lines = 1` costs, on the GPU and on the host.
    python tools/prof_lines.py                                                                 # stage times, pages/s, host rule times
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_lines.py pages <0|1>   # kernel table of the page workload, lines off / on
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_lines.py dense       # line_group_kernel on 8 pages of 4096 words
Page workload: 32 synthetic 1024 x 768 pages (config 5, f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four
timed calls per round; without arguments lines off and lines on alternate for ROUNDS rounds in this one process.  Dense workload:
ttr_group_lines on 8 pages of 4096 words (four of loose random quads, four of 64 rows of 64 linked words).  The host rule
(ttr_lines_from_quads) is timed on the same two inputs: the 32 pages' own quads, and the 8 dense pages."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lines_ref as L                                          # noqa: E402
from tuatara_amd import synth, weights as W                               # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine, lines_from_quads    # noqa: E402

ROUNDS = 3
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)


def dense_pages():
    loose = [L.random_quads(4096, 70 + k) for k in range(4)]
    rows = [np.concatenate([L.row_quads(20, 30 + 26.0 * r, [14.0 + (r + k + s) % 5 for k in range(64)], 16.0, 5.0) for r in range(64)]) for s in range(4)]
    return loose + rows


def page_run(eng, buf, calls=4):
    res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    t0 = time.perf_counter()
    for _ in range(calls):
        res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    dt = time.perf_counter() - t0
    ms = eng.last_stage_ms()
    return res, calls * 32 / dt, ms


def host_time(sets, reps=5):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        for q in sets:
            lines_from_quads(q)
        best = min(best, time.perf_counter() - t0)
    return best * 1e6


if mode in ("all", "pages"):
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    which = [int(sys.argv[2])] if mode == "pages" else [0, 1]
    engs = {k: Engine(d, lines=k) for k in which}
    for rnd in range(ROUNDS if mode == "all" else 1):
        for k in which:
            res, rate, ms = page_run(engs[k], buf)
            words = sum(len(r) for r in res)
            extra = f", {sum(len(r.lines) for r in res)} lines" if k else ""
            print(f"round {rnd} lines={k}: {words} words per call{extra}, pack {ms['pack']:.3f} ms, recogniser stage {ms['parseq']:.3f} ms (last call), "
                  f"{rate:.1f} pages/s over 4 synchronous calls, host_us {engs[k].last_host_us()}")
    if mode == "all":
        quads = [r.quad for r in Engine(d, crop_mode=1).pages_to_data_dev(buf, 32, 1024, 768)]   # (the same boxes; this crop mode's Python results carry the quads)
        print(f"host rule on the 32 pages' quads ({sum(len(q) for q in quads)} words, largest page {max(len(q) for q in quads)}): {host_time(quads):.1f} us per 32 pages")

if mode in ("all", "dense"):
    eng = Engine(d)
    sets = dense_pages()
    first = np.cumsum([0] + [len(q) for q in sets]).astype(np.int32)
    quads = np.concatenate(sets)
    eng.group_lines(quads, first)
    t0 = time.perf_counter()
    for _ in range(4):
        line, word, nl = eng.group_lines(quads, first)
    dt = (time.perf_counter() - t0) / 4
    print(f"dense: ttr_group_lines on 8 pages of 4096 words: {dt * 1e3:.3f} ms per call (upload, kernel, download, host conversion), lines per page {nl.tolist()}")
    if mode == "all":
        print(f"host rule on the 8 dense pages: {host_time(sets, 2) / 1e3:.1f} ms")
