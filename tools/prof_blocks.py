"""Profile target for text blocks (DESIGN.md "Text blocks"): what `blocks = 1` costs beside `lines = 1`, on the GPU and on the host.
    python tools/prof_blocks.py                                                                  # stage times, pages/s, host rule times
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_blocks.py pages <0|1|2>  # kernel table of the page workload
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_blocks.py dense        # both kernels on 8 pages of 4096 words
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_blocks.py cap          # ... on one page of 512 blocks
Page workload: 32 synthetic 1024 x 768 pages (config 5, f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four
timed calls per round; `pages 0` is the default engine (its dispatch count is the one to hold against the parent build's), `pages 1` lines
on, `pages 2` lines and blocks on.  Without arguments lines-only and lines + blocks alternate for ROUNDS rounds in this one process.  Dense
workload: ttr_group_blocks on 8 pages of 4096 words (four of loose random quads, four of 64 rows of 64 linked words).  Cap workload: one page
of 512 words far apart, 16 columns of 32: 512 blocks, the largest precedence matrix and the longest selection loop.  The host rule
(ttr_blocks_from_quads) is timed on the same inputs."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import blocks_ref as B                                         # noqa: E402
from tests import lines_ref as L                                          # noqa: E402
from tuatara_amd import synth, weights as W                               # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                       # noqa: E402

ROUNDS = 3
mode = sys.argv[1] if len(sys.argv) > 1 else "all"
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
CONFIGS = {0: {}, 1: {"lines": 1}, 2: {"lines": 1, "blocks": 1}}


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
    from tuatara_amd.engine import blocks_from_quads, lines_from_quads
    best = [1e9, 1e9]
    for _ in range(reps):
        for k, fn in enumerate((lines_from_quads, blocks_from_quads)):
            t0 = time.perf_counter()
            for q in sets:
                fn(q)
            best[k] = min(best[k], time.perf_counter() - t0)
    return best[0] * 1e6, best[1] * 1e6


def stage_time(eng, sets, calls=4):
    first = np.cumsum([0] + [len(q) for q in sets]).astype(np.int32)
    quads = np.concatenate(sets)
    out = {}
    for name, fn in (("ttr_group_lines", eng.group_lines), ("ttr_group_blocks", eng.group_blocks)):
        res = fn(quads, first)
        t0 = time.perf_counter()
        for _ in range(calls):
            res = fn(quads, first)
        out[name] = ((time.perf_counter() - t0) / calls * 1e3, res)
    return out


if mode in ("all", "pages"):
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    which = [int(sys.argv[2])] if mode == "pages" else [1, 2]
    engs = {k: Engine(d, **CONFIGS[k]) for k in which}
    for rnd in range(ROUNDS if mode == "all" else 1):
        for k in which:
            res, rate, ms = page_run(engs[k], buf)
            words = sum(len(r) for r in res)
            extra = (f", {sum(len(r.lines) for r in res)} lines" if k else "") + (f", {sum(len(r.blocks) for r in res)} blocks" if k == 2 else "")
            print(f"round {rnd} {CONFIGS[k] or 'default'}: {words} words per call{extra}, pack {ms['pack']:.3f} ms, recogniser stage {ms['parseq']:.3f} ms "
                  f"(last call), {rate:.1f} pages/s over 4 synchronous calls, host_us {engs[k].last_host_us()}")
    if mode == "all":
        quads = [r.quad for r in Engine(d, crop_mode=1).pages_to_data_dev(buf, 32, 1024, 768)]   # (the same boxes; this crop mode's Python results carry the quads)
        tl, tb = host_time(quads)
        print(f"host rules on the 32 pages' quads ({sum(len(q) for q in quads)} words, largest page {max(len(q) for q in quads)}): lines {tl:.1f} us, "
              f"lines + blocks {tb:.1f} us per 32 pages")

if mode in ("all", "dense"):
    eng = Engine(d)
    sets = dense_pages()
    t = stage_time(eng, sets)
    nb, md = t["ttr_group_blocks"][1][5], t["ttr_group_blocks"][1][6]
    print(f"dense, 8 pages of 4096 words: ttr_group_lines {t['ttr_group_lines'][0]:.3f} ms, ttr_group_blocks (both kernels) {t['ttr_group_blocks'][0]:.3f} ms per call "
          f"(upload, kernels, download, host conversion); blocks per page {nb.tolist()}, mode {md.tolist()}")
    if mode == "all":
        tl, tb = host_time(sets, 2)
        print(f"host rules on the 8 dense pages: lines {tl / 1e3:.1f} ms, lines + blocks {tb / 1e3:.1f} ms")

if mode in ("all", "cap"):
    eng = Engine(d)
    sets = [B.isolated_words(512, per_row=16)]
    t = stage_time(eng, sets)
    print(f"cap, one page of 512 blocks: ttr_group_lines {t['ttr_group_lines'][0]:.3f} ms, ttr_group_blocks (both kernels) {t['ttr_group_blocks'][0]:.3f} ms per call; "
          f"blocks {t['ttr_group_blocks'][1][5].tolist()}, mode {t['ttr_group_blocks'][1][6].tolist()}")
    if mode == "all":
        tl, tb = host_time(sets)
        print(f"host rules on the 512-block page: lines {tl:.1f} us, lines + blocks {tb:.1f} us")
