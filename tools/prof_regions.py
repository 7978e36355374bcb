"""Profile target for regions and per-row character sets (DESIGN.md "Regions and per-row character sets"); writes profiles/regions.md.
    python tools/prof_regions.py default                      # the default path: pages/s of 32 pages per call and single-page p50, three rounds; prints one line
                                                              # per round (runs on a build without the feature too: TUATARA_LIB=<the parent's library>)
    python tools/prof_regions.py rowtable                     # 320 crops under three sets: mixed in one call (the row table) against three set_charset passes
    python tools/prof_regions.py regions                      # 32 bench pages: each page's own word quads read as regions against the full page call
    python tools/prof_regions.py report LOG... [--out FILE]   # profiles/regions.md from the logs of the runs above and of bench.py (label=... lines, see below)
Every measuring mode prints `key=value` lines that begin with `prof_regions`; a log handed to `report` may carry a line `build=parent` or `build=this`
in front of the figures that follow it, and bench.py's JSON line is read as it is.  Workloads: f16x4, structured synthetic weights; pages are the
benchmark's 1024 x 768 synthetic pages (synth.synthetic_page(seed, 1024, 768, 40, layout="cells5x8")).  A set changes when words end, so the AR step
count under sets depends on the data: the row-table figures are a report, not a bar."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIGITS, UPPER = "0123456789", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
mode = sys.argv[1] if len(sys.argv) > 1 else "default"


def engine():
    from tuatara_amd import engine as E
    from tuatara_amd import weights as W
    if os.environ.get("TUATARA_LIB"):                      # another build of the library: bind the symbols it has
        try:
            import torch  # noqa: F401  (before the library, as engine.load() does: one HIP runtime per process)
        except ImportError:
            pass
        lib = C.CDLL(E.lib_path())
        E.SYMBOLS = [s for s in E.SYMBOLS if hasattr(lib, s[0])]
    d = tempfile.mkdtemp()
    W.make_synthetic_weights(d, seed=0, structured=True)
    return E, E.Engine(d), d


def bench_pages(n=32):
    from tuatara_amd import synth
    return np.stack([synth.synthetic_page(i, 1024, 768, 40, layout="cells5x8") for i in range(n)])


def out(**kv):
    print("prof_regions " + " ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


if mode == "default":
    E, eng, _ = engine()
    pages = bench_pages()
    buf, one = E.DeviceBuffer(pages.nbytes), E.DeviceBuffer(pages[0].nbytes)
    buf.upload(pages)
    one.upload(pages[0])
    for rnd in range(3):
        eng.pages_to_data_dev(buf, 32, 1024, 768, keep=False)
        t0 = time.perf_counter()
        for _ in range(4):
            eng.pages_to_data_dev(buf, 32, 1024, 768, keep=False)
        rate = 4 * 32 / (time.perf_counter() - t0)
        lat = []
        for _ in range(30):
            t0 = time.perf_counter()
            eng.pages_to_data_dev(one, 1, 1024, 768, keep=False)
            lat.append((time.perf_counter() - t0) * 1e3)
        out(mode="default", round=rnd, pages_per_s=f"{rate:.1f}", p50_ms=f"{float(np.median(lat)):.3f}")

elif mode == "rowtable":
    E, eng, _ = engine()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import charset_ref as CR
    crops = CR.sweep_crops(5, 320)
    sets = [(DIGITS, None), (UPPER, None), (None, None)]
    masks = E.charset_masks(sets)
    set_of = np.arange(320, dtype=np.int32) % 3

    def timed(fn, reps=5):
        fn()
        eng.set_profiling(2)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        prof = eng.get_profile()
        eng.set_profiling(0)
        return ms, {k: v["launches"] // reps for k, v in prof.items()}

    def three():
        for a, d in sets:
            eng.set_charset(a, d)
            eng.parseq_logits(crops)
        eng.set_charset()

    for rnd in range(3):
        ms1, l1 = timed(lambda: eng.parseq_logits(crops, set_of=set_of, sets=masks))
        ms3, l3 = timed(three)
        out(mode="rowtable", round=rnd, mixed_ms=f"{ms1:.2f}", mixed_launches=json.dumps(l1).replace(" ", ""), three_passes_ms=f"{ms3:.2f}",
            three_passes_launches=json.dumps(l3).replace(" ", ""))

elif mode == "regions":
    E, eng, d = engine()
    pages = bench_pages()
    buf = E.DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    rect = E.Engine(d, crop_mode=E.CROP_RECTIFIED)          # the words' quads, once, untimed (same items and order in every crop mode)
    found = rect.pages_to_data_dev(buf, 32, 1024, 768)
    rect.close()
    quads = [r.quad for r in found]
    n = sum(len(q) for q in quads)
    regs = (E.Region * n)()
    k = 0
    for pg, q in enumerate(quads):
        for row in q:
            regs[k] = E.Region((C.c_float * 8)(*[float(v) for v in row]), pg, -1)
            k += 1
    table = eng._page_array([(buf.ptr + i * pages[0].nbytes, 1024, 768) for i in range(32)])
    arr = (C.c_void_p * 32)()

    def regions_call():
        eng._check(eng.lib.ttr_regions_to_data_dev(eng.h, table, 32, regs, n, None, 0, arr))
        for i in range(32):
            eng.lib.ttr_result_free(arr[i])

    for rnd in range(3):
        res = {}
        for name, fn in (("page_call", lambda: eng.pages_to_data_dev(buf, 32, 1024, 768, keep=False)), ("regions", regions_call)):
            fn()
            t0 = time.perf_counter()
            for _ in range(4):
                fn()
            res[name] = (4 * 32 / (time.perf_counter() - t0), eng.last_stage_ms())
        out(mode="regions", round=rnd, words=n, page_call_pages_per_s=f"{res['page_call'][0]:.1f}", page_call_stage_ms=json.dumps({k: round(v, 3) for k, v in res["page_call"][1].items()}).replace(" ", ""),
            regions_pages_per_s=f"{res['regions'][0]:.1f}", regions_stage_ms=json.dumps({k: round(v, 3) for k, v in res["regions"][1].items()}).replace(" ", ""))

elif mode == "report":
    args = sys.argv[2:]
    dst = os.path.join(ROOT, "profiles", "regions.md")
    if "--out" in args:
        dst = args[args.index("--out") + 1]
        args = [a for i, a in enumerate(args) if a != "--out" and (i == 0 or args[i - 1] != "--out")]
    build = "this"
    fig = {"parent": {"bench": [], "rate": [], "p50": []}, "this": {"bench": [], "rate": [], "p50": []}}
    rowtable, regions = [], []
    for path in args:
        for line in open(path, errors="replace"):
            line = line.strip()
            if line.startswith("build="):
                build = line.split("=", 1)[1]
            elif line.startswith("{") and "\"metric\"" in line or line.startswith("{") and "pages_per_s" in line:
                try:
                    j = json.loads(line)
                    v = j.get("value", j.get("pages_per_s"))
                    if v is not None:
                        fig[build]["bench"].append(float(v))
                except ValueError:
                    pass
            elif line.startswith("prof_regions "):
                kv = dict(t.split("=", 1) for t in line.split()[1:])
                if kv["mode"] == "default":
                    fig[build]["rate"].append(float(kv["pages_per_s"]))
                    fig[build]["p50"].append(float(kv["p50_ms"]))
                elif kv["mode"] == "rowtable":
                    rowtable.append(kv)
                elif kv["mode"] == "regions":
                    regions.append(kv)

    def span(v):
        return f"{min(v):.3f} - {max(v):.3f}" if v else "not measured"

    def inside(mine, theirs):
        if not mine or not theirs:
            return "not measured"
        k = sum(min(theirs) <= x <= max(theirs) for x in mine)
        above, below = [x for x in mine if x > max(theirs)], [x for x in mine if x < min(theirs)]
        note = "".join(f"; {name} it: {', '.join(str(x) for x in v)}" for name, v in (("above", above), ("below", below)) if v)
        return f"{k} of {len(mine)} inside the parent's spread{note}"

    md = ["# Regions and per-row character sets: the default path against the parent build, the row table against one set per pass, regions against detection", "",
          "Written by `tools/prof_regions.py report` from the logs of its measuring modes and of `bench.py --gpus 1 --steps 20 --warmup 5` (MI355X, f16x4,",
          "synthetic structured weights; the tool's docstring describes the workloads).  The parent build and this build ran alternately, one process per run.", "",
          "## The default path (no regions, no row table) against the parent build", "",
          "| quantity | parent build, every figure in order | this build, every figure in order | this build against the parent's spread |", "|---|---|---|---|"]
    for key, name in (("bench", "headline pages/s (`bench.py --gpus 1 --steps 20 --warmup 5`)"), ("rate", "pages/s over 4 synchronous calls of 32 pages"), ("p50", "single-page p50 (30 calls), ms")):
        p, t = fig["parent"][key], fig["this"][key]
        md.append(f"| {name} | {', '.join(f'{x:.6g}' for x in p) or 'not measured'} ({span(p)}) | {', '.join(f'{x:.6g}' for x in t) or 'not measured'} ({span(t)}) | {inside(t, p)} |")
    worst = [inside(fig["this"][k], fig["parent"][k]) for k in ("bench", "rate", "p50")]
    met = all(w != "not measured" and w.split()[0] == w.split()[2] for w in worst)
    md += ["", "The bar is every figure of this build inside the parent's own spread from the same session: " + ("met by all figures." if met else "NOT met by all figures (see the last column)."), ""]
    md += ["## Row table against one set (a report: the step count depends on the data)", "",
           "The same 320 crops (`charset_ref.sweep_crops(5, 320)`) under digits, `A-Z` and the full set dealt by `i % 3`: mixed in one call (`ttr_parseq_logits_sets`, the row",
           "table) and as three `set_charset` passes over all 320 crops (what a caller without the table runs to read every crop under its set).  Milliseconds per",
           "call (host clock around the synchronous call, mean of 5) and timed matrix launches per call from `ttr_get_profile`.", "",
           "| round | mixed, ms | mixed, launches | three passes, ms | three passes, launches |", "|---|---|---|---|---|"]
    md += [f"| {r['round']} | {r['mixed_ms']} | `{r['mixed_launches']}` | {r['three_passes_ms']} | `{r['three_passes_launches']}` |" for r in rowtable] or ["| not measured | | | | |"]
    md += ["", "## Regions against detection (a report; no target is set)", "",
           "32 of the benchmark's 1024 x 768 synthetic pages per synchronous call: the full page call (`ttr_pages_to_data_dev`) against each page's own word quads",
           "read as regions (`ttr_regions_to_data_dev`, set -1).  pages/s over 4 calls and `ttr_last_stage_ms` of the last call ({craft, post, pack, parseq}).", "",
           "| round | words | page call, pages/s | page call, stage ms | regions, pages/s | regions, stage ms |", "|---|---|---|---|---|---|"]
    md += [f"| {r['round']} | {r['words']} | {r['page_call_pages_per_s']} | `{r['page_call_stage_ms']}` | {r['regions_pages_per_s']} | `{r['regions_stage_ms']}` |" for r in regions] or ["| not measured | | | | | |"]
    with open(dst, "w") as f:
        f.write("\n".join(md) + "\n")
    print(dst)

else:
    raise SystemExit("usage: prof_regions.py default | rowtable | regions | report LOG... [--out FILE]")
