"""Profile target for the best decode of patterns (DESIGN.md "Patterns", the likeliest member) -> profiles/pattern_best.md.
    python tools/prof_pattern_best.py decode OUT.json    # 1280 crops' logits through the two stage calls: decode_pat_kernel (greedy) beside decode_conf_kernel +
                                                         # pattern_best_kernel (best), three patterns; wall clock of the stage calls (upload, kernels, download,
                                                         # synchronise), median of 20 after a warm-up.  Under rocprofv3 --kernel-trace --stats the kernel table
                                                         # gives the kernels' own times: pass its *_kernel_stats.csv to `report`
    python tools/prof_pattern_best.py pages OUT.json     # pages/s of 32 pages per call and single-page p50 with no pattern, a greedy pattern and - where the
                                                         # library has the mode - the best decode, alternated in one process, three rounds; and how many words
                                                         # change their reading between the modes.  Runs on a parent build too (TUATARA_LIB=...)
    python tools/prof_pattern_best.py pages-greedy OUT.json   # the same without the best decode: the process a parent build runs, for a like-for-like comparison
    python tools/prof_pattern_best.py report OUT.md decode.json current.json [parent_a.json parent_b.json] [kernel_stats.csv]
Page workload: 32 synthetic 1024 x 768 pages (f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four timed calls per round;
single-page p50: 30 synchronous calls on the first page.  A figure that was not taken is written as "not measured"."""
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 3
PAGE_PATTERN = r"[A-Z][a-z]*"
DECODE_PATTERNS = [r"\d{2}/\d{2}/\d{4}", r".{0,25}", r"[ab]*a[ab]{7}"]      # the last one: a minimal automaton of 256 states


def engine():
    from tuatara_amd import weights as W
    from tuatara_amd.engine import Engine
    d = tempfile.mkdtemp()
    W.make_synthetic_weights(d, seed=0, structured=True)
    return Engine(d)


def decode(out):
    eng = engine()
    n = 1280
    x = np.random.default_rng(5).normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    of = np.zeros(n, np.int32)
    rows = []
    for p in DECODE_PATTERNS:
        calls = {"greedy": lambda: eng.logits_decode_patterns(x, [p], of), "best": lambda: eng.logits_decode_patterns(x, [p], of, best=True)}
        ms = {}
        for _ in range(2):                                      # alternated
            for name, f in calls.items():
                f()
                t = []
                for _ in range(10):
                    t0 = time.perf_counter()
                    f()
                    t.append((time.perf_counter() - t0) * 1e3)
                ms.setdefault(name, []).extend(t)
        g, b = eng.logits_decode_patterns(x, [p], of), eng.logits_decode_patterns(x, [p], of, best=True)
        changed = int((g[0] != b[0]).any(1).sum())
        rows.append({"pattern": p, "greedy_ms": float(np.median(ms["greedy"])), "best_ms": float(np.median(ms["best"])), "changed": changed, "n": n})
        print(rows[-1])
    json.dump({"decode": rows}, open(out, "w"))


def pages(out, with_best=True):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    eng = engine()
    has_mode = hasattr(eng.lib, "ttr_engine_set_pattern_decode")
    has_best = has_mode and with_best
    imgs = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
    buf, one = DeviceBuffer(imgs.nbytes), DeviceBuffer(imgs[0].nbytes)
    buf.upload(imgs)
    one.upload(imgs[0])

    def use(mode):
        if has_best:
            eng.set_pattern_decode(1 if mode == "best" else 0)
        eng.set_pattern(None if mode == "none" else PAGE_PATTERN)

    modes = ["none", "greedy"] + (["best"] if has_best else [])
    rate, p50, texts = {m: [] for m in modes}, {m: [] for m in modes}, {}
    for _ in range(ROUNDS):
        for m in modes:
            use(m)
            res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            t0 = time.perf_counter()
            for _ in range(4):
                res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            rate[m].append(4 * 32 / (time.perf_counter() - t0))
            lat = []
            for _ in range(30):
                t0 = time.perf_counter()
                eng.pages_to_data_dev(one, 1, 1024, 768)
                lat.append((time.perf_counter() - t0) * 1e3)
            p50[m].append(float(np.median(lat)))
            texts[m] = [t for r in res for t in r.texts]
    gain = None
    if has_best:                                                # the gain in logp: the pages' own crop batches through the stage calls, the greedy reading scored by rule 2 on the host (float64)
        use("best")
        gains = []
        for img in imgs[:8]:
            canvas, ratio = eng.resize_canvas(img)
            crops, _ = eng.pack_crops(img, eng.ccl_boxes(eng.craft_heatmap(canvas)), ratio)
            if not len(crops):
                continue
            lg, _ = eng.parseq_logits(crops)
            own = np.full(len(crops), -1, np.int32)
            b_ids, _, _, b_logp = eng.logits_decode_patterns(lg, None, own, best=True)
            g_ids = eng.logits_decode_patterns(lg, None, own)[0]
            x = lg.astype(np.float64)
            m = x.max(-1, keepdims=True)
            lp = x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))       # (the engine's set is every class)
            for i in np.nonzero((b_ids != g_ids).any(1))[0]:
                row = g_ids[i].tolist()
                L = row.index(0) if 0 in row else 25
                gains.append(float(b_logp[i]) - float(sum(lp[i, p, row[p]] for p in range(L)) + lp[i, L, 0]))
        gain = {"words": len(gains), "mean": float(np.mean(gains)) if gains else 0.0, "pages": 8}
    use("none")
    r = {"pages": {m: {"pages_per_s": rate[m], "p50_ms": p50[m]} for m in modes}, "words": len(texts["greedy"]), "build": "this" if has_mode else "parent"}
    if has_best:
        r["gain"] = gain
        r["changed"] = sum(a != b for a, b in zip(texts["greedy"], texts["best"]))
    print(r)
    json.dump(r, open(out, "w"))


def report(out, paths):
    data, stats = [], None
    for p in paths:
        if p.endswith(".csv"):
            stats = {row.get("Name", ""): row for row in csv.DictReader(open(p))}
        else:
            data.append(json.load(open(p)))
    dec = next((d["decode"] for d in data if "decode" in d), None)
    runs = [d for d in data if "pages" in d]
    cur = next((d for d in runs if "best" in d["pages"]), None)
    parents = [d for d in runs if "best" not in d["pages"] and d.get("build") != "this"]
    alike = [d for d in runs if "best" not in d["pages"] and d.get("build") == "this"]
    md = ["# The best decode of patterns: what it costs", "",
          "Written by `tools/prof_pattern_best.py report` from runs on one MI355X (f16x4, structured synthetic weights).  Nothing was fixed in advance.", ""]
    md += ["## The decode stage on 1280 crops", "",
           "Wall clock of the stage calls `ttr_logits_decode_patterns` (greedy: `decode_pat_kernel`) and `ttr_logits_decode_patterns_best` (`decode_conf_kernel`",
           "into scratch, then `pattern_best_kernel`): the upload of 12.6 MB of logits, the table, the kernels, the download and the synchronise; median of 20,",
           "the two alternated.", "",
           "| pattern | greedy call (ms) | best call (ms) | rows whose reading changes |", "|---|---|---|---|"]
    if dec:
        md += [f"| `{r['pattern']}` | {r['greedy_ms']:.3f} | {r['best_ms']:.3f} | {r['changed']} of {r['n']} |" for r in dec]
    else:
        md += ["| not measured | | | |"]
    md += ["", "The kernels' own times (`rocprofv3 --kernel-trace --stats`, a run of its own):", ""]
    names = [k for k in (stats or {}) if any(s in k for s in ("pattern_best_kernel", "decode_pat_kernel", "decode_conf_kernel"))]
    if names:
        md += ["| kernel | calls | average (us) |", "|---|---|---|"]
        for k in names:
            row = stats[k]
            avg = row.get("AverageNs") or row.get("Average") or ""
            md.append(f"| `{k.split('(')[0]}` | {row.get('Calls', '')} | {float(avg) / 1e3:.1f} |" if avg else f"| `{k}` | {row.get('Calls', '')} | not measured |")
    else:
        md += ["not measured"]

    def line(name, d, m):
        if d is None or m not in d["pages"]:
            return f"| {name} | not measured | not measured |"
        v = d["pages"][m]
        return f"| {name} | {', '.join(f'{x:.1f}' for x in v['pages_per_s'])} | {', '.join(f'{x:.2f}' for x in v['p50_ms'])} |"

    md += ["", "## Pages", "", f"Engine pattern `{PAGE_PATTERN}`; 32 pages per call (pages/s, three rounds) and single-page p50 (ms, three rounds); the modes alternate in one process.",
           "", "| run | pages/s | single-page p50 (ms) |", "|---|---|---|",
           line("this build, no pattern", cur, "none"), line("this build, greedy pattern", cur, "greedy"), line("this build, best decode", cur, "best")]
    for i, d in enumerate(parents):
        md += [line(f"parent build, run {i + 1}, no pattern", d, "none"), line(f"parent build, run {i + 1}, greedy pattern", d, "greedy")]
    for i, d in enumerate(alike):
        md += [line(f"this build, greedy-only process, run {i + 1}, no pattern", d, "none"), line(f"this build, greedy-only process, run {i + 1}, greedy pattern", d, "greedy")]
    if not parents:
        md += ["| parent build | not measured | not measured |"]
    if len(parents) >= 2 and (alike or cur):
        md += ["", "The parent's run-to-run spread is taken as the range of its rounds over both runs; this build's rounds are those of its greedy-only processes where",
               "there are any (the same process a parent build runs), else those of the process that also runs the best decode."]
        for m in ("none", "greedy"):
            pv = [x for d in parents for x in d["pages"][m]["pages_per_s"]]
            tv = [x for d in (alike or [cur]) for x in d["pages"][m]["pages_per_s"]]
            lo, hi = min(pv), max(pv)
            inside = lo <= float(np.median(tv)) <= hi
            md += ["", f"{'No pattern' if m == 'none' else 'Greedy pattern'}: the parent's rounds span {lo:.1f} .. {hi:.1f} pages/s ({(hi - lo) / hi * 100:.2f} %); this build's span "
                   f"{min(tv):.1f} .. {max(tv):.1f}, median {np.median(tv):.1f}: " + ("inside the parent's span." if inside else
                   f"{'below' if np.median(tv) < lo else 'above'} it by {min(abs(np.median(tv) - lo), abs(np.median(tv) - hi)) / hi * 100:.2f} %.")]
    md += ["", "## Readings", ""]
    if cur and "changed" in cur:
        md += [f"On the 32 synthetic pages {cur['changed']} of {cur['words']} words change their reading between greedy and best mode under `{PAGE_PATTERN}`."]
    else:
        md += ["Words that change their reading: not measured."]
    g = (cur or {}).get("gain")
    if g and g["words"]:
        md += [f"The mean gain in `logp` over the {g['words']} words that change on the first {g['pages']} pages (their own crop batches through `ttr_parseq_logits` and the two",
               f"stage decodes; the greedy reading scored by the rule on the host, in float64): {g['mean']:.4f}."]
    else:
        md += ["The mean gain in `logp` over those words: not measured."]
    open(out, "w").write("\n".join(md) + "\n")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "decode":
        decode(sys.argv[2])
    elif mode == "pages":
        pages(sys.argv[2])
    elif mode == "pages-greedy":
        pages(sys.argv[2], with_best=False)
    elif mode == "report":
        report(sys.argv[2], sys.argv[3:])
    else:
        sys.exit(__doc__)
