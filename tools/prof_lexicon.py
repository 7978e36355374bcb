"""Profile target for lexicon matching (DESIGN.md "Lexicon matching"); writes profiles/lexicon.md.
    rocprofv3 --kernel-trace -d <dir> -o k --output-format csv -- python tools/prof_lexicon.py kernel
                                                              # for a batch of 1 page and of 32 pages, at V = 10^3, 10^5 and 10^6 (M = 4) in that order: 1 warm-up + 5
                                                              # synchronous calls each; the trace holds lexicon_score_kernel and lexicon_merge_kernel, and every call
                                                              # prints the recogniser stage's time of the same batch (the engine's events), with no lexicon set too
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d <dir> -o c --output-format csv -- python tools/prof_lexicon.py counters
                                                              # a run of its own, no tracing beside it: 32 pages, V = 10^5, 1 warm-up + 2 calls
    rocprofv3 --kernel-trace -d <dir> -o t --output-format csv -- python tools/prof_lexicon.py trace [<tree>]
                                                              # no lexicon set: 1 warm-up + 2 calls of 2 pages; <tree>: the checkout whose tuatara_amd to import
                                                              # (default: this one), so that the parent build is traced by the same script
    python tools/prof_lexicon.py default [<tree>]            # no lexicon set: pages/s of 32 pages per call and single-page p50, three rounds, one line per round
    python tools/prof_lexicon.py report [--kernel CSV] [--counters CSV] [--trace-this CSV] [--trace-parent CSV] LOG... [--out FILE]
                                                              # profiles/lexicon.md from those files and the logs of `kernel`, `default` and bench.py (a line `build=parent` or
                                                              # `build=this` in a log names the build of the figures behind it); whatever is missing reads "not measured"
Workloads: f16x4, structured synthetic weights, the benchmark's 1024 x 768 synthetic pages (synth.synthetic_page(seed, 1024, 768, 40, layout="cells5x8")); the
lexicon: unique random words of 1..25 characters, lengths uniform, classes uniform over the characters a lexicon byte can name - the layout's worst case
for LDS bank conflicts (lexicon.hip's header)."""
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else ""
VS = (10 ** 3, 10 ** 5, 10 ** 6)
BATCHES = (1, 32)
M = 4
CALLS = 5


def engine(tree):
    sys.path.insert(0, tree or ROOT)
    from tuatara_amd import engine as E
    from tuatara_amd import weights as W
    d = tempfile.mkdtemp()
    W.make_synthetic_weights(d, seed=0, structured=True)
    return E, E.Engine(d)


def bench_pages(n):
    from tuatara_amd import synth
    return np.stack([synth.synthetic_page(i, 1024, 768, 40, layout="cells5x8") for i in range(n)])


def random_words(v, seed=0):
    """v unique words as bytes: lengths uniform in 1..25, characters uniform over the ones a lexicon byte can name"""
    chars = np.frombuffer(("0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ" + "!\"#$%&'()*+,-./:;<=>?@[^_`{|}").encode(), np.uint8)
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < v:
        L = rng.integers(1, 26, v)
        body = chars[rng.integers(0, len(chars), (v, 25))]
        for i in range(v):
            out.add(body[i, :L[i]].tobytes())
            if len(out) == v:
                break
    return sorted(out)


def out(**kv):
    print("prof_lexicon " + " ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


def kernel_rows(path):
    """rocprofv3's kernel trace -> [(kernel name, duration in ns)] in start order"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    return [(name, ns) for _, name, ns in rows]


def short(name):
    """a kernel's name without its arguments and template list (the sequence is compared on these)"""
    name = name.split("(")[0]
    return name.split("<")[0].replace("void ", "").replace("ttr::", "").strip()


if mode == "kernel":
    E, eng = engine(None)
    lex = {v: random_words(v) for v in VS}
    for b in BATCHES:
        pages = bench_pages(b)
        buf = E.DeviceBuffer(pages.nbytes)
        buf.upload(pages)
        for v in (0,) + VS:
            eng.set_lexicon(lex[v] if v else None, M)
            ms = []
            for _ in range(1 + CALLS):
                res = eng.pages_to_data_dev(buf, b, 1024, 768)
                ms.append(eng.last_stage_ms()["parseq"])
            out(mode="kernel", pages=b, v=v, m=M if v else 0, crops=sum(len(r) for r in res), calls=1 + CALLS, parseq_ms=",".join(f"{x:.3f}" for x in ms[1:]))
        buf.free()
    eng.set_lexicon(None)

elif mode == "counters":
    E, eng = engine(None)
    pages = bench_pages(32)
    buf = E.DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    eng.set_lexicon(random_words(10 ** 5), M)
    for _ in range(3):
        res = eng.pages_to_data_dev(buf, 32, 1024, 768)
    out(mode="counters", pages=32, v=10 ** 5, m=M, crops=sum(len(r) for r in res), calls=3)

elif mode == "trace":
    E, eng = engine(sys.argv[2] if len(sys.argv) > 2 else None)
    pages = bench_pages(2)
    buf = E.DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    for _ in range(3):
        res = eng.pages_to_data_dev(buf, 2, 1024, 768)
    out(mode="trace", crops=sum(len(r) for r in res), calls=3)

elif mode == "default":
    E, eng = engine(sys.argv[2] if len(sys.argv) > 2 else None)
    pages = bench_pages(32)
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

elif mode == "report":
    args = sys.argv[2:]
    opt = {"--out": os.path.join(ROOT, "profiles", "lexicon.md"), "--kernel": None, "--counters": None, "--trace-this": None, "--trace-parent": None}
    logs, i = [], 0
    while i < len(args):
        if args[i] in opt:
            opt[args[i]] = args[i + 1]
            i += 2
        else:
            logs.append(args[i])
            i += 1
    build = "this"
    fig = {b: {"bench": [], "rate": [], "p50": []} for b in ("parent", "this")}
    runs = []                                                   # the `kernel` mode's lines, in order
    for path in logs:
        for line in open(path, errors="replace"):
            line = line.strip()
            if line.startswith("build="):
                build = line.split("=", 1)[1]
            elif line.startswith("{") and ("\"metric\"" in line or "pages_per_s" in line):
                try:
                    j = json.loads(line)
                    v = j.get("value", j.get("pages_per_s"))
                    if v is not None:
                        fig[build]["bench"].append(float(v))
                except ValueError:
                    pass
            elif line.startswith("prof_lexicon "):
                kv = dict(t.split("=", 1) for t in line.split()[1:])
                if kv["mode"] == "default":
                    fig[build]["rate"].append(float(kv["pages_per_s"]))
                    fig[build]["p50"].append(float(kv["p50_ms"]))
                elif kv["mode"] == "kernel":
                    runs.append(kv)

    def span(v):
        return f"{min(v):.6g} - {max(v):.6g}" if v else "not measured"

    def med(v):
        return f"{np.median(v):.2f}; {min(v):.2f} - {max(v):.2f}" if len(v) else "not measured"

    def inside(mine, theirs):
        if not mine or not theirs:
            return "not measured"
        k = sum(min(theirs) <= x <= max(theirs) for x in mine)
        above, below = [x for x in mine if x > max(theirs)], [x for x in mine if x < min(theirs)]
        note = "".join(f"; {name} it: {', '.join(f'{x:.6g}' for x in v)}" for name, v in (("above", above), ("below", below)) if v)
        return f"{k} of {len(mine)} inside the parent's spread{note}"

    md = ["# Lexicon matching: the scorer and its merge beside the recogniser pass, the gather's LDS bank conflicts, and the default path (no lexicon) against the parent build", "",
          "Written by `tools/prof_lexicon.py report` from rocprofv3 output and the logs of its `kernel` and `default` modes and of `bench.py --gpus 1 --steps 20",
          "--warmup 5` (MI355X, f16x4, structured synthetic weights; the tool's docstring describes the workloads).  No figure was fixed in advance.", "",
          "## The kernels (a report)", "",
          f"The benchmark's pages per synchronous call (`ttr_pages_to_data_dev`), M = {M}, 1 warm-up + {CALLS} calls at each lexicon size, one process under",
          "`rocprofv3 --kernel-trace`; kernel times are the trace's end - start per launch.  The recogniser stage is the engine's own event pair around",
          "`parseq_forward` of the same calls, the scorer and the merge included; V = 0 is the same batch with no lexicon set.", "",
          "| pages per call | V | crops per call | lexicon_score_kernel, us per launch (median; min - max of the timed launches) | lexicon_merge_kernel, us (median; min - max) | recogniser stage of the same calls, ms (median; min - max) |",
          "|---|---|---|---|---|---|"]
    score, merge = [], []
    if opt["--kernel"]:
        for name, ns in kernel_rows(opt["--kernel"]):
            if short(name) == "lexicon_score_kernel":
                score.append(ns / 1e3)
            elif short(name) == "lexicon_merge_kernel":
                merge.append(ns / 1e3)
    with_lex = [r for r in runs if int(r["v"]) > 0]
    complete = bool(score) and len(score) == len(merge) == len(with_lex) * (1 + CALLS)
    k = 0
    for r in runs:
        ms = [float(x) for x in r["parseq_ms"].split(",")]
        if int(r["v"]) == 0:
            md.append(f"| {r['pages']} | 0 | {r['crops']} | - | - | {med(ms)} |")
            continue
        if complete:
            a, b = score[k * (1 + CALLS) + 1:(k + 1) * (1 + CALLS)], merge[k * (1 + CALLS) + 1:(k + 1) * (1 + CALLS)]   # (the first launch is the warm-up call's)
            md.append(f"| {r['pages']} | {r['v']} | {r['crops']} | {med(a)} | {med(b)} | {med(ms)} |")
        else:
            md.append(f"| {r['pages']} | {r['v']} | {r['crops']} | not measured | not measured | {med(ms)} |")
        k += 1
    if not runs:
        md.append("| not measured | | | | | |")
    if opt["--kernel"] and not complete:
        md += ["", f"(the trace holds {len(score)} scorer and {len(merge)} merge launches, {len(with_lex) * (1 + CALLS)} expected: the kernel columns are not filled in)"]
    md += ["", f"The side block is 8 M = {8 * M} bytes per crop (M indices, M log-probabilities), one device-to-host copy per batch; with no lexicon set no side block",
           "exists and nothing is launched or copied.", "",
           "## LDS bank conflicts of the scorer's gather", "",
           "`rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE` in a run of its own, no tracing beside it: 32 pages per call, V = 10^5 uniformly random words (the",
           "layout's worst case), 1 warm-up + 2 calls; the counters of `lexicon_score_kernel`'s launches, summed.", ""]
    if opt["--counters"]:
        tot = {}
        with open(opt["--counters"], newline="") as f:
            for r in csv.DictReader(f):
                if short(r.get("Kernel_Name", "")) == "lexicon_score_kernel":
                    tot[r["Counter_Name"]] = tot.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        c, a = tot.get("SQ_LDS_BANK_CONFLICT"), tot.get("SQ_LDS_IDX_ACTIVE")
        if c is not None and a:
            md += [f"- SQ_LDS_BANK_CONFLICT = {c:.6g}, SQ_LDS_IDX_ACTIVE = {a:.6g}: {100 * c / a:.1f} % of the LDS-array cycles are conflict cycles, an average degree of {a / (a - c):.2f}" if a > c else
                   f"- SQ_LDS_BANK_CONFLICT = {c:.6g}, SQ_LDS_IDX_ACTIVE = {a:.6g}", ""]
        else:
            md += ["not measured (the counter file holds no row of the scorer)", ""]
    else:
        md += ["not measured", ""]
    md += ["## No lexicon set runs the parent's launch sequence", "",
           "Two pages per synchronous call, 1 warm-up + 2 calls, nothing set, each build in its own process under `rocprofv3 --kernel-trace`; the kernels' names",
           "(template arguments dropped) in start order."]
    if opt["--trace-this"] and opt["--trace-parent"]:
        a, b = [short(n) for n, _ in kernel_rows(opt["--trace-this"])], [short(n) for n, _ in kernel_rows(opt["--trace-parent"])]
        md += ["", f"- this build: {len(a)} launches, {a.count('decode_conf_kernel')} of `decode_conf_kernel`, {a.count('lexicon_score_kernel')} of `lexicon_score_kernel`",
               f"- parent build: {len(b)} launches, {b.count('decode_conf_kernel')} of `decode_conf_kernel`",
               f"- the two sequences of kernel names are {'identical' if a == b else 'NOT identical'}" +
               ("" if a == b else f" (first difference at launch {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))})"), ""]
    elif opt["--trace-this"]:
        a = [short(n) for n, _ in kernel_rows(opt["--trace-this"])]
        md += ["", f"- this build: {len(a)} launches, {a.count('decode_conf_kernel')} of `decode_conf_kernel`, {a.count('lexicon_score_kernel')} of `lexicon_score_kernel`, "
               f"{a.count('lexicon_merge_kernel')} of `lexicon_merge_kernel`", "- parent build: not measured", ""]
    else:
        md += ["", "not measured", ""]
    md += ["## The default path (no lexicon) against the parent build", "",
           "The parent build and this build ran alternately on the same box, one process per run.", "",
           "| quantity | parent build, every figure in order | this build, every figure in order | this build against the parent's spread |", "|---|---|---|---|"]
    for key, name in (("bench", "headline pages/s (`bench.py --gpus 1 --steps 20 --warmup 5`)"), ("rate", "pages/s over 4 synchronous calls of 32 pages"), ("p50", "single-page p50 (30 calls), ms")):
        p, t = fig["parent"][key], fig["this"][key]
        md.append(f"| {name} | {', '.join(f'{x:.6g}' for x in p) or 'not measured'} ({span(p)}) | {', '.join(f'{x:.6g}' for x in t) or 'not measured'} ({span(t)}) | {inside(t, p)} |")
    with open(opt["--out"], "w") as f:
        f.write("\n".join(md) + "\n")
    print(opt["--out"])

else:
    raise SystemExit("usage: prof_lexicon.py kernel | counters | trace [TREE] | default [TREE] | report [--kernel CSV] [--counters CSV] [--trace-this CSV] [--trace-parent CSV] LOG... [--out FILE]")
