"""Profile target for the fuzzy alignment of lexicon entries (DESIGN.md "Lexicon matching", Fuzzy alignment); writes profiles/lexicon_fuzzy.md.
    rocprofv3 --kernel-trace -d <dir> -o k --output-format csv -- python tools/prof_lexicon_fuzzy.py kernel
                                                              # for a batch of 1 page and of 32 pages, at V = 10^3, 10^5 and 10^6 (M = 4), with the mode off (the rigid
                                                              # scorer of the same build) and at band 0..3, in that order: 1 warm-up + 3 synchronous calls each; every
                                                              # call prints the recogniser stage's time of the same batch (the engine's events)
    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d <dir> -o c --output-format csv -- python tools/prof_lexicon_fuzzy.py counters
                                                              # a run of its own, no tracing beside it: 32 pages, V = 10^5, the mode off and band 0..3, 1 warm-up + 1 call each
    python tools/prof_lexicon_fuzzy.py report [--kernel CSV] [--counters CSV] LOG... [--out FILE]
                                                              # profiles/lexicon_fuzzy.md from those files and the logs of `kernel` and of bench.py (a line `build=parent` or
                                                              # `build=this` in a log names the build of the figures behind it); whatever is missing reads "not measured"
Workloads: tools/prof_lexicon.py's - f16x4, structured synthetic weights, the benchmark's 1024 x 768 synthetic pages, unique uniformly random words of 1..25
characters (the worst case for LDS bank conflicts).  The gap is the convenience layers' default, ln 1e-3."""
import csv
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else ""
VS = (10 ** 3, 10 ** 5, 10 ** 6)
BATCHES = (1, 32)
BANDS = (-1, 0, 1, 2, 3)                                        # -1: the mode off, the rigid scorer
M = 4
CALLS = 3
GAP = -6.9077554
SCORERS = ("lexicon_score_kernel", "lexicon_fuzzy_score_kernel")


def engine():
    sys.path.insert(0, ROOT)
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
    print("prof_lexicon_fuzzy " + " ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


def short(name):
    name = name.split("(")[0]
    return name.split("<")[0].replace("void ", "").replace("ttr::", "").strip()


def kernel_rows(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    return [(short(name), ns / 1e3) for _, name, ns in rows]


def med(v):
    return f"{np.median(v):.1f}; {min(v):.1f} - {max(v):.1f}" if len(v) else "not measured"


if mode == "kernel":
    E, eng = engine()
    lex = {v: random_words(v) for v in VS}
    for b in BATCHES:
        pages = bench_pages(b)
        buf = E.DeviceBuffer(pages.nbytes)
        buf.upload(pages)
        for v in VS:
            eng.set_lexicon(lex[v], M)
            for band in BANDS:
                eng.set_lexicon_fuzzy(band if band >= 0 else None, GAP)
                ms = []
                for _ in range(1 + CALLS):
                    res = eng.pages_to_data_dev(buf, b, 1024, 768)
                    ms.append(eng.last_stage_ms()["parseq"])
                out(mode="kernel", pages=b, v=v, band=band, m=M, crops=sum(len(r) for r in res), calls=1 + CALLS, parseq_ms=",".join(f"{x:.3f}" for x in ms[1:]))
        buf.free()
    eng.set_lexicon_fuzzy(None)
    eng.set_lexicon(None)

elif mode == "counters":
    E, eng = engine()
    pages = bench_pages(32)
    buf = E.DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    eng.set_lexicon(random_words(10 ** 5), M)
    for band in BANDS:
        eng.set_lexicon_fuzzy(band if band >= 0 else None, GAP)
        for _ in range(2):
            res = eng.pages_to_data_dev(buf, 32, 1024, 768)
        out(mode="counters", pages=32, v=10 ** 5, band=band, m=M, crops=sum(len(r) for r in res), calls=2)

elif mode == "report":
    args = sys.argv[2:]
    opt = {"--out": os.path.join(ROOT, "profiles", "lexicon_fuzzy.md"), "--kernel": None, "--counters": None}
    logs, i = [], 0
    while i < len(args):
        if args[i] in opt:
            opt[args[i]] = args[i + 1]
            i += 2
        else:
            logs.append(args[i])
            i += 1
    build = "this"
    bench = {"parent": [], "this": []}
    runs = []
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
                        bench[build].append(float(v))
                except ValueError:
                    pass
            elif line.startswith("prof_lexicon_fuzzy "):
                kv = dict(t.split("=", 1) for t in line.split()[1:])
                if kv["mode"] == "kernel":
                    runs.append(kv)
    md = ["# Fuzzy alignment of lexicon entries: the fuzzy scorer beside the rigid one and the recogniser pass, the edits kernel, LDS bank conflicts, and the mode-off path against the parent build", "",
          "Written by `tools/prof_lexicon_fuzzy.py report` from rocprofv3 output and the logs of its `kernel` mode and of `bench.py --gpus 1 --steps 20 --warmup 5`",
          "(MI355X, f16x4, structured synthetic weights; the tool's docstring describes the workloads).  No figure was fixed in advance: the expectation that the",
          "scorer's cost grows roughly with 2B + 1 over the rigid one is an estimate from the count of LDS reads, not an acceptance bar.", "",
          "## The kernels (a report)", "",
          f"The benchmark's pages per synchronous call (`ttr_pages_to_data_dev`), M = {M}, gap ln 1e-3, 1 warm-up + {CALLS} calls per row, one process under",
          "`rocprofv3 --kernel-trace`; kernel times are the trace's end - start, summed over a call's launches (a batch of more than 4096 crops goes through the",
          "recogniser in groups, one scorer launch each).  Band -1 is the mode off: `lexicon_score_kernel`, the rigid scorer of the",
          "same build.  The recogniser stage is the engine's own event pair around `parseq_forward` of the same calls, scorer, merge and edits kernel included.", "",
          "| pages per call | V | band | crops per call | scorer, us per call (median; min - max) | against the rigid scorer | lexicon_fuzzy_edits_kernel, us (median; min - max) | recogniser stage of the same calls, ms (median; min - max) |",
          "|---|---|---|---|---|---|---|---|"]
    score, edits = [], []
    if opt["--kernel"]:
        for name, us in kernel_rows(opt["--kernel"]):
            if name in SCORERS:
                score.append(us)
            elif name == "lexicon_fuzzy_edits_kernel":
                edits.append(us)
    def groups(r):
        return -(-int(r["crops"]) // 4096)                                          # a batch of more than 4096 crops goes through the recogniser in even groups: one launch per group

    def per_call(v, at, g):
        """the launches of one run from index `at` on, summed per call; the warm-up call's left out"""
        return [sum(v[at + c * g:at + (c + 1) * g]) for c in range(1, 1 + CALLS)]
    want_score = sum((1 + CALLS) * groups(r) for r in runs)
    want_edits = sum((1 + CALLS) * groups(r) for r in runs if int(r["band"]) >= 0)
    complete = bool(score) and len(score) == want_score and len(edits) == want_edits
    k = ke = 0
    rigid = None
    for r in runs:
        ms = [float(x) for x in r["parseq_ms"].split(",")]
        band = int(r["band"])
        if complete:
            g = groups(r)
            a = per_call(score, k, g)
            e = per_call(edits, ke, g) if band >= 0 else []
            if band < 0:
                rigid = float(np.median(a))
            ratio = "1" if band < 0 else f"{np.median(a) / rigid:.2f} x (2B + 1 = {2 * band + 1})" if rigid else "not measured"
            md.append(f"| {r['pages']} | {r['v']} | {band} | {r['crops']} | {med(a)} | {ratio} | {med(e) if band >= 0 else '-'} | {med(ms)} |")
        else:
            md.append(f"| {r['pages']} | {r['v']} | {band} | {r['crops']} | not measured | not measured | not measured | {med(ms)} |")
        k += (1 + CALLS) * groups(r)
        ke += (1 + CALLS) * groups(r) if band >= 0 else 0
    if not runs:
        md.append("| not measured | | | | | | | |")
    if opt["--kernel"] and not complete:
        md += ["", f"(the trace holds {len(score)} scorer and {len(edits)} edits launches, {want_score} and {want_edits} expected: the kernel columns are not filled in)"]
    md += ["", f"In the mode the side block is 12 M = {12 * M} bytes per crop (M indices, M log-probabilities, M edit counts), one device-to-host copy per batch; with the",
           "mode off it is the lexicon's own 8 M bytes, and nothing of this file's is launched, sized or copied.", "",
           "## LDS bank conflicts of the scorers' gathers", "",
           "`rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE` in a run of its own, no tracing beside it: 32 pages per call, V = 10^5 uniformly random words (the",
           "layout's worst case), the mode off and band 0..3, 1 warm-up + 1 call each; the counters of each scorer instantiation's launches, summed.", ""]
    if opt["--counters"]:
        tot = {}
        with open(opt["--counters"], newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                if short(name) in SCORERS:
                    key = name.split("(")[0].replace("void ", "").replace("ttr::", "").strip()
                    tot.setdefault(key, {}).setdefault(r["Counter_Name"], 0.0)
                    tot[key][r["Counter_Name"]] += float(r["Counter_Value"])
        if tot:
            md += ["| kernel<CAP[, B]> | SQ_LDS_BANK_CONFLICT | SQ_LDS_IDX_ACTIVE | conflict cycles of the LDS-array cycles |", "|---|---|---|---|"]
            for key in sorted(tot):
                c, a = tot[key].get("SQ_LDS_BANK_CONFLICT"), tot[key].get("SQ_LDS_IDX_ACTIVE")
                md.append(f"| `{key}` | {c:.6g} | {a:.6g} | {100 * c / a:.1f} % |" if c is not None and a else f"| `{key}` | not measured | not measured | not measured |")
            md.append("")
        else:
            md += ["not measured (the counter file holds no row of a scorer)", ""]
    else:
        md += ["not measured", ""]
    md += ["## The mode-off path against the parent build", "",
           "`bench.py --gpus 1 --steps 20 --warmup 5` (no lexicon, no mode), the parent build and this build alternately on the same box, one process per run; the",
           "parent's spread is the spread of its own repeated runs.", "",
           "| quantity | parent build, every figure in order | this build, every figure in order | this build against the parent's spread |", "|---|---|---|---|"]
    p, t = bench["parent"], bench["this"]

    def span(v):
        return f"{min(v):.6g} - {max(v):.6g}" if v else "not measured"
    if p and t:
        inside = sum(min(p) <= x <= max(p) for x in t)
        above, below = [x for x in t if x > max(p)], [x for x in t if x < min(p)]
        verdict = f"{inside} of {len(t)} inside" + "".join(f"; {nm} it: {', '.join(f'{x:.6g}' for x in v)}" for nm, v in (("above", above), ("below", below)) if v)
    else:
        verdict = "not measured"
    md.append(f"| headline pages/s | {', '.join(f'{x:.6g}' for x in p) or 'not measured'} (spread {span(p)}) | {', '.join(f'{x:.6g}' for x in t) or 'not measured'} (spread {span(t)}) | {verdict} |")
    with open(opt["--out"], "w") as f:
        f.write("\n".join(md) + "\n")
    print(opt["--out"])

else:
    raise SystemExit("usage: prof_lexicon_fuzzy.py kernel | counters | report [--kernel CSV] [--counters CSV] LOG... [--out FILE]")
