"""Profile target for the character alternatives (DESIGN.md "Character alternatives"); writes profiles/alts.md.
    rocprofv3 --kernel-trace -d <dir> -o k --output-format csv -- python tools/prof_alts.py kernel
                                                              # 32 bench pages per synchronous call, 1 warm-up + 5 calls at each of K = 2, 5, 8 in that order: the
                                                              # trace holds decode_alts_kernel beside decode_conf_kernel of the same run
    rocprofv3 --kernel-trace -d <dir> -o t --output-format csv -- python tools/prof_alts.py trace [<tree>]
                                                              # K = 0 (nothing set): 1 warm-up + 2 calls of 2 pages; <tree>: the checkout whose tuatara_amd to import
                                                              # (default: this one), so that the parent build is traced by the same script
    python tools/prof_alts.py default [<tree>]               # K = 0: pages/s of 32 pages per call and single-page p50, three rounds, one line per round
    python tools/prof_alts.py report --kernel CSV --trace-this CSV --trace-parent CSV LOG... [--out FILE]
                                                              # profiles/alts.md from the kernel traces (rocprofv3's *_kernel_trace.csv) and the logs of `default` and of
                                                              # bench.py (a line `build=parent` or `build=this` in a log names the build of the figures behind it)
Workloads: f16x4, structured synthetic weights, the benchmark's 1024 x 768 synthetic pages (synth.synthetic_page(seed, 1024, 768, 40, layout="cells5x8"))."""
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mode = sys.argv[1] if len(sys.argv) > 1 else ""
KS = (2, 5, 8)
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


def out(**kv):
    print("prof_alts " + " ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


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
    pages = bench_pages(32)
    buf = E.DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    for k in KS:
        eng.set_alternatives(k)
        for _ in range(1 + CALLS):
            res = eng.pages_to_data_dev(buf, 32, 1024, 768)
        out(mode="kernel", k=k, crops=sum(len(r) for r in res), calls=1 + CALLS, extra_bytes_per_crop=26 * k * 8)
    eng.set_alternatives(0)

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
    opt = {"--out": os.path.join(ROOT, "profiles", "alts.md"), "--kernel": None, "--trace-this": None, "--trace-parent": None}
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
    kern = {}
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
            elif line.startswith("prof_alts "):
                kv = dict(t.split("=", 1) for t in line.split()[1:])
                if kv["mode"] == "default":
                    fig[build]["rate"].append(float(kv["pages_per_s"]))
                    fig[build]["p50"].append(float(kv["p50_ms"]))
                elif kv["mode"] == "kernel":
                    kern[int(kv["k"])] = kv

    def span(v):
        return f"{min(v):.6g} - {max(v):.6g}" if v else "not measured"

    def inside(mine, theirs):
        if not mine or not theirs:
            return "not measured"
        k = sum(min(theirs) <= x <= max(theirs) for x in mine)
        above, below = [x for x in mine if x > max(theirs)], [x for x in mine if x < min(theirs)]
        note = "".join(f"; {name} it: {', '.join(f'{x:.6g}' for x in v)}" for name, v in (("above", above), ("below", below)) if v)
        return f"{k} of {len(mine)} inside the parent's spread{note}"

    md = ["# Character alternatives: decode_alts_kernel beside decode_conf_kernel, the bytes it adds, and the default path (K = 0) against the parent build", "",
          "Written by `tools/prof_alts.py report` from rocprofv3 kernel traces and the logs of its `default` mode and of `bench.py --gpus 1 --steps 20 --warmup 5`",
          "(MI355X, f16x4, structured synthetic weights; the tool's docstring describes the workloads).  No figure was fixed in advance.", "",
          "## The kernel (a report)", "",
          "32 of the benchmark's pages per synchronous call (`ttr_pages_to_data_dev`), 1 warm-up + 5 calls at each K, one process under `rocprofv3 --kernel-trace`;",
          "kernel times are the trace's end - start per launch.  `decode_conf_kernel` is the launch directly in front of each `decode_alts_kernel`, in the same run.", "",
          "| K | crops per call | decode_alts_kernel, us per launch (median; min - max of the timed launches) | decode_conf_kernel beside it, us (median; min - max) | side block, bytes per crop (26 K ids + 26 K probabilities, one device-to-host copy per batch) |",
          "|---|---|---|---|---|"]
    if opt["--kernel"]:
        rows = kernel_rows(opt["--kernel"])
        pairs = [(rows[i - 1][1], ns) for i, (name, ns) in enumerate(rows) if short(name) == "decode_alts_kernel" and i > 0 and short(rows[i - 1][0]) == "decode_conf_kernel"]
        per = len(pairs) // len(KS) if pairs else 0
        for j, k in enumerate(KS):
            mine = pairs[j * per:(j + 1) * per][1:]                 # (the first launch at each K is the warm-up call's)
            if not mine or per != 1 + CALLS:
                md.append(f"| {k} | not measured (the trace holds {len(pairs)} launch pairs, {len(KS) * (1 + CALLS)} expected) | | | |")
                continue
            a, c = [ns / 1e3 for _, ns in mine], [ns / 1e3 for ns, _ in mine]
            md.append(f"| {k} | {kern.get(k, {}).get('crops', '?')} | {np.median(a):.2f}; {min(a):.2f} - {max(a):.2f} | {np.median(c):.2f}; {min(c):.2f} - {max(c):.2f} | {26 * k * 8} |")
    else:
        md.append("| not measured | | | | |")
    md += ["", "The standard block is 212 bytes per crop (26 ids, 26 probabilities, 1 confidence); with K = 0 no side block exists and nothing is copied.", ""]
    md += ["## K = 0 runs the parent's launch sequence", "",
           "Two pages per synchronous call, 1 warm-up + 2 calls, nothing set, each build in its own process under `rocprofv3 --kernel-trace`; the kernels' names",
           "(template arguments dropped) in start order."]
    if opt["--trace-this"] and opt["--trace-parent"]:
        a, b = [short(n) for n, _ in kernel_rows(opt["--trace-this"])], [short(n) for n, _ in kernel_rows(opt["--trace-parent"])]
        md += ["", f"- this build: {len(a)} launches, {a.count('decode_conf_kernel')} of `decode_conf_kernel`, {a.count('decode_alts_kernel')} of `decode_alts_kernel`",
               f"- parent build: {len(b)} launches, {b.count('decode_conf_kernel')} of `decode_conf_kernel`",
               f"- the two sequences of kernel names are {'identical' if a == b else 'NOT identical'}" +
               ("" if a == b else f" (first difference at launch {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))})"), ""]
    else:
        md += ["", "not measured", ""]
    md += ["## The default path (K = 0) against the parent build", "",
           "The parent build and this build ran alternately on the same box, one process per run.", "",
           "| quantity | parent build, every figure in order | this build, every figure in order | this build against the parent's spread |", "|---|---|---|---|"]
    for key, name in (("bench", "headline pages/s (`bench.py --gpus 1 --steps 20 --warmup 5`)"), ("rate", "pages/s over 4 synchronous calls of 32 pages"), ("p50", "single-page p50 (30 calls), ms")):
        p, t = fig["parent"][key], fig["this"][key]
        md.append(f"| {name} | {', '.join(f'{x:.6g}' for x in p) or 'not measured'} ({span(p)}) | {', '.join(f'{x:.6g}' for x in t) or 'not measured'} ({span(t)}) | {inside(t, p)} |")
    with open(opt["--out"], "w") as f:
        f.write("\n".join(md) + "\n")
    print(opt["--out"])

else:
    raise SystemExit("usage: prof_alts.py kernel | trace [TREE] | default [TREE] | report --kernel CSV --trace-this CSV --trace-parent CSV LOG... [--out FILE]")
