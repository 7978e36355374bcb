"""CPU suite: the barcode host rule (tuatara_amd/csrc/geometry.cpp and barcodes_rule.h; DESIGN.md "Barcodes") under AddressSanitizer and UBSan.
tests/native/barcodes_san.cpp is a stand-alone program built with the host compiler - no HIP, nothing loaded into Python.  It drives the ink pass, the
transpose, the whole rule under both ink rules, the items' barcodes and the block's validation over seeded pages of the kinds tests/test_barcodes_cpu.py uses
(codes across word boundaries, on and cut by the page's edges, cut short, a page beyond the cap, widths about the word size and padded strides included), every
buffer sized exactly: any out-of-bounds access or signed overflow turns into a sanitizer report and a non-zero exit.  Fails on the parent commit: geometry.cpp
has no barcodes_from_page there, so the program does not build - which this test treats as a failure, not a skip, once a plain build works."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "barcodes_san.cpp"), os.path.join(CSRC, "geometry.cpp")]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path_factory.mktemp("barcodes_san"))
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(flags + [probe, "-o", os.path.join(d, "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer build not available here")
    out = os.path.join(d, "barcodes_san")
    r = subprocess.run(flags + SRC + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_host_rule_under_sanitizers(san_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([san_bin, str(seed), "120"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "pages" and int(words[1]) == 120 and int(words[3]) > 0 and int(words[5]) > 0 and int(words[7]) > 0   # (barcodes, hits and overflows occurred)
