"""CPU suite: the local ink host rule (tuatara_amd/csrc/geometry.cpp and ink_rule.h; DESIGN.md "Local ink") under AddressSanitizer and UBSan.
tests/native/ink_san.cpp is a stand-alone program built with the host compiler - no HIP, nothing loaded into Python.  It drives the whole rule, the record's validation and the ink forms of
the tables and deskew rules over seeded pages of the kinds tests/test_ink_cpu.py uses (gradients under noise, blank and all-black pages, inverses, widths about
the word size, heights of 1, pages smaller than the window, padded strides), every buffer sized exactly, and holds every bit to the rule evaluated from its
definition: any out-of-bounds access or signed overflow turns into a sanitizer report and a non-zero exit.  Fails on the parent commit: geometry.cpp has no
ink_from_page there, so the program does not build - which this test treats as a failure, not a skip, once a plain build works."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "ink_san.cpp"), os.path.join(CSRC, "geometry.cpp")]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path_factory.mktemp("ink_san"))
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(flags + [probe, "-o", os.path.join(d, "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer build not available here")
    out = os.path.join(d, "ink_san")
    r = subprocess.run(flags + SRC + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_host_rule_under_sanitizers(san_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([san_bin, str(seed), "36"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "pages" and int(words[1]) == 36 and int(words[3]) > 0 and int(words[5]) > 0   # (pages were read as light ink, and pixels were ink)
