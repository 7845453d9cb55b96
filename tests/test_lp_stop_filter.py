"""The stop-test filters of csrc/lpbox_lp_stoptest.h on the CPU: tests/lp_stop_filter_check.cpp, a stand-alone program built from that
header alone, checks that wherever a filter says "certainly above the threshold" the exact expression is above it -- on random
operands over the guarded range, on operands at threshold * (1 +- {0, 2^-52, 2^-40, 2^-31, 2^-30, 2^-29}) -- and that every guard
case (zero, subnormal, infinity, NaN, |x|^2 below 2^-100, a zero deviation) is inconclusive.  Built with AddressSanitizer + UBSan where
the host compiler can link them, plain otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated-lpbox-admm_amd", "csrc")
BASE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("stopfilter") / "lp_stop_filter_check")
    probe = subprocess.run([gxx, *BASE, *SAN, "-x", "c++", "-", "-o", exe], input="int main() { return 0; }\n", text=True, capture_output=True)
    flags = BASE + (SAN if probe.returncode == 0 else [])
    subprocess.run([gxx, *flags, "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "lp_stop_filter_check.cpp"), "-o", exe], check=True)
    return exe


def test_filters_never_contradict_the_exact_expressions(checker):
    run = subprocess.run([checker], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stop filter ok" in run.stdout


def test_thresholds_of_the_checker_are_the_kernels():
    """The program hard-codes the two thresholds; they must be those of csrc/lpbox_lp.h."""
    import re
    text = open(os.path.join(CSRC, "lpbox_lp.h")).read()
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"#define (LP_STOP_THRESHOLD|LP_STD_THRESHOLD)\s+(\S+)", text)}
    assert got == {"LP_STOP_THRESHOLD": 1e-4, "LP_STD_THRESHOLD": 1e-12}
