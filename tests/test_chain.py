"""The host side of the adaptive launch chains: csrc/lpbox_chain.h (what the loops decide) and csrc/lpbox_host.h (the driver, the
graph cache).

CPU: tests/chain_check.cpp, a stand-alone program built from lpbox_chain.h alone, holds the decisions against a table under
AddressSanitizer + UBSan; the rules it prints are the constants tests/chain_cases.py computes the expected resumes with.
GPU: the tree's library reproduces, window for window, the bookkeeping recorded from the commit before the loops were shared
(tests/golden/chain_parent.json, see tests/golden/make_chain_fixture.py), with eager launches and with graphs -- so graph replays and
eager launches count the same launches and collectives, also when the graph cache is hit after kmax has moved away and come back.
"""
import functools
import json
import os
import shutil
import subprocess
import sys

import pytest

from helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated-lpbox-admm_amd", "csrc")
sys.path.insert(0, GOLDEN)
import make_chain_fixture as fixture  # noqa: E402

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def chain_check(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("chain") / "chain_check")
    probe = subprocess.run([gxx, *FLAGS, "-x", "c++", "-", "-o", exe], input="int main() { return 0; }\n", text=True, capture_output=True)
    if probe.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes")
    subprocess.run([gxx, *FLAGS, "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "chain_check.cpp"), "-o", exe], check=True)
    return exe


def test_chain_decisions_under_sanitizers(chain_check):
    run = subprocess.run([chain_check], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "chain ok" in run.stdout


def test_rules_are_the_constants_of_the_resume_tests(chain_check):
    import chain_cases as cc
    run = subprocess.run([chain_check, "rules"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rules = {}
    for line in run.stdout.splitlines():
        name, *fields = line.split()
        rules[name] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    assert sorted(rules) == ["big", "gen", "seg"]
    assert all(r["pairs_per_resume"] == cc.PAIRS_PER_RESUME for r in rules.values())
    assert (rules["seg"]["kmax_start"], rules["seg"]["kmax_cap"], rules["gen"]["kmax_start"]) == (cc.SEG_KMAX_START, cc.SEG_KMAX_LIMIT, cc.BQP_KMAX_START)
    assert rules["seg"]["pcg_cap"] == rules["gen"]["pcg_cap"] == rules["big"]["pcg_cap"] == cc.PCG_MAXITERS
    assert all(r["resume_limit"] == cc.PCG_MAXITERS // cc.PAIRS_PER_RESUME + 2 for r in rules.values())


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def recorded():
    with open(fixture.OUT) as fh:
        return json.load(fh)


@functools.lru_cache(None)
def from_the_tree(eager):
    return fixture.record(eager, extras=True)


def without_extras(rows):
    return [{k: v for k, v in row.items() if k not in fixture.EXTRAS and not (k == "pcg_resumes" and "collectives" in row)} for row in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("launches", ["eager", "graph"])
def test_bookkeeping_equals_the_recorded_one(launches):
    want, got = recorded(), from_the_tree(launches == "eager")
    assert sorted(got) == sorted(want) and len(want) == 9
    for case in sorted(want):
        print(launches, case, got[case])
        assert without_extras(got[case]) == want[case], case
    # the records hold what they are there for: resumes in the adaptive and the forced cases, a moving kmax
    assert want["S2"][0]["pcg_resumes"] >= 2 and want["S2"][2]["kmax"] == 24 and want["S1_kmax2"][2]["pcg_resumes"] == 30
    assert want["batch_legacy"][0]["pcg_resumes"][1] > 0 and want["G4"][0]["pcg_resumes"] >= 2 and want["G1_kmax3"][0]["pcg_resumes"] == 30
    assert want["big_kmax4"][2]["kmax"] == 4 and want["big"][2]["kmax"] != 28


@pytest.mark.gpu
def test_graph_and_eager_count_the_same_where_the_cache_is_revisited():
    """The recorded cases come back to a cached graph of another kmax than the one captured last (there the parent commit added the wrong
    graph's launch count), and none of them starts a batch without a PCG count to track (there the tree keeps kmax, the parent did not)."""
    eager, graph = from_the_tree(True), from_the_tree(False)
    for case in ("G3_120", "big"):
        assert graph[case][-1]["graph_revisits"] > 0 and eager[case][-1]["graph_revisits"] == 0, case
        assert [r["launches"] for r in graph[case]] == [r["launches"] for r in eager[case]], case
    assert [r["collectives"] for r in graph["big"]] == [r["collectives"] for r in eager["big"]]
    for case in ("G4", "G3_120", "G1_kmax3", "big", "big_kmax4"):
        assert all(r["kmax_kept"] == 0 for r in graph[case] + eager[case]), case
    assert graph["big_kmax4"][-1]["pcg_resumes"] == eager["big_kmax4"][-1]["pcg_resumes"] > 0
