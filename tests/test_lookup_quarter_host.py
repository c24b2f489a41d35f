"""Quartered entries of the pooled lookup's stripe map, on the host (csrc/et_lookup_order.h,
DESIGN §4 "Column quarters").

tests/lookup_quarter_host.cpp is a stand-alone program (its own main, nothing loaded into Python)
that includes the header the kernel uses.  It is compiled here with AddressSanitizer and
UndefinedBehaviorSanitizer and run once.  For ntables 2..32, every number of quartered tables among
them in either class, stripe_chunks in {1, 2, 3, 65, 128}, rounds in {1, 8} and batch sizes around
every boundary it asserts that every XCD has one entry per table, that the eight (quarter, half)
pairs of a quartered table have one owner each, that every (bag, quarter) of a quartered table and
every (bag, whole row) of the others is covered exactly once, and that without quartered tables the
entries are those of the placement as it was."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "embeddingtables.jl_amd", "csrc")
SRC = os.path.join(REPO, "tests", "lookup_quarter_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("quarter") / "lookup_quarter_host")
    # the sanitizer runtimes are linked in statically, so the program runs whatever else the
    # environment preloads
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", f"-I{CSRC}", SRC, "-o", exe],
                   check=True)
    return exe


def test_quartered_placement_and_coverage_under_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 50000, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
