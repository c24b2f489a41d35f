"""The item order of the queued lookup's class queues, on the host (csrc/et_lookup_order.h).

tests/lookup_order_host.cpp is a stand-alone program (its own main, nothing loaded into Python)
that includes the header the kernel uses.  It is compiled here with AddressSanitizer and
UndefinedBehaviorSanitizer and run once.  For ntables 2..32, nheavy 0..ntables, stripe_chunks in
{1, 2, 3, 65, 128}, both maps (tables fastest, table-major) in either segment and every policy's
host ordering it asserts that, per XCD, the claims h = 0 .. nk * sc - 1 of the two classes together
hit every slot j * ntables + k exactly once, that h >= nk * sc yields the "none" value, and that
every XCD's entry list is a permutation, class by class, of what the stripe placement assigns
(placement unchanged)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "embeddingtables.jl_amd", "csrc")
SRC = os.path.join(REPO, "tests", "lookup_order_host.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("order") / "lookup_order_host")
    # the sanitizer runtimes are linked in statically, so the program runs whatever else the
    # environment preloads
    subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-pthread", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", f"-I{CSRC}", SRC, "-o", exe],
                   check=True)
    return exe


def test_maps_and_orderings_under_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout[-500:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_header_is_plain_cxx():
    """No HIP types or headers: a host compiler must be able to include it."""
    text = open(os.path.join(CSRC, "et_lookup_order.h")).read()
    assert "hip/" not in text and "hipStream" not in text and "dim3" not in text
