"""The member gazette through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/gazette_example.cpp, compiled against the
HIP library and run as a host program; its figures are checked for what the scenario must show.  build() compiles the example
too (serf_amd/host/gazette_example); the test compiles its own copy, so that it also runs on a tree that was built by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "gazette_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "gazette_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_gazette_example_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_gazette_example_runs(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:ticks]]
    assert [w[0] for w in rows] == list(range(1, ticks + 1))
    assert rows[2][1] == n and rows[3][1] == n - 1 and rows[9][1] == n - 2               # the crashes at ticks 3 and 9
    assert rows[-1][2] == 3 and sum(w[3] for w in rows) == 3                             # three subjects, each fresh once
    sums = [sum(w[4 + k] for w in rows) for k in range(7)]                               # join .. cleared
    assert sums[2] > 0 and sums[5] > 0, "two crashed nodes: suspected, then announced Failed"
    assert sums[4] <= sums[0] and all(w[11] <= w[1] and w[12] <= w[2] for w in rows)
    nodes = [int(x) for x in [ln for ln in lines if ln.startswith("nodes ")][0].split()[1:]]
    subj = [int(x) for x in [ln for ln in lines if ln.startswith("subjects ")][0].split()[1:]]
    assert nodes[0] == subj[0] == n and nodes[1] == subj[1] == sums[2] and nodes[2] == subj[2] == sums[1]
    assert 1 <= nodes[3] <= 3                                                            # a node's events in one sample: three subjects
    top = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("top ")]
    assert len(top) == 3 and {top[0][0], top[1][0]} == {7, n // 2} and top[0][1] >= top[1][1] > 0
    assert top[0][1] + top[1][1] + top[2][1] <= sums[2] and top[2][1] <= top[1][1]
    assert all(1 <= t[2] <= t[1] for t in top[:2])
