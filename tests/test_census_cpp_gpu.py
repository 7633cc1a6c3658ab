"""The census through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/census_example.cpp, compiled against the HIP
library and run as a host program; its figures are checked for what the scenario must show."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "census_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "census_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_census_example_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_census_example_runs(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:ticks]]
    assert [w[0] for w in rows] == list(range(1, ticks + 1))
    # running nodes: the crashes at ticks 3 and 9; the member that left has stopped as well by the end
    assert rows[2][1] == n and rows[3][1] == n - 1 and rows[9][1] == n - 2 and rows[-1][1] == n - 3
    assert rows[-1][2] == 3 and all(w[3] == min(w[2], 2) for w in rows)               # three subjects, two records kept
    assert max(w[5] for w in rows) == 2 and rows[-1][5] == 0 and rows[-1][6] == 3     # held Alive at first, all three known gone in the end
    assert min(w[4] for w in rows[9:]) == 0 and rows[-1][4] >= 2                      # disagreement, then agreement
    now = lines[ticks].split()
    assert now[0] == "now" and [int(x) for x in now[1:]] == rows[-1][:3] + [3] + rows[-1][4:]
    subj = [ln.split() for ln in lines[ticks + 1:]]
    assert [(s[1], s[3]) for s in subj] == [("7", "0"), (str(n // 2), "1"), ("11", "2")]
    assert [s[5] for s in subj] == ["0", "0", "0"] and subj[0][7] == subj[1][7] == str(n - 3) and subj[2][9] == str(n - 3)
