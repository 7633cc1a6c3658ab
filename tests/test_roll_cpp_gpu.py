"""The observer roll through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/roll_example.cpp, compiled against the HIP
library and run as a host program; its figures are checked for what the scenario must show."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "roll_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "roll_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_roll_example_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_roll_example_runs(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:ticks]]
    assert [w[0] for w in rows] == list(range(1, ticks + 1))
    # running nodes: the crashes at ticks 3 and 9; the member that left has stopped as well by the end
    assert rows[2][1] == n and rows[3][1] == n - 1 and rows[9][1] == n - 2 and rows[-1][1] == n - 3
    assert rows[-1][2] == 3 and all(w[4] == 2 for w in rows)                          # three subjects; ranked by MISSED
    # behind the first crash every running node holds one stopped member Alive: 4 095 holders, the four lowest ids listed
    assert rows[3][7:] == [n - 1, n - 1, 0] and rows[3][3] == 4
    assert rows[9][8] > rows[9][7] > 0                                                # two stopped members held Alive by some
    assert rows[-1][7:] == [0, 0, -1] and rows[-1][3] == 0                            # all three known gone in the end
    assert max(w[6] for w in rows) > 0 and all(w[5] <= w[1] and w[6] >= w[1] - w[5] for w in rows)   # some fall behind; the current ones are observers
    assert rows[0][5:7] == [n, 0]                                                     # before anything happens everybody is current
    now = lines[ticks].split()
    assert now[0] == "now" and [int(x) for x in now[1:]] == rows[-1]
    assert lines[ticks + 1].split() == ["nodes", str(n), str(n - 3), "0"]
