"""The rumour ledger through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/ledger_example.cpp, compiled against the HIP
library and run as a host program; its figures are checked for what the scenario must show."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "ledger_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "ledger_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_ledger_example_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_ledger_example_runs(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:ticks]]
    assert [w[0] for w in rows] == list(range(1, ticks + 1)) and all(w[2] == 3 for w in rows)
    assert rows[2][1] == n and rows[3][1] == n - 1 and rows[-1][1] == n - 1               # the crash at tick 3
    # the event: behind the first tick its origin alone has it, queued once, and its first packets are under way
    assert rows[0][6:9] == [1, 1, 1] and rows[0][10] > 0
    reach = [w[6] for w in rows]
    assert 1 < reach[4] < reach[9] <= reach[-1] == rows[-1][1]                            # it spreads; in the end everybody running has it
    assert rows[-1][8] == 0 and rows[-1][10] == 0                                         # and nobody carries it any more
    assert all(w[7] <= w[8] <= w[3] and w[10] <= w[4] and w[11] <= w[8] for w in rows)    # holders <= queued <= all queued; in flight <= all in flight
    assert all(w[5] <= w[4] for w in rows)                                                # a counted packet has a record
    sent = sum(w[10] for w in rows)
    assert 8 * n < sent <= 16 * n + 64                                                    # 16 transmits a node at most (and a few of the node that crashes)
    assert max(w[12] for w in rows) > 0 and max(w[13] for w in rows) > 0                  # the crashed node is suspected, then declared dead
    assert rows[-1][12] == 0 and rows[-1][13] == 0
    now = lines[ticks].split()
    assert now[0] == "now" and [int(x) for x in now[1:]] == [rows[-1][0], rows[-1][1], 1, rows[-1][6], rows[-1][8], rows[-1][10]]
    assert lines[ticks + 1].split() == ["sent", str(sent)]
