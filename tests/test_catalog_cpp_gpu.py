"""The rumour catalogue through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/catalog_example.cpp, compiled against the
HIP library and run as a host program; its figures are checked for what the scenario must show."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")
K_EVENT, K_SUSPECT, K_DEAD = 3, 6, 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "catalog_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "catalog_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_catalog_example_compiles(exe):
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_cpp_catalog_example_runs(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    rows = [[int(x) for x in ln.split()] for ln in lines[:ticks]]
    assert [w[0] for w in rows] == list(range(1, ticks + 1)) and not any(w[3] for w in rows)
    assert rows[2][1] == n and rows[3][1] == n - 1 and rows[-1][1] == n - 1               # the crash at tick 3
    assert rows[0][2] == 1 and rows[0][4] == 1 and rows[0][9] == 1 and rows[0][10] > 0   # the event: one identity, queued once, under way
    ids = [[int(x) for x in ln.split()[1:]] for ln in lines[ticks:] if ln.startswith("id ")]
    assert len(ids) == rows[-1][7] == sum(w[4] for w in rows) and rows[-1][8] == 0          # the registry is what the samples appended
    assert ids[0][:2] == [K_EVENT, 0x43415441] and ids[0][3] == 1
    kinds = {(x[0], x[1]) for x in ids}
    assert (K_SUSPECT, 7) in kinds and (K_DEAD, 7) in kinds, "the records about the crashed node, which nobody named"
    assert 8 * n < ids[0][8] <= 16 * n + 64                                               # the event's copies: 16 transmits a node at most
    assert all(x[3] <= x[4] and x[5] >= 1 for x in ids)
    assert sum(w[5] for w in rows) >= sum(w[6] for w in rows) and rows[-1][2] == sum(w[4] + w[6] - w[5] for w in rows)
    now = [ln.split() for ln in lines if ln.startswith("now ")][0]
    assert [int(x) for x in now[1:]] == [rows[-1][0], rows[-1][2], rows[-1][2]]
    led = [ln.split() for ln in lines if ln.startswith("ledger ")][0]
    assert int(led[1]) >= 1 and int(led[2]) == 0
