"""The rumour tree through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/tree_example.cpp, compiled against the HIP
library and run as a host program; what it prints equals the reference model (tests/tree_model.py) on the oracle for the same
configuration and script."""
import os
import subprocess

import numpy as np
import pytest

from serf_amd import _ffi
from tests._oracle import load_oracle
from tests.tree_model import TreeModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")
KEYS = [0x5A000000 + i for i in range(3)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "tree_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "tree_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_tree_example_compiles(exe):
    assert os.path.exists(exe)


def model_side(n, ticks):
    """serf::Options::lan(n).with_view_slots(64).with_packet_loss(0.25) and the example's script on the oracle with the model."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, fanout=3, view_slots=64, event_ring=512, query_ring=512, retransmit_mult=4,
                                                 probe_interval=5, reap_interval=75, queue_check_interval=150, push_pull_interval=150,
                                                 reconnect_interval=150, ring_overflow=8, tcp_fallback=True, nacks=True, loss=0.25))
    entries = [(_ffi.K_EVENT, key, o.stats(5 + 100 * i).event_time) for i, key in enumerate(KEYS)]
    o.inject(6, _ffi.OP_CRASH, n // 2)
    m = TreeModel(o)
    m.start(entries, 0, ticks)
    for i, key in enumerate(KEYS):
        o.user_event(5 + 100 * i, key, 64)
    m.step(ticks)
    return o, m


@pytest.mark.gpu
def test_cpp_tree_example_prints_what_the_model_says(exe):
    n, ticks = 512, 40
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    o, m = model_side(n, ticks)
    assert lines[0] == ["counts", str(ticks), "0"] and m.count() == (ticks, 0)
    assert lines[1][0] == "sample" and [int(x) for x in lines[1][1:]] == m.samples[-1].tolist()
    summ = m.summary()
    got = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "summary"]
    assert got == summ.view(np.uint64).reshape(len(summ), -1).tolist()
    top = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "top"]
    assert top == m.top(0, 8).view(np.uint32).reshape(8, -1).tolist()
    paths = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "path"]
    assert paths == [[e, m.path(e, n - 1)[1]] + m.path(e, n - 1)[0].tolist() for e in range(3)]
    links = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "link"]
    assert links == m.links(0, 0, 16).view(np.uint32).reshape(16, -1).tolist()
    assert len(lines) == 2 + 3 + 8 + 3 + 16
    # the scenario shows what it is for: under a quarter of the packets lost the events reach nearly everybody through trees several
    # hops deep, each with its origin as the only orphan
    assert (summ["reached"] > n // 2).all() and (summ["depth"] >= 4).all() and summ["orphans"].tolist() == [1, 1, 1]
    assert summ["most_children"].min() >= 2
    o.close()
