"""The query board through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/qboard_example.cpp, compiled against the HIP
library and run as a host program; what it prints equals the reference model (tests/qboard_model.py) on the oracle for the same
configuration and script."""
import os
import subprocess

import numpy as np
import pytest

from serf_amd import _ffi
from tests._oracle import load_oracle
from tests.qboard_model import OPEN, WAITING, QBoardModel, Script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")
IDS = [0x51, 0x52, 0x53]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "qboard_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "qboard_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_qboard_example_compiles(exe):
    assert os.path.exists(exe)


def model_side(n, ticks):
    """serf::Options::lan(n).with_view_slots(64).with_packet_loss(0.25) and the example's script on the oracle with the model."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, fanout=3, view_slots=64, event_ring=512, query_ring=512, retransmit_mult=4,
                                                 probe_interval=5, reap_interval=75, queue_check_interval=150, push_pull_interval=150,
                                                 reconnect_interval=150, ring_overflow=8, tcp_fallback=True, nacks=True, loss=0.25))
    sc = Script(o)
    m = QBoardModel(o, sc)
    m.start(IDS, 0, 1, ticks)
    sc.query(0, 5, 0x51, _ffi.F_ACK | _ffi.F_RESPOND | (2 << 8))
    sc.query(0, 105, 0x52, _ffi.F_ACK, ids=[1, 2, 3, n // 2])
    sc.inject(6, _ffi.OP_CRASH, n // 2)
    m.step(ticks)
    return o, m


def as_words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1).tolist()


@pytest.mark.gpu
def test_cpp_qboard_example_prints_what_the_model_says(exe):
    n, ticks = 512, 40
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    o, m = model_side(n, ticks)
    assert lines[0] == ["counts", str(ticks), "0"] and m.count() == (ticks, 0)
    assert lines[1][0] == "sample" and [int(x) for x in lines[1][1:]] == m.samples[-1].tolist()
    hdr, rec = m.now(IDS[::-1])
    assert lines[2][0] == "now" and [int(x) for x in lines[2][1:]] == as_words(hdr) + as_words(rec)
    silent = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "silent"]
    assert silent == [[e, which, m.silent(e, which)[1]] + m.silent(e, which, 8)[0].tolist() for e in range(3) for which in (0, 1)]
    top = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "top"]
    assert top == np.ascontiguousarray(m.top(8)).view(np.uint64).reshape(8, -1).tolist()
    nodes = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "node"]
    assert nodes == np.ascontiguousarray(m.nodes(0, 16)).view(np.uint64).reshape(16, -1).tolist()
    assert len(lines) == 3 + 6 + 8 + 16
    # the scenario shows what it is for: under a quarter of the packets lost, with two relays, nearly everybody's ack arrives but
    # not everybody's; the crashed node of the second query stays out of `eligible`; the third id is never seen
    last = m.read()[1][-1]
    assert last["state"].tolist() == [OPEN, OPEN, WAITING] and n * 9 // 10 < last["answered"][0] < last["eligible"][0] == n - 1
    assert last["eligible"][1] == 3 and last["t_90"][0] > last["t_half"][0] > last["t_first"][0] > 0 and last["t_all"][0] == 0
    o.close()
