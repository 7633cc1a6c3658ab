"""The detection log through the C++ host wrapper (serf_amd/host/serf.hpp): tests/cpp/detect_example.cpp, compiled against the
HIP library and run as a host program; the log it prints equals the Python binding's for the same configuration."""
import os
import subprocess

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp") / "detect_example"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "detect_example.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    return str(out)


def test_cpp_detect_example_compiles(exe):
    assert os.path.exists(exe)


def python_side(n, ticks):
    """serf::Options::lan(n).with_view_slots(64) and the example's script through the Python binding."""
    g = serf_amd.create(n, fanout=3, view_slots=64, event_ring=512, query_ring=512, retransmit_mult=4, probe_interval=5,
                        reap_interval=75, queue_check_interval=150, push_pull_interval=150, reconnect_interval=150, ring_overflow=8,
                        tcp_fallback=True, nacks=True)
    g.inject(3, _ffi.OP_CRASH, 7)
    g.inject(9, _ffi.OP_CRASH, n // 2)
    g.inject(60, _ffi.OP_REVIVE, 7)
    g.detect_start(0, 1, ticks, 64)
    g.step(20)
    g.leave(11)
    g.step(ticks - 20)
    return g


@pytest.mark.gpu
def test_cpp_detect_example_prints_the_python_bindings_log(exe):
    n, ticks = 4096, 160
    r = subprocess.run([exe, str(n), str(ticks)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    g = python_side(n, ticks)
    hdr, log, opened = g.detect_read(), g.detect_log(), g.detect_open()
    assert lines[0] == ["counts"] + [str(x) for x in g.detect_count() + g.detect_log_count()] and g.detect_count() == (ticks, 0)
    assert lines[1][0] == "header" and [int(x) for x in lines[1][1:]] == hdr[-1:].view(np.uint64).tolist()
    got_log = [[int(x) for x in ln[1:]] for ln in lines[2:] if ln[0] == "episode"]
    got_open = [[int(x) for x in ln[1:]] for ln in lines[2:] if ln[0] == "open"]
    assert len(got_log) + len(got_open) == len(lines) - 2
    assert got_log == log.view(np.uint64).reshape(-1, 8).tolist() and got_open == opened.view(np.uint64).reshape(-1, 8).tolist()
    # the scenario shows what it is for: node 7 is down, returns, is accused behind its return; n / 2 is detected by everybody
    assert len(log) >= 3 and set(log["outcome"].tolist()) >= {_ffi.DETECT_DETECTED, _ffi.DETECT_RETURNED}
    assert (log[log["outcome"] == _ffi.DETECT_RETURNED]["subject"] == 7).all() and n // 2 in log[log["outcome"] == _ffi.DETECT_DETECTED]["subject"].tolist()
