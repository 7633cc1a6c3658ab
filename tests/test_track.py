"""Device-resident trackers (include/serf_sim_track.h), the part that needs no GPU: the extension's interface next to the
ABI it must not disturb, and the reference model (tests/track_model.py) against an independent route on the oracle."""
import ctypes as C
import os
import re
import subprocess

import serf_amd
from serf_amd import _ffi
from tests import test_abi
from tests.track_model import TrackModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_HEADER = os.path.join(ROOT, "include", "serf_sim_track.h")

# include/serf_sim.h as it stands: the extension adds nothing to it
ABI_SYMBOLS_15 = (
    "create", "destroy", "set_stream", "join", "leave", "force_leave", "user_event", "query", "inject", "step", "sync", "tick",
    "members", "stats_get", "watch", "drain_events", "state_digest", "dump_state", "convergence", "convergence_many",
    "exchange_bytes", "bind_exchange", "snapshot", "restore", "query_status", "query_responders", "profile", "profile_read",
    "profile_read_stats", "cluster_stats_get", "resident_planes", "bind_exchange2", "bind_exchange3", "exchange_chunks",
    "exchange_layout", "step_begin", "step_chunk", "step_end", "recycle_due", "recycle_scan", "recycle_apply", "pp_due", "pp_plan",
    "pp_export", "pp_merge", "query_filtered", "set_tags", "init_tags", "inject_record", "deliver_message", "user_event_bytes",
    "peek_packet", "suspect_requests", "suspect_export", "suspect_import", "exchange_unique_id", "exchange_init", "exchange_chunk",
    "exchange_wait", "exchange_library", "abi_version", "backend_name")


def track_declared():
    src = re.sub(r"/\*.*?\*/", "", open(TRACK_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_track_header_declares_what_the_binding_binds():
    assert track_declared() == sorted("sim_" + s for s in _ffi.TRACK_SYMBOLS)
    assert len(_ffi.TRACK_SYMBOLS) == 5


def test_hip_library_exports_the_trackers():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in track_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_track_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_trackers and lib.track_version() == 1


def test_the_abi_is_what_it_was(oracle):
    """The trackers are an extension: serf_sim.h, ABI_SYMBOLS and the ABI version do not know them; the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    assert not set(_ffi.TRACK_SYMBOLS) & set(_ffi.ABI_SYMBOLS)
    assert serf_amd.load().abi_version() == 15 and oracle.abi_version() == 15
    assert not oracle.has_trackers and oracle.track_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.TRACK_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)


def test_track_struct_layouts_match_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_track.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %u %u\\n",sizeof(sim_tracker),sizeof(sim_track_result),'
                    "offsetof(sim_tracker,ltime),offsetof(sim_tracker,max_age),offsetof(sim_track_result,peak),"
                    "offsetof(sim_track_result,state),SIM_TRACK_MAX,SIM_TRACK_NEVER);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_ffi.Tracker), C.sizeof(_ffi.TrackResult), _ffi.Tracker.ltime.offset, _ffi.Tracker.max_age.offset,
            _ffi.TrackResult.peak.offset, _ffi.TrackResult.state.offset, _ffi.TRACK_MAX, _ffi.TRACK_NEVER]
    assert got == want
    assert got[:2] == [32, 56]


def test_model_dump_route_equals_oracle_convergence(oracle):
    """Two independent routes to the same count, at every tick of a 4096-node run: the model's (dumps + numpy, with the
    baseline of slot-less subjects carried across a recycling pass) and the oracle's own sim_convergence.  The run has a
    leave, a re-join of the same node and a second leave; a third node crashes, comes back and refutes: once everybody
    holds it Alive again (at incarnation 1) its view slot is recycled and its rumours are answered from the baseline."""
    n = 4096
    sim = _ffi.Sim(oracle, _ffi.make_config(n, fanout=4, view_slots=16, event_ring=64, query_ring=64, probe_interval=5, loss=0.01,
                                            push_pull_interval=150, join_sync=True, recycle_interval=20,
                                            flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT))
    m = TrackModel(sim)
    rumours = []     # (kind, subject, ltime)
    handles = []
    peaks = {}

    def follow(kind, subject, ltime):
        rumours.append((kind, subject, ltime))
        handles.append(m.add(_ffi.rumour_tracker(kind, subject, ltime)))

    sim.inject(5, _ffi.OP_CRASH, 300)
    sim.inject(40, _ffi.OP_REVIVE, 300)
    follow(_ffi.K_JOIN, 300, 1)      # status_time 1 from the baseline on: everybody, whatever the status
    follow(_ffi.K_JOIN, 300, 2)      # nobody, ever
    for t in range(170):
        if t == 3:
            follow(_ffi.K_LEAVE, 100, sim.stats(100).member_time)
            sim.leave(100)
        if t == 12:
            follow(_ffi.K_LEAVE, 2000, sim.stats(2000).member_time)
            sim.leave(2000)
        if t == 50:
            follow(_ffi.K_JOIN, 100, sim.stats(100).member_time)
            sim.join(100, 7)
        m.step(1)
        slot, view, up = m._dumps()
        for r in rumours:
            seen, nup = sim.convergence(*r)
            spec = _ffi.rumour_tracker(*r)
            assert (m.count_view(spec, slot, view, up), int(up.sum())) == (seen, nup), f"tick {t} rumour {r}"
            peaks[r] = max(peaks.get(r, 0), seen)
    cs = sim.cluster_stats()
    assert cs["slots_recycled"] > 0 and 300 in m.base, "the revived node's slot was to be recycled"
    assert m.base[300][1] == 1, "the baseline carried across the pass holds the refuting incarnation"
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    assert peaks.pop((_ffi.K_JOIN, 300, 2)) == 0
    assert all(peaks[r] > n // 2 for r in peaks), peaks      # the rumours did spread
    res = [m.result(h) for h, r in zip(handles, rumours) if r != (_ffi.K_JOIN, 300, 2)]
    assert all(r["first"] != _ffi.TRACK_NEVER and r["p99"] != _ffi.TRACK_NEVER for r in res), res
    assert all(r["first"] <= r["half"] <= r["p90"] <= r["p99"] <= r["all"] for r in res), res
