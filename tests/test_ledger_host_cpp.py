"""The host side of the rumour ledger without a device: tests/cpp/ledger_host_check.cpp — the five calls' argument paths with a
null handle and with the handle sim_create refuses — compiled against the HIP library and run with every device hidden.  The same
program is what a sanitizer build of the host side runs (its header says how)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")


def test_ledger_host_paths_without_a_device(tmp_path):
    exe = tmp_path / "ledger_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "ledger_host_check.cpp"), "-L", CSRC, "-lserf_sim",
                           "-Wl,-rpath," + CSRC, "-Wl,-rpath-link,/opt/rocm/lib"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    assert "no handle" in r.stderr
