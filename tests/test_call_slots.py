"""CPU: the completion slots of the _wait entries (gamma_amd/csrc/call_slots.h / .cpp: the events of the calls in flight, their
pinned overflow words, who owns one when) against the deferring streams of tests/sanitize/fakehip -- tests/sanitize/
call_slots_check.cc, a stand-alone program that links call_slots.cpp alone, built by g++ once with AddressSanitizer + UBSan and
once with ThreadSanitizer and run as a child process.  No GPU, no HIP, no extension."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gamma_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_every_waiter_reads_its_own_call(san, tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "call_slots_check")
    flags = ["-fsanitize=" + san] + (["-fno-sanitize-recover=undefined"] if "undefined" in san else [])
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DFAKEHIP_DEFERRED"] + flags +
                       ["-I", os.path.join(SAN, "fakehip"), "-o", exe, os.path.join(SAN, "call_slots_check.cc"),
                        os.path.join(CSRC, "call_slots.cpp"), "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    m = re.search(r"call slots ok: (\d+) scripted, (\d+) threaded calls, (\d+) mismatches", r.stdout)
    assert m, out[-6000:]
    assert int(m.group(1)) > 1000 and int(m.group(2)) == 1600 and int(m.group(3)) == 0, m.group(0)
    assert "Sanitizer" not in out and "runtime error" not in out, out[-6000:]


def test_call_slots_is_runtime_api_host_code():
    """call_slots.h / .cpp know nothing of the handle or the kernels, and the library's other files keep no completion event or
    overflow word of their own: no slot is picked by a sequence number, the _wait entries go through the pool."""
    for name in ("call_slots.h", "call_slots.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "gamma_hip_internal.h" not in text and "kernels.h" not in text and "__global__" not in text, name
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".h", ".hip")):
            text = open(os.path.join(CSRC, name)).read()
            for gone in ("call_seq", "ev_call", "pin_flat_over"):
                assert gone not in text, (name, gone)
    for name in ("gamma_hip_search.cpp", "gamma_hip_search_flat.cpp"):
        assert "CallTicket" in open(os.path.join(CSRC, name)).read(), name
    assert "call_slots.cpp" in open(os.path.join(CSRC, "Makefile")).read()
