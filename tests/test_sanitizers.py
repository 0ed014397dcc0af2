"""The plugins' threaded host code under the sanitizers the CPU build has: tests/sanitize/ builds the
RetrievalModel plugins (gamma_amd/host) + the harness on a CPU stub of the C ABI (stub_abi.cpp, backed by the oracle) with
-fsanitize=thread and with -fsanitize=address,undefined, and plugin_stress.cc drives the engine's threading contract
(SURVEY 8b): four client threads searching, the indexing thread growing the store / Add / Update, an API thread deleting.
Any report fails the test.  stress_group_tsan links the REAL csrc/gamma_hip_group.cpp (member threads, barriers, snapshots;
replicate placement) over three stub members, its HIP runtime calls answered by tests/sanitize/fakehip (host memory, copies on
the calling thread).  group_protocol_tsan / group_protocol_asan link it too, in LIST-SHARD placement: group_protocol.cc scripts
the members' list-shard entries (patterns in, patterns checked) and drives the search protocol of both families at W = 2, 3 and
4 members over BOTH transports -- peer copies, and RCCL on tests/sanitize/fakerccl, a stand-in communicator linked into the
program under RCCL's soname, where the members' threads are the ranks: slice offsets, counts, the reduction op, tie rounds, and
a failure injected at every entry x every member, after which the call must return (all members entered a collective, or none)
and the next one succeed.  The stand-in's call counters say after every search which transport carried it, so that no RCCL case
can have run over copies; fakerccl_selftest_* holds the stand-in itself to the rules it enforces (a correct all-gather, min, max
and all-to-all against a plain loop; a wrong count, a misplaced in-place all-gather, a short recv and another reduction each
refused at every rank without hanging).  (The combining queue and the store locks of the device library live in translation
units full of kernel launches: they are exercised by the GPU suites, tests/test_gpu_concurrent.py; GPU sanitizers do not exist
on this pool.  Caller bookkeeping that was moved out of those units is checked on the CPU like the code above: the owners of
device memory by tests/test_dev_mem.py, the completion slots of the _wait entries -- with the interleaving of enqueue, completion
and wait scripted -- by tests/test_call_slots.py.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")
TSAN = ("ThreadSanitizer",)
ASAN = ("AddressSanitizer", "runtime error", "LeakSanitizer")


@pytest.fixture(scope="module")
def built():
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-C", SAN], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return os.path.join(SAN, "_build")


def run(built, binary):
    env = dict(os.environ, OMP_NUM_THREADS="1", TSAN_OPTIONS="halt_on_error=0 second_deadlock_stack=1",
               ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(built, binary)], capture_output=True, text=True, timeout=600, env=env)
    return r, r.stdout + r.stderr


@pytest.mark.parametrize("binary,marks", [("stress_tsan", TSAN),
                                          ("stress_asan", ASAN),
                                          # the REAL in-process group (csrc/gamma_hip_group.cpp: a thread per member, barriers, go / no-go
                                          # snapshots) behind the plugin's "devices" key, on three stub members (fakehip/: its HIP calls)
                                          ("stress_group_tsan", TSAN),
                                          # the same file's list-sharded search protocol on scripted members (group_protocol.cc), over peer
                                          # copies and over the stand-in communicator (fakerccl/): the meeting points ...
                                          ("group_protocol_tsan", TSAN + ("WATCHDOG", "CHECK FAILED", "FAKE RCCL")),
                                          # ... and the buffers the exchanges move rows into
                                          ("group_protocol_asan", ASAN + ("WATCHDOG", "CHECK FAILED", "FAKE RCCL"))])
def test_plugins_under_sanitizer(built, binary, marks):
    r, out = run(built, binary)
    assert r.returncode == 0, out[-4000:]
    for m in marks:
        assert m not in out, out[-6000:]
    assert " 0 failures" in out and " 0 searches" not in out
    if binary.startswith("group_protocol"):   # no plugin behind it: every injected case returned with its error, then recovered
        assert "group_protocol:" in out and "NOT RECOVERED" not in out and "WRONG ANSWER" not in out
        assert out.count("returned with its error") == out.count("\ninject ") > 0
        # both transports at every W, the failure sweep on both at W = 3 (the 201 cases over copies as they have always been; every
        # entry the RCCL path reaches: bound_combine belongs to the copy path), none of it with a stub-side check failed
        last = out.strip().splitlines()[-1]
        for w in (2, 3, 4):
            for transport in ("copies", "rccl"):
                assert "W=%d %s: " % (w, transport) in last, last
        assert "W=3 copies: 70 clean + 201 injected" in last and "W=3 rccl: 72 clean + 144 injected" in last, last
        assert "W=3 rccl-refused: 20 clean + 0 injected" in last and ", 0 stub-side checks failed, 0 failures" in last, last
        assert out.count("\ninject rccl ") == 144 and out.count("\ninject copies ") == 201
        return
    assert "HIPIVFPQ:" in out
    if "group" not in binary:
        assert "HIPFLAT:" in out


@pytest.mark.parametrize("binary,marks", [("fakerccl_selftest_tsan", TSAN), ("fakerccl_selftest_asan", ASAN)])
def test_stand_in_communicator_keeps_its_own_rules(built, binary, marks):
    """Without this a stand-in that checks nothing would make the RCCL cases of group_protocol_* vacuous."""
    r, out = run(built, binary)
    assert r.returncode == 0, out[-4000:]
    for m in marks + ("WATCHDOG", "FAILED"):
        assert m not in out, out[-6000:]
    assert "fakerccl_selftest: " in out and " 0 failures" in out
    for said in ("the ranks disagree in a collective", "not at rank x sendcount", "whose matching send has",
                 "ncclFloat32 with ncclMin / ncclMax only", "named twice"):
        assert "FAKE RCCL: " in out and said in out, said
    assert out.count("\nrefused: ") >= 4


def test_stand_in_is_linked_where_the_loader_looks_first(built):
    """DT_RPATH, not RUNPATH: a RUNPATH entry loses to a ROCm library directory on the loader's configured path, and the program
    would load the real librccl.so.1 (group_protocol.cc refuses to go on then; this says why before it runs)."""
    if not shutil.which("readelf"):
        pytest.skip("no readelf")
    for binary, flavour in (("group_protocol_tsan", "fakerccl_tsan"), ("group_protocol_asan", "fakerccl_asan")):
        dyn = subprocess.run(["readelf", "-d", os.path.join(built, binary)], capture_output=True, text=True, timeout=60).stdout
        assert "Shared library: [librccl.so.1]" in dyn, dyn
        assert "(RPATH)" in dyn and os.path.join(built, flavour) in dyn and "(RUNPATH)" not in dyn, dyn
