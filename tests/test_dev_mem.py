"""CPU: the owners of device memory (gamma_amd/csrc/dev_mem.h / .cpp: DevBuf, VmRange, DevArray::grow, the arena's column sets)
against the stand-in runtime of tests/sanitize/fakehip -- tests/sanitize/dev_mem_check.cc, a stand-alone program that links
dev_mem.cpp alone, built by g++ with AddressSanitizer + UBSan and run as a child process.  No GPU, no HIP, no extension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gamma_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")


def test_dev_mem_growth_failures_and_ownership(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "dev_mem_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", os.path.join(SAN, "fakehip"), "-o", exe,
                        os.path.join(SAN, "dev_mem_check.cc"), os.path.join(CSRC, "dev_mem.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dev mem ok" in r.stdout, (r.stdout + r.stderr)[-6000:]


def test_dev_mem_is_runtime_api_host_code():
    """dev_mem.h / .cpp know nothing of the handle or the kernels (a host compiler builds them against the stand-in runtime), and
    they are the one place that grows a device array: no other .cpp of the library calls a VmRange member."""
    for name in ("dev_mem.h", "dev_mem.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "gamma_hip_internal.h" not in text and "kernels.h" not in text and "__global__" not in text, name
    for name in os.listdir(CSRC):
        if name.endswith(".cpp") and name != "dev_mem.cpp":
            text = open(os.path.join(CSRC, name)).read()
            for call in (".map_to(", ".unmap_all(", "vm.release(", "hipMemMap(", "hipMemCreate(", "hipMemAddressReserve("):
                assert call not in text, (name, call)
