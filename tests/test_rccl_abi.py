"""CPU: the part of RCCL's ABI that csrc/gamma_hip_group.cpp writes out by hand (gamma_hip_group_rccl.h: ncclInt8 = 0,
ncclFloat32 = 7, ncclMax = 2, ncclMin = 3 and the nine entries' pointer types -- the library is resolved by name at run time)
against the installed <rccl/rccl.h>: tests/sanitize/rccl_abi_check.cc static_asserts every value and every type, compiled with
-fsyntax-only.  And the stand-in communicator of the sanitizer programs (tests/sanitize/fakerccl) against the same header, which
needs no ROCm: its declarations must be the types the group casts to."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")


def rocm_include():
    for base in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if base and os.path.exists(os.path.join(base, "include", "rccl", "rccl.h")):
            return os.path.join(base, "include")
    return None


def syntax_only(args):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall"] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-6000:]


def test_hand_written_rccl_abi_matches_the_installed_header():
    inc = rocm_include()
    if not inc:
        pytest.skip("rccl/rccl.h is not installed (looked under $ROCM_PATH/include and /opt/rocm/include)")
    syntax_only(["-D__HIP_PLATFORM_AMD__", "-I" + inc, os.path.join(SAN, "rccl_abi_check.cc")])


def test_stand_in_declares_what_the_group_casts_to():
    syntax_only(["-I" + os.path.join(SAN, "fakehip"), os.path.join(SAN, "fakerccl", "fakerccl.cc")])


def test_the_check_would_notice(tmp_path):
    """The same translation unit against a header whose AllReduce lost its reduction argument must NOT compile: the
    static_asserts are looked at, not just parsed."""
    inc = rocm_include()
    if not inc or not shutil.which("g++"):
        pytest.skip("rccl/rccl.h is not installed, or no g++")
    good = open(os.path.join(ROOT, "gamma_amd", "csrc", "gamma_hip_group_rccl.h")).read()
    was = "int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t)"
    assert good.count(was) == 1 and good.count("kNcclMin = 3") == 1
    check = open(os.path.join(SAN, "rccl_abi_check.cc")).read().replace('"../../gamma_amd/csrc/gamma_hip_group_rccl.h"', '"bent.h"')
    for bent in (good.replace(was, "int (*AllReduce)(const void*, void*, size_t, int, void*, hipStream_t)"), good.replace("kNcclMin = 3", "kNcclMin = 2")):
        (tmp_path / "bent.h").write_text(bent)
        (tmp_path / "check.cc").write_text(check)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I" + str(tmp_path), str(tmp_path / "check.cc")],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "static assertion failed" in r.stderr, r.stderr[-3000:]
