"""CPU: the scan stage's decisions (gamma_amd/csrc/scan_plan.h / .cpp: ScanSwitches, ScanShape -> ScanPlan, the bound feedback's
step) on shapes whose plans follow from the rules by hand -- tests/scan_plan_check.cc, a stand-alone program that links
scan_plan.cpp alone, built by g++ with AddressSanitizer + UBSan and run as a child process.  No GPU, no HIP, no extension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gamma_amd", "csrc")


def test_scan_plan_and_bound_feedback(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "scan_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "scan_plan_check.cc"),
                        os.path.join(CSRC, "scan_plan.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)   # (it clears the switches it reads from its own environment)
    assert r.returncode == 0 and "scan plan ok" in r.stdout, (r.stdout + r.stderr)[-6000:]


def test_the_plan_is_host_code():
    """scan_plan.h / .cpp include nothing of HIP (a host compiler alone builds them), and they are the one place of the scan
    stage that reads the environment: gamma_hip_search.cpp's stage A holds no getenv of a plan switch."""
    for name in ("scan_plan.h", "scan_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "#include \"kernels.h\"" not in text, name
    switches = ("GAMMA_HIP_NO_C8", "GAMMA_HIP_NO_FUSED_IP", "GAMMA_HIP_NO_SCAN_CF", "GAMMA_HIP_SCAN_CF_CODES", "GAMMA_HIP_NO_Q8",
                "GAMMA_HIP_Q8_MINLEN", "GAMMA_HIP_NO_Q8_DEMAND", "GAMMA_HIP_NO_BOUND_FEEDBACK", "GAMMA_HIP_SCAN_G")
    plan = open(os.path.join(CSRC, "scan_plan.cpp")).read()
    for sw in switches:
        assert plan.count('getenv("%s")' % sw) == 1, sw
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".h")) and name != "scan_plan.cpp":
            text = open(os.path.join(CSRC, name)).read()
            for sw in switches:
                assert 'getenv("%s")' % sw not in text, (name, sw)
