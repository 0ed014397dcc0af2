"""CPU: the IVFFLAT scan stage's decisions (gamma_amd/csrc/ivfflat_plan.h / .cpp: IvfflatSwitches, the list-major shape functions,
IvfflatScanShape -> IvfflatScanPlan) on chunks whose plans follow from the table by hand -- tests/ivfflat_plan_check.cc, a
stand-alone program that links ivfflat_plan.cpp alone, built by g++ with AddressSanitizer + UBSan and run as a child process.
No GPU, no HIP, no extension."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gamma_amd", "csrc")


def test_ivfflat_scan_plan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "ivfflat_plan_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "ivfflat_plan_check.cc"),
                        os.path.join(CSRC, "ivfflat_plan.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-6000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)   # (it sets and clears the switches in its own environment)
    assert r.returncode == 0 and "ivfflat plan ok" in r.stdout, (r.stdout + r.stderr)[-6000:]


def test_the_plan_is_host_code():
    """ivfflat_plan.h / .cpp include nothing of HIP (a host compiler alone builds them), and ivfflat_plan.cpp is the one place of
    csrc/ that reads the two switches from the environment."""
    for name in ("ivfflat_plan.h", "ivfflat_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "#include \"kernels.h\"" not in text, name
    switches = ("GAMMA_HIP_NO_IVFFLAT_LM", "GAMMA_HIP_NO_SMALL_PATH")
    plan = open(os.path.join(CSRC, "ivfflat_plan.cpp")).read()
    for sw in switches:
        assert plan.count('getenv("%s")' % sw) == 1, sw
    for name in os.listdir(CSRC):
        if name.endswith((".cpp", ".hip", ".h")) and name != "ivfflat_plan.cpp":
            text = open(os.path.join(CSRC, name)).read()
            for sw in switches:
                assert 'getenv("%s")' % sw not in text, (name, sw)


def test_two_scan_launch_entries_and_no_removed_name():
    """kernels.h declares the pair entry and the list-major entry (and launch_masked_list_len), nothing else of that family; the
    launchers they replaced are named nowhere in the package."""
    text = open(os.path.join(CSRC, "kernels.h")).read()
    decl = re.findall(r"^(?:void|bool|int)\s+(launch_ivfflat_\w+)\s*\(", text, flags=re.M)
    assert sorted(decl) == ["launch_ivfflat_lm", "launch_ivfflat_pair"], decl
    assert len(re.findall(r"^void\s+launch_masked_list_len\s*\(", text, flags=re.M)) == 1
    gone = ("launch_ivfflat_scan_sparse", "launch_ivfflat_lm_sparse", "launch_ivfflat_lm_tail", "launch_ivfflat_scan_t",
            "ivfflat_shard_scan")
    for base, _, files in os.walk(os.path.join(ROOT, "gamma_amd")):
        for f in files:
            if f.endswith((".cpp", ".hip", ".h", ".cc", ".py")) or f == "Makefile":
                body = open(os.path.join(base, f), errors="replace").read()
                for name in gone:
                    assert name not in body, (os.path.join(base, f), name)
