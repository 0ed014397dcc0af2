#!/usr/bin/env python3
"""Per-kernel resource table of a built libgamma_hip.so, and its difference against a second build.

    python tools/isa_table.py gamma_amd/libgamma_hip.so                       # the table
    python tools/isa_table.py NEW.so --against OLD.so                         # kernels of both, side by side

Reads only: the gfx950 code objects are unbundled into a temporary directory (as tests/test_isa.py does).  Per kernel, from
the code object's metadata note: VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, spilled SGPRs / VGPRs; from the disassembly:
the number of instructions and a hash of the sequence of mnemonics (operands ignored -- kernel-argument offsets may move).
By default the code objects of scan.hip, q8scan.hip, tables.hip and ties.hip (found by a kernel each of them defines)."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MARKERS = ["k_ivfpq_scan_pair", "k_q8_quant", "k_pq_ip_table", "k_tie_replay"]
FIELDS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
          ("scratch", ".private_segment_fixed_size"), ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count")]


def tool(name):
    return os.path.join(LLVM, name)


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy.so")],
                   check=True, capture_output=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    out = []
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        src, dst = os.path.join(tmp, "b%d.bin" % n), os.path.join(tmp, "b%d.co" % n)
        open(src, "wb").write(data[a:b])
        r = subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + src,
                            "--output=" + dst], capture_output=True, text=True)
        if r.returncode == 0 and os.path.getsize(dst) > 0:
            out.append(dst)
    return out


def kernels_of(co):
    """{mangled kernel name: {field: value, 'insns': n, 'hash': h}}"""
    notes = subprocess.run([tool("llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    out, cur = {}, None
    for ln in notes.splitlines():
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- ") and re.match(r"\s{2,4}- \.", ln):   # a new kernel record of amdhsa.kernels
            cur = {}
        if cur is None:
            continue
        key, val = m.group(1), m.group(2)
        if key == ".name":
            out[val] = cur
        for f, k in FIELDS:
            if key == k:
                cur[f] = int(val)
    dis = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    name, seq = None, []

    def close():
        if name in out:
            out[name]["insns"] = len(seq)
            out[name]["hash"] = hashlib.sha1(" ".join(seq).encode()).hexdigest()[:10]
    for ln in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", ln)
        if m:
            close()
            name, seq = m.group(1), []
        elif name and (ln.startswith(" ") or ln.startswith("\t")):
            t = re.sub(r"//.*$", "", ln).split()
            if t:
                seq.append(t[0])
    close()
    return {k: v for k, v in out.items() if "hash" in v}


def table(lib, everything):
    with tempfile.TemporaryDirectory() as tmp:
        ks = {}
        for co in code_objects(lib, tmp):
            k = kernels_of(co)
            if everything or any(any(mk in n for mk in MARKERS) for n in k):
                ks.update(k)
    names = sorted(ks)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")   # (without one: mangled names)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if filt else names
    short = [re.sub(r"\(.*$", "", d).replace("void ", "").replace("gh::", "") for d in dem]
    return {s: ks[n] for s, n in zip(short, names)}


def waves(r):   # waves per SIMD the registers allow (512 VGPRs + AGPRs per lane, allocated in eights, at most 8 waves)
    regs = (r.get("vgpr", 0) + r.get("agpr", 0) + 7) // 8 * 8
    return min(8, 512 // max(8, regs))


def row(r):
    return "%4d %4d %4d %6d %7d %3d %3d %2d %6d %s" % (r.get("vgpr", 0), r.get("agpr", 0), r.get("sgpr", 0), r.get("lds", 0),
                                                       r.get("scratch", 0), r.get("sspill", 0), r.get("vspill", 0), waves(r),
                                                       r["insns"], r["hash"])


HEAD = "vgpr agpr sgpr    lds scratch ssp vsp wv  insns mnemonics "


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib")
    ap.add_argument("--against", help="an older build: kernels present in both are compared")
    ap.add_argument("--all", action="store_true", help="every code object, not only scan / q8scan / tables / ties")
    a = ap.parse_args()
    new = table(a.lib, a.all)
    if not a.against:
        print("%-70s %s" % ("kernel", HEAD))
        for k in new:
            print("%-70s %s" % (k[:70], row(new[k])))
        return 0
    old = table(a.against, a.all)
    same = [k for k in new if k in old and row(new[k]) == row(old[k])]
    diff = [k for k in new if k in old and row(new[k]) != row(old[k])]
    print("# identical in both builds (registers, LDS, scratch, spills, mnemonic sequence): %d kernels" % len(same))
    print("%-70s %s" % ("kernel", HEAD))
    for k in same:
        print("%-70s %s" % (k[:70], row(new[k])))
    print("\n# changed: %d kernels (first line: --against, second line: this build)" % len(diff))
    worse = 0
    for k in diff:
        print("%-70s %s\n%-70s %s" % (k[:70], row(old[k]), "", row(new[k])))
        if waves(new[k]) < waves(old[k]) or new[k].get("scratch", 0) > old[k].get("scratch", 0):
            worse += 1
            print("%-70s ^^^ fewer waves per SIMD or more scratch" % "")
    print("\n# only in --against: %s" % (", ".join(k for k in old if k not in new) or "none"))
    print("# only in this build: %s" % (", ".join(k for k in new if k not in old) or "none"))
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
