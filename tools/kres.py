#!/usr/bin/env python3
"""Register / scratch / occupancy / LDS report of the library's kernels,
from hipcc's kernel-resource-usage remarks (no GPU needed): the five device
translation units of `make asm`, compiled side by side, one line per kernel
sorted by unit and name, so that two runs compare with diff(1).
usage: python tools/kres.py [name-filter-regex] > report.txt   (takes minutes)"""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM", "/opt/rocm")
UNITS = ["aead_api", "launch_chacha", "launch_aes", "worker", "launch_dh"]


def remarks(unit):
    cmd = [f"{ROCM}/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-I../include",
           "-Icsrc", "--cuda-device-only", "-c", f"csrc/{unit}.hip", "-o", "/dev/null",
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "noise-c_amd"), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{unit}: hipcc failed\n{r.stderr[-2000:]}")
    cur, rows = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*)", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = t.split(":", 1)[1].split(" [")[0].strip()
            rows[cur] = {}
        elif cur and ":" in t:
            k, v = t.split(":", 1)
            rows[cur][k.strip()] = v.split("[")[0].strip()
    return rows


def demangle(names):
    filt = shutil.which("llvm-cxxfilt", path=f"{ROCM}/llvm/bin") or shutil.which("c++filt")
    if not filt or not names:
        return names
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void |\((?:[^()]|\([^()]*\))*\)$", "", n) for n in out[:len(names)]]


def main():
    flt = re.compile(sys.argv[1]) if len(sys.argv) > 1 else None
    with ThreadPoolExecutor(len(UNITS)) as ex:
        reports = list(ex.map(remarks, UNITS))
    for unit, rows in zip(UNITS, reports):
        names = list(rows)
        for n, r in sorted(zip(demangle(names), (rows[k] for k in names)), key=lambda t: t[0]):
            if flt and not flt.search(n):
                continue
            g = lambda k: r.get(k, "?")
            print(f"{unit:13s} vgpr {g('VGPRs'):>4s} scratch {g('ScratchSize [bytes/lane]'):>4s} "
                  f"occ {g('Occupancy [waves/SIMD]')} lds {g('LDS Size [bytes/block]'):>6s}  {n}")


if __name__ == "__main__":
    main()
