#!/usr/bin/env python3
"""Compare the compiler's resource report of the device code between two trees (RobustOutlierFilter added template
parameters and arguments to k_hist1 / k_hist_refine / k_normal_eq / k_normal_eq_loop: their existing instantiations must
keep their registers, scratch and LDS -- DESIGN.md §3, "RobustOutlierFilter").

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -c \
        -Rpass-analysis=kernel-resource-usage -o /dev/null laser_slam_amd/csrc/lsgpu_icp.hip 2> remarks.txt    # in each tree
    devtools/compare_kernel_resources.py parent/remarks.txt remarks.txt

Kernels are matched by demangled name; template arguments only the newer tree has (HistPlain, the trailing RB = false, the
trailing DENS = false of k_snf_tile / k_snf_fallback) and
the argument lists are dropped first.  Exit status 1 if a kernel both trees have differs in SGPRs, VGPRs, AGPRs, scratch, LDS or
occupancy; kernels only the second tree has are listed with their figures."""
import re
import subprocess
import sys

KEYS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds",
        "Occupancy [waves/SIMD]": "occ"}


def report(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name and m.group(1) in KEYS:
            out[name][KEYS[m.group(1)]] = m.group(2)
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*", "", d)                                   # argument list
        d = d.replace("<lsgpu::HistPlain>", "").replace(", lsgpu::HistPlain>", ">")
        d = re.sub(r"(k_normal_eq_loop<[^,>]+, [^,>]+, [^,>]+), false>", r"\1>", d)
        d = re.sub(r"(k_normal_eq<[^,>]+, [^,>]+, [^,>]+), false>", r"\1>", d)
        d = re.sub(r"(icp_update_lane<[^,>]+), false>", r"\1>", d)
        d = re.sub(r"(k_snf_(?:tile|fallback)<[^,>]+), false>", r"\1>", d)         # DENS = false: the kernels as they were
        res[d] = out[n]
    return res


def main():
    a, b = report(sys.argv[1]), report(sys.argv[2])
    bad = 0
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            print("DIFFERS", k, a[k], "->", b[k])
            bad += 1
    for k in sorted(set(b) - set(a)):
        print("new    ", k, b[k])
    for k in sorted(set(a) - set(b)):
        print("gone   ", k, a[k])
    print(f"{len(set(a) & set(b))} kernels in both reports, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
