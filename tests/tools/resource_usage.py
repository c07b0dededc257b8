#!/usr/bin/env python
"""Register / scratch / LDS usage of every kernel of the library, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks (cross-compiles for gfx950 without a GPU).

    python tests/tools/resource_usage.py [-D...] > profiles/rNN_resource_usage.txt

Every kernel translation unit of csrc/ (*.hip except the four host units, HOST_UNITS) is compiled with the Makefile's flags; the remarks
of all of them go into one sorted table.  EBM_KERNEL_SRC names another directory of sources.
One line per kernel instantiation: name, VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy.
Exit status 1 if any kernel of the shipped library uses scratch (register spills), 2 if a translation unit does not
compile or a kernel comes out of two of them."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.environ.get("EBM_KERNEL_SRC") or os.path.join(ROOT, "energybalancemodel.jl_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17"]
HOST_UNITS = ("ebm_runtime.hip", "ebm_fields.hip", "ebm_columns.hip", "ebm_drive.hip")      # no kernels: the host runtime


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                         capture_output=True, check=True).stdout.splitlines()
    return [re.sub(r"\(ebm::\w+\)|\(ebm::\w+ const\)|\(.*\)$", "", n).replace("void ebm::", "") for n in out]


def remarks(unit, extra):
    """The resource-usage remarks of one translation unit: [{name, VGPRs, ...}], or the compiler's stderr if there are none."""
    cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + ["-c", os.path.join(SRC, unit), "-o", os.devnull,
                                             "-Rpass-analysis=kernel-resource-usage"] + extra
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: .*?(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            cur = {"name": val, "unit": unit}
            rows.append(cur)
        elif cur is not None:
            cur[key.split(" ")[0]] = val
    return rows or err


def main():
    extra = [a for a in sys.argv[1:] if a.startswith("-")]
    units = sorted(f for f in os.listdir(SRC) if f.endswith(".hip") and f not in HOST_UNITS)
    with ThreadPoolExecutor(max_workers=6) as pool:
        per_unit = list(pool.map(lambda u: remarks(u, extra), units))
    rows, seen = [], {}
    for unit, got in zip(units, per_unit):
        if isinstance(got, str):
            sys.stderr.write(f"{unit}: no kernel remarks\n{got}")
            return 2
        for r in got:
            if r["name"] in seen:
                sys.stderr.write(f"{r['name']} comes out of both {seen[r['name']]} and {unit}\n")
                return 2
            seen[r["name"]] = unit
        rows += got
    names = demangle([r["name"] for r in rows])
    bad = 0
    print(f"# {' '.join(FLAGS + extra)} -Rpass-analysis=kernel-resource-usage: {' '.join(units)}")
    print(f"{'kernel':58s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'scratch B/lane':>15s} {'waves/SIMD':>11s}")
    for r, n in sorted(zip(rows, names), key=lambda t: t[1]):
        sc = int(r.get("ScratchSize", 0))
        bad += sc > 0
        print(f"{n:58s} {r.get('VGPRs', '?'):>5s} {r.get('AGPRs', '?'):>5s} {r.get('TotalSGPRs', '?'):>5s} "
              f"{sc:>15d} {r.get('Occupancy', '?'):>11s}")
    print(f"# kernels: {len(rows)}, with scratch: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
