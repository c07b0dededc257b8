"""Which kernels the library launches, with which workgroup size, grid and LDS: every plan of csrc/ebm_plan.h touched once, at
small shapes, through the public Engine API only — so the same script runs against any build of the library (EBM_LIB) and two
builds can be compared launch for launch.  The kernel families compute the same bits, so only a trace shows which one ran.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/plan_trace.py        (GPU box, nothing else enabled)
    python tests/tools/plan_trace.py summarize DIR > profiles/rNN_plan_trace_X.txt      (anywhere: count, kernel, workgroup, grid, LDS)
    python tests/tools/plan_trace.py compare A.txt B.txt                                (exit status 1 unless equal row for row)

Cases: one-step state, diag and save; deriving and eliding; register fused-K at 180 latitudes; resident by column count
(4 CUs + 7 columns), by size (4096 latitudes) and for the extension; fused integrate at four and at two cells per thread;
classic one-step and fused; every fused case once more with forcing noise installed."""
import csv
import glob
import os
import re
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MIZ_VARS = ("E", "T", "h", "Ei", "Ew", "Ti", "Tw", "D", "phi", "n")


def run():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nt = 16

    def engine(model, nlat, ncol, noise=False, **opt):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        par = pkg.default_parameters("Classic" if model == "Classic" else "MIZ")
        dt = st.dt if model != "MIZ" else 1.0 / max(2000.0, 0.7 * nlat * nlat)
        opt.setdefault("use_graph", False)
        eng = pkg.Engine(model, st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), dt, ncol, device=0, **opt)
        eng.set_column_forcing(np.linspace(-1.0, 1.0, ncol))
        eng.set_time_table((np.arange(nt) + 0.5) * dt)
        if noise:
            eng.set_column_noise(0.5, rho=0.9, seed=7)
        return eng

    def fused(model, nlat, ncol, **opt):            # plain fused stepping, without and with noise
        for noise in (False, True):
            with engine(model, nlat, ncol, noise, **opt) as eng:
                eng.run(0, 8, None, True, steps_per_launch=4)

    def integrate(model, nlat, ncol, **opt):        # the fused stretches with savesol!'s sums, without and with noise
        for noise in (False, True):
            with engine(model, nlat, ncol, noise, integrate_steps_per_launch=4, **opt) as eng:
                eng.integrate(nt, 1, None, True, 3, 9, MIZ_VARS, want_raw=False, want_seasonal=False)

    with engine("MIZ", 180, 2, elide_zero_lines=False) as eng:        # one-step: state (deriving), diag, save
        eng.run(0, 3, None, True)
        eng.integrate(nt, 1, None, False, 3, 9, MIZ_VARS)
    with engine("MIZ", 180, 2, elide_zero_lines=True) as eng:         # ... eliding
        eng.run(0, 3, None, False)
    with engine("MIZ", 180, 2, cells_per_thread=2) as eng:            # ... two cells: never deriving
        eng.run(0, 3, None, True)
    with engine("MIZ_IMEX", 180, 2) as eng:
        eng.run(0, 3, None, True)
    fused("MIZ", 180, 3)                                # registers
    fused("MIZ", 180, 3, cells_per_thread=2)
    fused("MIZ", 1100, 2, cells_per_thread=2)           # 768 threads: registers, noise from memory
    fused("MIZ", 180, 4 * ncu + 7)                      # resident by column count
    fused("MIZ", 4096, 5)                               # resident by size
    fused("MIZ_IMEX", 180, 3)                           # the extension
    integrate("MIZ", 180, 3)
    integrate("MIZ_IMEX", 180, 3)
    integrate("MIZ", 180, 3, cells_per_thread=2)
    with engine("Classic", 180, 2) as eng:
        eng.run(0, 3, None, True)
    fused("Classic", 180, 3)
    torch.cuda.synchronize()


def summarize(directory):
    rows = Counter()
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = re.sub(r"\(.*\)$| \[clone .*\]$", "", r["Kernel_Name"]).replace("void ebm::", "")
            col = lambda *names: next((r[n] for n in names if n in r), "?")      # (the column names of two rocprofv3 versions)
            rows[(name, col("Workgroup_Size_X", "Workgroup_Size"), col("Grid_Size_X", "Grid_Size"),
                  col("LDS_Block_Size", "Group_Segment_Size"))] += 1
    print(f"# {'count':>5s} {'workgroup':>9s} {'grid':>8s} {'LDS B':>7s}  kernel")
    for (name, wg, grid, lds), n in sorted(rows.items()):
        print(f"  {n:5d} {wg:>9s} {grid:>8s} {lds:>7s}  {name}")
    print(f"# dispatches: {sum(rows.values())}, distinct rows: {len(rows)}")


def compare(a, b):
    la, lb = ([l for l in open(p).read().splitlines() if not l.startswith("# rocprof")] for p in (a, b))
    only_a, only_b = sorted(set(la) - set(lb)), sorted(set(lb) - set(la))
    for l in only_a:
        print(f"< {l}")
    for l in only_b:
        print(f"> {l}")
    print(f"# {a} vs {b}: " + ("EQUAL row for row" if la == lb else f"DIFFERENT ({len(only_a)} / {len(only_b)} rows on one side only)"))
    return 0 if la == lb else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["summarize"]:
        summarize(sys.argv[2])
    elif sys.argv[1:2] == ["compare"]:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        run()
