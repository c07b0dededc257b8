#!/usr/bin/env python
"""What a time series of hemispheric means costs (ebm_run_series), on one handle and from one start state per workload:
  (a) series  ebm_run_series
  (b) loop    the host loop written with the calls the library had before: ebm_run_fused for `every` steps with diag_last,
              then ebm_hemispheric_mean per variable (a stream synchronisation, a blocking copy and one launch each)
  (c) plain   ebm_run_fused of the same steps without sampling
Workloads: `ensemble` = 180 latitudes x 4096 members with forcing noise, nt = 2000, a year sampled every 20 steps, T and phi;
`long` = 1024 latitudes x 512 columns sampled every 64 steps, all ten variables.  One warm-up of each mode, then `--rounds`
rounds in rotating order; medians and the spread (min ... max) of each mode, (a)/(b) and (a)/(c).  (a) and (b) are also
compared bit for bit.

    python tests/tools/series_cost.py [--rounds 5] > profiles/r10_series_cost.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

PROG = ("Ei", "Ew", "h", "D", "phi")
ALL = PROG + ("Tw", "Ti", "n", "E", "T")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default="ensemble,long")
    args = ap.parse_args()
    pkg = graft.load_package()
    print(f"# library: {os.environ.get('EBM_LIB') or pkg.LIB_PATH}")
    for case in args.cases.split(","):
        if case == "ensemble":
            nlat, ncol, nt, every, nsteps, names, noisy, spin = 180, 4096, 2000, 20, 2000, ("T", "phi"), True, 1000
        else:
            nlat, ncol, nt, every, nsteps, names, noisy, spin = 1024, 512, 262144, 64, 1024, ALL, False, 512
        K = 64
        st = pkg.SpaceTime("sin", nlat, nt, 1)
        par = pkg.default_parameters("MIZ")
        e = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0)
        e.set_column_forcing(0.5 * np.sin(2.0 * np.pi * np.arange(ncol) / ncol))
        e.set_time_table(st.t)
        if noisy:
            e.set_column_noise(0.5, 0.9, seed=7)
        e.run(0, spin, None, diag_last=True, steps_per_launch=K)         # away from the all-zero start: ice and open water
        start = e.get_state(PROG + ("T0",))
        nstate = e.noise_state()

        def restore():
            e.set_state(start)
            if noisy:
                e.set_noise_state(nstate)
            e.sync()

        def series():
            return e.run_series(spin, nsteps, every, names, None, K)

        def loop():
            out = np.empty((len(names), nsteps // every, ncol))
            for j in range(nsteps // every):
                e.run(spin + j * every, every, None, diag_last=True, steps_per_launch=K)
                for v, n in enumerate(names):
                    out[v, j] = e.hemispheric_mean(n)
            return out

        def plain():
            e.run(spin, nsteps, None, diag_last=True, steps_per_launch=K)
            e.sync()

        modes = {"series": series, "loop": loop, "plain": plain}
        got = {}
        for m, fn in modes.items():                                       # warm-up, and the bits of (a) against (b)
            restore()
            got[m] = fn()
        same = np.array_equal(got["series"].view(np.uint64), got["loop"].view(np.uint64))
        res = {m: [] for m in modes}
        order = list(modes)
        for r in range(args.rounds):
            for m in order[r % 3:] + order[:r % 3]:
                restore()
                t0 = time.perf_counter()
                modes[m]()
                res[m].append((time.perf_counter() - t0) * 1e3)
        med = {m: statistics.median(v) for m, v in res.items()}
        print(f"{case}: {nlat} x {ncol}, {nsteps} steps, every {every}, {len(names)} variables, {K} steps per launch"
              f"{', noise' if noisy else ''}; series == loop bit for bit: {same}")
        for m in modes:
            print(f"  {m:6s} median {med[m]:9.3f} ms   min {min(res[m]):9.3f}   max {max(res[m]):9.3f}   "
                  f"{['%.3f' % v for v in res[m]]}")
        print(f"  series/loop {med['series'] / med['loop']:.4f}   series/plain {med['series'] / med['plain']:.4f}   "
              f"spread of loop {(max(res['loop']) - min(res['loop'])) / med['loop']:.4f}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
