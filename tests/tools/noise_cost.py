#!/usr/bin/env python
"""ms per step with and without the per-column forcing noise (ebm_set_column_noise) on three cases, on one handle each:
the 4096 x 2048 headline (one launch per step), the 180-band single meridian fused 64 steps per launch (two cells per
thread: latency-bound) and a year of ebm_integrate_hemispheric on 1024 x 2048 (64 steps per launch).  Alternates off / on
for `--rounds` rounds and prints the medians.

    python tests/tools/noise_cost.py [--rounds 3] > profiles/r07_noise_cost.txt
EBM_LIB=... selects another build of the library (the A/B of the fused kernels' two ways of drawing the innovations)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def engine(pkg, nlat, ncol, nt, **opt):
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    par = pkg.default_parameters("MIZ")
    e = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0, **opt)
    e.set_column_forcing(0.5 * np.sin(2.0 * np.pi * np.arange(ncol) / max(ncol, 2)))
    e.set_time_table(st.t)
    return st, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="headline,band180,integrate")
    args = ap.parse_args()
    pkg = graft.load_package()
    print(f"# library: {pkg.LIB_PATH if not os.environ.get('EBM_LIB') else os.environ['EBM_LIB']}")
    cases = args.cases.split(",")
    for case in cases:
        if case == "headline":
            st, e = engine(pkg, 4096, 2048, 1048576)
            nsteps, spl, spin = 100, 1, 200
        elif case == "band180":
            st, e = engine(pkg, 180, 1, 2000, cells_per_thread=2)
            nsteps, spl, spin = 4096, 64, 2000
        else:
            st, e = engine(pkg, 1024, 2048, 65536)
            nsteps, spl, spin = st.nt, None, 256
        clock = [0]

        def go(n):
            if spl is None:
                e.set_step_clock(clock[0])
                e.integrate_hemispheric(st.nt, 1, None, st.winter.inx, st.summer.inx, ("T",))
            else:
                e.run(clock[0], n, None, diag_last=False, steps_per_launch=spl)
            clock[0] += n

        if spl is None:
            e.run(0, spin, None, diag_last=False, steps_per_launch=64)
            clock[0] = st.nt                                    # integrate starts a year
        else:
            go(spin)
        e.sync()
        res = {"off": [], "on": []}
        for r in range(args.rounds):
            for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
                if mode == "on":
                    e.set_column_noise(0.5, 0.9, seed=7)
                else:
                    e.set_column_noise(None)
                e.sync()
                t0 = time.perf_counter()
                go(nsteps)
                e.sync()
                res[mode].append((time.perf_counter() - t0) * 1e3 / nsteps)
        off, on = statistics.median(res["off"]), statistics.median(res["on"])
        print(f"{case}: ms/step off {off:.5f} {['%.5f' % v for v in res['off']]}  on {on:.5f} {['%.5f' % v for v in res['on']]}"
              f"  on/off {on / off:.4f}", flush=True)
        e.close()


if __name__ == "__main__":
    main()
