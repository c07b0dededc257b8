#!/usr/bin/env python
"""What ebm_equilibrate saves: a 180 x 2000 MIZ ensemble whose members reach their seasonal cycle in different years
(a sweep of D and of the forcing offset, started from the golden mid-year state), spun up once through ebm_equilibrate
and once through ebm_integrate for max_years (lastonly, no outputs: the fused stepping of every year for every member).
Prints one JSON line per tolerance: both times, their ratio, and the ideal ratio sum(Y_c) / (ncol * max_years) — the
fraction of column-years equilibrate actually steps.

    python tests/tools/equilibrate_cost.py [--ncol 4096] [--max-years 40] [--tol 1e-2,1e-3,1e-4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ncol", type=int, default=4096)
    ap.add_argument("--max-years", type=int, default=40)
    ap.add_argument("--tol", default="1e-2,1e-3,1e-4", help="absolute tolerances of T, comma-separated: one run each")
    args = ap.parse_args()
    pkg = __graft_entry__.load_package()
    g = np.load(os.path.join(ROOT, "tests", "golden", "miz_sin_180_2000.npz"))
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    par = pkg.default_parameters("MIZ")
    base = pkg.engine.param_vector(par, pkg.default_parval)
    n = args.ncol
    rows = np.tile(base, (n, 1))
    rng = np.random.default_rng(0)
    rows[:, 0] = base[0] * rng.uniform(0.7, 1.3, n)
    fcol = rng.uniform(-6.0, 6.0, n)
    state = {k: np.tile(np.interp(st.x, g["x"], g[f"s1000_{k}"]), (n, 1)) for k in ("Ei", "Ew", "h", "D", "phi", "T0")}

    def engine():
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, base, st.dt, n, device=0)
        eng.set_column_params(rows)
        eng.set_column_forcing(fcol)
        eng.set_time_table(st.t)
        eng.set_state(state)
        return eng

    tols = [float(t) for t in args.tol.split(",")]
    with engine() as eng:                      # warm-up of both paths (kernels loaded, buffers sized)
        eng.equilibrate(st.nt, 2, None, {"T": tols[0]})
        eng.integrate(st.nt, 1, None, True, st.winter.inx, st.summer.inx, ("T",), want_raw=False, want_seasonal=False,
                      want_avg=False)
    with engine() as eng:
        eng.sync()
        t0 = time.perf_counter()
        eng.integrate(st.nt, args.max_years, None, True, st.winter.inx, st.summer.inx, ("T",), want_raw=False,
                      want_seasonal=False, want_avg=False)
        integrate_s = time.perf_counter() - t0
    for tol in tols:
        out = dict(shape=f"180 x 2000 steps/year x {n} members", max_years=args.max_years, tol_T=tol)
        with engine() as eng:
            eng.sync()
            t0 = time.perf_counter()
            r = eng.equilibrate(st.nt, args.max_years, None, {"T": tol})
            out["equilibrate_s"] = time.perf_counter() - t0
        out["integrate_s"] = integrate_s
        y = r["years"]
        out["converged"] = int(r["converged"].sum())
        out["years_min_median_max"] = [int(y.min()), float(np.median(y)), int(y.max())]
        hist = np.bincount(y, minlength=args.max_years + 1)
        out["active_in_year"] = [int(n - hist[:k].sum()) for k in range(1, args.max_years + 1)]
        out["time_ratio"] = out["equilibrate_s"] / integrate_s
        out["ideal_ratio"] = float(y.sum()) / (n * args.max_years)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
