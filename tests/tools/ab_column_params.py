#!/usr/bin/env python
"""Cost of per-column parameter sets (ebm_set_column_params) on the headline grid, 4096 x 2048 MIZ: milliseconds per step
with no table (the default path), 1, 64 and 2048 distinct sets (D swept), for K = 1 (ebm_run, one launch per step) and
K = 64 (ebm_run_fused).  Every variant starts from the same spun-up state; the variants are taken in turn, `repeats`
rounds, and each prints its median.

    python tests/tools/ab_column_params.py [steps] [repeats]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 256
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nlat, ncol, nt, spinup = 4096, 2048, 1048576, 2000
pkg = graft.load_package()
st = pkg.SpaceTime("sin", nlat, nt, 1)
par = pkg.default_parameters("MIZ")
pv = pkg.engine.param_vector(par, pkg.default_parval)
fcol = 0.5 * np.sin(2.0 * np.pi * np.arange(ncol) / ncol)
iD = pkg.engine.PARAM_ORDER.index("D")


def rows(nsets):
    r = np.tile(pv, (ncol, 1))
    r[:, iD] = pv[iD] * (0.8 + 0.4 * (np.arange(ncol) % nsets) / max(1, nsets - 1))
    return r


eng = pkg.Engine("MIZ", st.grid_kind, st.x, pv, st.dt, ncol, device=0)
eng.set_column_forcing(fcol)
eng.set_time_table(st.t)
eng.run(0, spinup, None, True, 64)
start = eng.get_state(("Ei", "Ew", "h", "D", "phi", "T0"))
variants = [("none", None), ("1", rows(1)), ("64", rows(64)), ("2048", rows(2048))]
times = {(v, K): [] for v, _ in variants for K in (1, 64)}
for rep in range(repeats):
    for K in (1, 64):
        for name, r in variants:
            eng.set_column_params(r)
            eng.set_state(start)
            eng.run(spinup, 64, None, False, K)          # pre-roll: the tables and the state into L2 / MALL
            eng.timer_start()
            eng.run(spinup + 64, steps, None, False, K)
            times[(name, K)].append(eng.timer_stop() / steps)
eng.close()
for (name, K), t in times.items():
    t = sorted(t)
    print(json.dumps({"sets": name, "K": K, "ms_per_step_median": t[len(t) // 2], "min": t[0], "max": t[-1],
                      "steps": steps, "repeats": repeats}))
