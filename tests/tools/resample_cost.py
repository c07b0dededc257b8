#!/usr/bin/env python
"""What does a resample cost?  Times ebm_resample_columns on 4096 x 2048 MIZ (the headline state) and on 180 x 4096 against
the route through the host that it replaces, on the same handle in the same process:

  shift      every column moved (the cyclic shift parent[c] = c - 1)
  selection  about 10 % moved: one selection_parents draw from mildly unequal (log-normal) weights, their spread chosen so
             (the share that moves at other spreads is printed too)
  identity   nothing moved (the call returns after reading the map)
  host       get_state, NumPy gather, set_state of the prognostic fields and T0, plus the noise state

Each is the median of `--rounds` rounds, timed with ebm_timer_start / ebm_timer_stop (HIP events on the handle's stream)
around the call plus a sync; the host route by the wall clock, as its transfers are synchronous.  Every field is current
when the device calls run (a diagnostic step comes first), so they move all eleven MIZ fields, the active set and N_c.
Bytes: moved columns x rows per column x row bytes, read and written twice each (stage, scatter).  Prints one JSON line per
shape.

    python tests/tools/resample_cost.py [--rounds 7] [--shapes 4096x2048,180x4096] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import __graft_entry__ as graft  # noqa: E402

PROG = ("Ei", "Ew", "h", "D", "phi")


def measure(pkg, nlat, ncol, rounds):
    nt = max(2000, nlat * nlat // 16)                     # bench.py's steps per year for the headline meridian
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
    rng = np.random.default_rng(0)
    with eng:
        eng.set_state({k: np.zeros((ncol, nlat)) for k in PROG})
        eng.set_column_forcing(np.linspace(-2.0, 2.0, ncol))
        eng.set_time_table(st.t)
        eng.set_column_noise(np.full(ncol, 1.0), rho=np.full(ncol, 0.9), seed=1)
        info = eng.launch_info()
        pitch = info["threads"] * info["cells_per_thread"]
        row_bytes = 11 * pitch * 8 + info["threads"] * 2 + 8          # eleven fields, the active-set row, N_c
        shift = (np.arange(ncol) - 1) % ncol
        # log-normal weights; the spread is searched for (host only) so that about 10 % of the members move: the ascending
        # parents keep a survivor in its slot only while the cumulative weights stay within one slot of the slot index
        z, draws = rng.standard_normal(ncol), {}
        for sigma in np.geomspace(0.003, 0.35, 40):
            p = pkg.selection_parents(np.exp(sigma * z), np.random.default_rng(1))
            draws[float(sigma)] = (p, float((p != np.arange(ncol)).mean()))
        sigma = min(draws, key=lambda v: abs(draws[v][1] - 0.10))
        selection = draws[sigma][0]
        maps = {"shift": shift, "selection": selection, "identity": np.arange(ncol)}
        out = dict(nlat=nlat, ncol=ncol, pitch=pitch, rounds=rounds, selection_sigma=sigma,
                   moved_fraction_at_sigma={f"{v:.3g}": round(draws[v][1], 3) for v in list(draws)[::6]})
        step = 0
        for name, p in maps.items():
            ms = []
            for _ in range(rounds):
                eng.run(step, 2, None, True, 1)                       # every field current, the state pair-split
                step += 2
                eng.sync()
                eng.timer_start()
                eng.resample_columns(p)
                ms.append(eng.timer_stop())
            moved = int((p != np.arange(ncol)).sum())
            med = float(np.median(ms))
            nbytes = 4 * moved * row_bytes
            out[name] = dict(moved=moved, ms=med, ms_all=[round(v, 4) for v in ms], bytes=nbytes,
                             TBps=(nbytes / (med * 1e-3) / 1e12) if moved and med > 0 else None)
        ms = []
        for _ in range(max(3, rounds // 2)):
            eng.run(step, 2, None, True, 1)
            step += 2
            eng.sync()
            t0 = time.perf_counter()
            state, N = eng.get_state(PROG + ("T0",)), eng.noise_state()
            eng.set_state({k: v[selection] for k, v in state.items()})
            eng.set_noise_state(N[selection])
            eng.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        out["host"] = dict(ms=float(np.median(ms)), ms_all=[round(v, 2) for v in ms], fields=6)
        out["host_over_shift"] = out["host"]["ms"] / out["shift"]["ms"]
        out["host_over_selection"] = out["host"]["ms"] / out["selection"]["ms"]
        ms = []
        for _ in range(3):
            eng.sync()
            eng.timer_start()
            eng.run(step, 100, None, False, 1)
            ms.append(eng.timer_stop() / 100)
            step += 100
        out["step_ms"] = float(np.median(ms))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="4096x2048,180x4096", help="nlat x ncol, comma-separated")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    pkg = graft.load_package()
    for shape in args.shapes.split(","):
        nlat, ncol = (int(v) for v in shape.split("x"))
        line = json.dumps(measure(pkg, nlat, ncol, args.rounds))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
