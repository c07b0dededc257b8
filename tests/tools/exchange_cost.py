#!/usr/bin/env python
"""What do an export and an import of whole columns cost?  On the two shapes of tests/tools/resample_cost.py (4096 x 2048 MIZ,
the headline state, and 180 x 4096), on one handle in one process, alternating in every round:

  pair       ebm_export_columns of the distinct parents of the moved columns + ebm_import_columns into the moved columns,
             through one device buffer, nothing synchronised between the two (2 launches)
  resample   ebm_resample_columns with the same map (2 x 12 launches; code the parent commit has)
  host       get_state, NumPy gather, set_state of the prognostic fields and T0, plus the noise state (selection map only)

for the maps `shift` (every column moved) and `selection` (about a tenth moved: the selection_parents draw of
resample_cost.py).  Each is the median of `--rounds` rounds timed with ebm_timer_start / ebm_timer_stop (HIP events on the
handle's stream) around the calls; the host route by the wall clock.  Every field is current (a diagnostic step comes first)
and the rows are pair-split, so the pair un-permutes and permutes.  Bytes of the pair: records x record bytes, written once
and read once per importing column.  The all-to-all between shards that the buffer is meant for is NOT measured here: it
needs more than one GPU.  Prints one JSON line per shape.

    python tests/tools/exchange_cost.py [--rounds 7] [--shapes 4096x2048,180x4096] [--out FILE]
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
    import torch
    nt = max(2000, nlat * nlat // 16)
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
    rng = np.random.default_rng(0)
    with eng:
        eng.set_state({k: np.zeros((ncol, nlat)) for k in PROG})
        eng.set_column_forcing(np.linspace(-2.0, 2.0, ncol))
        eng.set_time_table(st.t)
        eng.set_column_noise(np.full(ncol, 1.0), rho=np.full(ncol, 0.9), seed=1)
        R, _ = eng.column_record()
        z, draws = rng.standard_normal(ncol), {}
        for sigma in np.geomspace(0.003, 0.35, 40):
            p = pkg.selection_parents(np.exp(sigma * z), np.random.default_rng(1))
            draws[float(sigma)] = (p, float((p != np.arange(ncol)).mean()))
        sigma = min(draws, key=lambda v: abs(draws[v][1] - 0.10))
        maps = {"shift": (np.arange(ncol) - 1) % ncol, "selection": draws[sigma][0]}
        buf = torch.empty((ncol, R), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        out = dict(nlat=nlat, ncol=ncol, record_doubles=R, rounds=rounds, selection_sigma=sigma)
        step = 0

        def fresh():
            nonlocal step
            eng.run(step, 2, None, True, 1)                       # every field current, the state pair-split
            step += 2
            eng.sync()
        for name, p in maps.items():
            moved = np.flatnonzero(p != np.arange(ncol))
            distinct = np.unique(p[moved])
            records = np.searchsorted(distinct, p[moved])
            pair, whole = [], []
            for _ in range(rounds + 1):                           # the first round warms both up and is dropped
                fresh()
                eng.timer_start()
                mask = eng.export_columns(distinct, buf.data_ptr())
                eng.import_columns(moved, buf.data_ptr(), mask, records)
                pair.append(eng.timer_stop())
                fresh()
                eng.timer_start()
                eng.resample_columns(p)
                whole.append(eng.timer_stop())
            pair, whole = pair[1:], whole[1:]
            nbytes = 8 * R * (2 * len(distinct) + 2 * len(moved))     # export: read + write; import: read + write
            out[name] = dict(moved=int(len(moved)), records=int(len(distinct)), pair_ms=float(np.median(pair)),
                             pair_ms_all=[round(v, 4) for v in pair], resample_ms=float(np.median(whole)),
                             resample_ms_all=[round(v, 4) for v in whole], pair_bytes=nbytes,
                             pair_TBps=nbytes / (float(np.median(pair)) * 1e-3) / 1e12,
                             pair_over_resample=float(np.median(pair) / np.median(whole)))
        p = maps["selection"]
        ms = []
        for _ in range(max(3, rounds // 2)):
            fresh()
            t0 = time.perf_counter()
            state, N = eng.get_state(PROG + ("T0",)), eng.noise_state()
            eng.set_state({k: v[p] for k, v in state.items()})
            eng.set_noise_state(N[p])
            eng.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        out["host"] = dict(ms=float(np.median(ms)), ms_all=[round(v, 2) for v in ms])
        out["host_over_pair_selection"] = out["host"]["ms"] / out["selection"]["pair_ms"]
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
