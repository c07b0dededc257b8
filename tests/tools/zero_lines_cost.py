#!/usr/bin/env python
"""What zero-line elision (ebm_options.elide_zero_lines) costs on a state that gains nothing from it: 4096 latitudes x 2048
columns, partial ice with warm water in EVERY cell, set through set_field — no KiB of Ei, Ew, h or D is zero, so the eliding
kernel loads and stores everything the plain one does and pays its ballots, its three scalar loads and its flag word on top.

Each measurement is a fresh process (`--child on|off`): handle, state, `--warmup` steps, then `--steps` steps of ebm_run
between two events of the handle's stream.  The child with the option on also reads the flags back: none may be set, before
or after.  The parent runs `--rounds` rounds in alternating order (off on / on off / ...) and prints every figure, the medians
and the spread (max - min over the median) of each mode, and the cost of `on` against `off`.

    python tests/tools/zero_lines_cost.py [--rounds 3] > profiles/rNN_zero_lines_cost.txt"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

NLAT, NCOL, NT = 4096, 2048, 1048576
PROG = ("Ei", "Ew", "h", "D", "phi")


def child(mode, steps, warmup):
    pkg = graft.load_package()
    st = pkg.SpaceTime("sin", NLAT, 2000, 1)
    par = pkg.default_parameters("MIZ")
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), 1.0 / NT, NCOL, device=0,
                     elide_zero_lines=(mode == "on"))
    eng.set_time_table(np.array([(2 * i + 1) / (2.0 * NT) for i in range(4096)]))
    eng.set_column_forcing(np.linspace(-10.0, 10.0, NCOL))
    # half cover of ice one metre thick over water two degrees above freezing, everywhere: phi = -Ei / (Lf h)
    h = np.full((NCOL, NLAT), 1.0)
    state = {"h": h, "phi": np.full_like(h, 0.5), "Ei": -0.5 * par["Lf"] * h, "D": np.full_like(h, 10.0),
             "Ew": np.full_like(h, 2.0 * par["cw"] * 0.5)}
    for k in PROG:
        eng.set_field(k, state[k])
    eng.run(0, warmup, None, False)
    flags_before = int(eng.zero_line_flags()[0].any()) if mode == "on" else 0
    eng.timer_start()
    eng.run(warmup, steps, None, False)
    ms = eng.timer_stop() / steps
    flags_after = int(eng.zero_line_flags()[0].any()) if mode == "on" else 0
    got = eng.get_state(PROG)
    finite = all(bool(np.isfinite(v).all()) for v in got.values())
    nonzero = all(bool((got[k] != 0.0).all()) for k in ("Ei", "Ew", "h", "D"))
    eng.close()
    print(json.dumps({"mode": mode, "ms_per_step": ms, "any_flag_set": flags_before or flags_after, "finite": finite,
                      "every_cell_nonzero": nonzero}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--child", choices=("on", "off"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.warmup)
    ms = {"on": [], "off": []}
    for r in range(args.rounds):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(args.steps),
                                  "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                return out.returncode
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            assert rec["finite"] and rec["every_cell_nonzero"] and not rec["any_flag_set"], rec
            rec["round"] = r + 1
            print(json.dumps(rec), flush=True)
            ms[mode].append(rec["ms_per_step"])
    med = {m: statistics.median(v) for m, v in ms.items()}
    spread = {m: (max(v) - min(v)) / med[m] for m, v in ms.items()}
    cost = med["on"] / med["off"] - 1.0
    print(json.dumps({"median_ms": med, "spread": spread, "cost_of_on": cost,
                      "inside_the_off_spread": abs(cost) <= spread["off"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
