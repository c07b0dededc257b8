#!/usr/bin/env python
"""Equilibrium branches: the hysteresis of Wagner & Eisenman (2015) without a ramp.  Every member of one ensemble sits at
its own constant forcing F (a per-member offset), half of them started from a warm equilibrium and half from a cold
one, and ebm_equilibrate spins each member up until its seasonal cycle repeats — each member stops at its own year.
Where the warm and the cold member of the same F end in different states, the model has two stable climates there.

    python examples/equilibrium_branches.py [--nlat 180] [--nt 2000] [--fmin -8] [--fmax 8] [--nf 17] [--max-years 60]

Prints, per member, F, the start, the equilibrium year, whether it converged, and the annual-end hemispheric means of
T and of the ice concentration phi.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

PROG = ("Ei", "Ew", "h", "D", "phi", "T0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlat", type=int, default=180)
    ap.add_argument("--nt", type=int, default=2000)
    ap.add_argument("--fmin", type=float, default=-8.0)
    ap.add_argument("--fmax", type=float, default=8.0)
    ap.add_argument("--nf", type=int, default=17)
    ap.add_argument("--max-years", type=int, default=60)
    ap.add_argument("--tol", type=float, default=1e-3, help="absolute tolerance of T between consecutive year ends")
    args = ap.parse_args()
    pkg = graft.load_package()
    st = pkg.SpaceTime("sin", args.nlat, args.nt, 1)
    par = pkg.default_parameters("MIZ")
    tol = {"T": args.tol}

    # the two starting climates: equilibria far on the cold and on the warm side
    zero = {k: np.zeros(st.nx) for k in PROG[:-1]}
    ends = pkg.EnsembleRun("MIZ", st, par, zero, fcol=np.array([args.fmin - 10.0, args.fmax + 10.0]))
    r = ends.equilibrate(args.max_years, tol)
    start = ends.state(PROG)
    ends.close()
    print(f"starting climates: cold after {r['years'][0]} years, warm after {r['years'][1]} years")

    F = np.linspace(args.fmin, args.fmax, args.nf)
    fcol = np.repeat(F, 2)                               # member 2i: cold start at F[i], member 2i+1: warm start
    init = {k: np.tile(start[k], (args.nf, 1)) for k in PROG}
    run = pkg.EnsembleRun("MIZ", st, par, init, fcol=fcol)
    out = run.equilibrate(args.max_years, tol)
    hT, hphi = run.engine.hemispheric_mean("T"), run.engine.hemispheric_mean("phi")
    run.close()
    print(f"{2 * args.nf} members x {args.nlat} latitudes, {args.nt} steps per year; stepped "
          f"{out['years'].sum()} member-years of {2 * args.nf * args.max_years} at most")
    print("    F  start  years conv    <T>    <phi>")
    for m in range(2 * args.nf):
        print(f"{fcol[m]:5.2f}  {'cold' if m % 2 == 0 else 'warm'}  {out['years'][m]:5d}  {int(out['converged'][m]):3d}"
              f"  {hT[m]:6.2f}  {hphi[m]:6.3f}")
    split = [F[i] for i in range(args.nf) if abs(hT[2 * i] - hT[2 * i + 1]) > 0.5]
    print("two equilibria (warm and cold end more than 0.5 degrees apart) at F =", ", ".join(f"{f:.2f}" for f in split) or "none")


if __name__ == "__main__":
    main()
