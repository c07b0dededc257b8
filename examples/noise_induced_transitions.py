#!/usr/bin/env python
"""Noise-induced transitions: inside the bistable window of the Wagner & Eisenman (2015) model (examples/
equilibrium_branches.py finds it), does weather-like variability push a warm climate onto the cold branch, and how
often?  Every member starts from the warm equilibrium at its forcing F; each member then gets its own realisation of
AR(1) ("red") noise on the forcing, drawn on the device (ebm_set_column_noise, one stream per member), and the ensemble
runs `--years` years.  Printed per F and year: the fraction of members whose annual-mean hemispheric temperature has
fallen below the midpoint between the warm and the cold branch.  With `--every N` the noisy ensemble runs through
EnsembleRun.series instead (ebm_run_series: <T> of every member sampled on the device every N steps) and the script prints,
per F, the quartiles of the FIRST time a member's <T> falls below that midpoint, in years at N * dt resolution.  With
`--until` as well, the same table comes from EnsembleRun.first_passage (ebm_run_until): the level is tested on the device
every N steps and a member that has fallen takes no further step — its state stays that of its crossing — so the table is
the same and the script also prints the share of column-steps that were not taken.  With `--quantiles` the yearly table
is followed, per F, by the profile of T(x) and phi(x) across the members at the end of the run: the ensemble mean beside the
median and the 5-95 % band (EnsembleRun.moments and EnsembleRun.quantiles, both reduced on the device) — where members sit
on both branches the mean describes none of them.  With `--eofs N` it is followed, per F, by the N leading EOFs of T(x) across
the members (EnsembleRun.eofs: the nlat x nlat covariance reduced on the device by ebm_ensemble_covariance, diagonalised on the
host under the grid's trapezoid weights) and the fraction of the variance each explains — with members on two branches the
first EOF is the difference between the branches.

    python examples/noise_induced_transitions.py [--nlat 180] [--nt 2000] [--forcings -2,0,2] [--members 64]
        [--years 20] [--sigma 4.0] [--tau 0.1] [--seed 1] [--max-years 60] [--every 0] [--until] [--quantiles] [--eofs 0]
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
    ap.add_argument("--forcings", default="-2,0,2", help="forcings F (W m^-2) inside the bistable window")
    ap.add_argument("--members", type=int, default=64, help="noise realisations per forcing")
    ap.add_argument("--years", type=int, default=20)
    ap.add_argument("--sigma", type=float, default=4.0, help="stationary standard deviation of the noise (W m^-2)")
    ap.add_argument("--tau", type=float, default=0.1, help="e-folding time of the noise (years)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-years", type=int, default=60, help="spin-up limit of the warm and cold equilibria")
    ap.add_argument("--every", type=int, default=0,
                    help="sample <T> every N steps and print first-passage times (0: the yearly table only)")
    ap.add_argument("--until", action="store_true",
                    help="with --every: stop each member at its first passage (EnsembleRun.first_passage) instead of "
                         "thresholding the whole series")
    ap.add_argument("--until-edge", type=float, default=None, metavar="X",
                    help="with --every: stop each member when its ice edge (phi >= 0.15, walking poleward) has come down to "
                         "x = X (EnsembleRun.first_passage_scalar), and print those first-passage times")
    ap.add_argument("--quantiles", action="store_true",
                    help="after the yearly table: mean, median and 5-95 %% band of T(x) and phi(x) across the members, per F")
    ap.add_argument("--eofs", type=int, default=0, metavar="N",
                    help="after the yearly table: the N leading EOFs of T(x) across the members, per F (0: none)")
    args = ap.parse_args()
    if args.eofs < 0 or args.eofs > args.nlat:
        ap.error("--eofs N needs 0 <= N <= nlat")
    if args.until and not args.every:
        ap.error("--until needs --every N: the level is tested every N steps")
    if args.until_edge is not None and (not args.every or args.until):
        ap.error("--until-edge X needs --every N (the edge is tested every N steps) and excludes --until")
    if args.every < 0 or (args.every and (args.nt * args.years) % args.every):
        ap.error("--every must be positive and divide nt * years")
    pkg = graft.load_package()
    st = pkg.SpaceTime("sin", args.nlat, args.nt, 1)
    par = pkg.default_parameters("MIZ")
    F = np.array([float(v) for v in args.forcings.split(",")])
    nf = len(F)

    # the warm and the cold equilibrium at every F: started far on the warm and on the cold side, spun up
    zero = {k: np.zeros(st.nx) for k in PROG[:-1]}
    far = pkg.EnsembleRun("MIZ", st, par, zero, fcol=np.array([-20.0, 20.0]))
    far.equilibrate(args.max_years)
    ends = far.state(PROG)
    far.close()
    init = {k: np.concatenate([np.tile(ends[k][0], (nf, 1)), np.tile(ends[k][1], (nf, 1))]) for k in PROG}
    branches = pkg.EnsembleRun("MIZ", st, par, init, fcol=np.concatenate([F, F]))
    branches.equilibrate(args.max_years)
    eq = branches.state(PROG)
    cold_T, warm_T = np.split(branches.engine.hemispheric_mean("T"), 2)
    branches.close()
    print("    F   cold <T>  warm <T>")
    for i in range(nf):
        print(f"{F[i]:5.2f}  {cold_T[i]:8.2f}  {warm_T[i]:8.2f}" + ("" if warm_T[i] - cold_T[i] > 0.5 else "   (one branch only)"))

    # the noisy ensemble: member (i, m) starts on the warm branch at F[i] and draws stream i*members + m
    n = args.members
    fcol = np.repeat(F, n)
    init = {k: np.repeat(eq[k][nf:], n, axis=0) for k in PROG}
    run = pkg.EnsembleRun("MIZ", st, par, init, fcol=fcol,
                          noise=dict(sigma=args.sigma, tau=args.tau, seed=args.seed), noise_streams=np.arange(nf * n))
    threshold = np.repeat(0.5 * (cold_T + warm_T), n)
    if args.every and args.until_edge is not None:
        # the transition seen where the model is known for it: the ice edge of a warm-branch member comes down to X
        edge = pkg.scalar_spec(st, "edge_ge", "phi", None, 0.15)
        print(f"\nice edge at the start, per forcing (x): " + " ".join(f"{v:.3f}" for v in run.ice_edge()[::n]))
        fp = run.first_passage_scalar(args.nt * args.years, args.every, edge, level=args.until_edge, direction="down")
        run.close()
        first = np.where(fp["crossed"], fp["samples"] * args.every * st.dt, np.inf)                      # years
        print(f"{nf * n} members ({n} per forcing), noise sigma = {args.sigma} W m^-2, tau = {args.tau} y, the ice edge tested "
              f"every {args.every} steps for {args.years} years; first time it is at or below x = {args.until_edge} (years; inf: never):")
        print("    F   fell   25 %     50 %     75 %")
        for i in range(nf):
            t = first[i * n:(i + 1) * n]
            q = np.quantile(t, [0.25, 0.5, 0.75], method="lower")
            print(f"{F[i]:5.2f}  {np.isfinite(t).mean():5.2f}  " + "  ".join(f"{v:7.3f}" for v in q))
        taken, total = int(fp["samples"].sum()) * args.every, nf * n * args.nt * args.years
        print(f"column-steps taken: {taken} of {total} ({100.0 * (1.0 - taken / total):.1f} % not taken)")
        return
    if args.every:
        if args.until:
            # "<T> < threshold", as the series is thresholded below: at or under the next number down
            fp = run.first_passage(args.nt * args.years, args.every, "T", level=np.nextafter(threshold, -np.inf), direction="down")
            first = np.where(fp["crossed"], fp["samples"] * args.every * st.dt, np.inf)                  # years
            taken = int(fp["samples"].sum()) * args.every
        else:
            T = run.series(args.nt * args.years, args.every, names=("T",))[0]      # [samples, members]
            below = T < threshold
            first = np.where(below.any(axis=0), (below.argmax(axis=0) + 1) * args.every * st.dt, np.inf)    # years
        run.close()
        print(f"\n{nf * n} members ({n} per forcing), noise sigma = {args.sigma} W m^-2, tau = {args.tau} y, <T> sampled every "
              f"{args.every} steps ({args.every * st.dt:.4f} y) for {args.years} years; first time <T> falls below the branches' "
              "midpoint (years; inf: never):")
        print("    F   fell   25 %     50 %     75 %")
        for i in range(nf):
            t = first[i * n:(i + 1) * n]
            q = np.quantile(t, [0.25, 0.5, 0.75], method="lower")
            print(f"{F[i]:5.2f}  {np.isfinite(t).mean():5.2f}  " + "  ".join(f"{v:7.3f}" for v in q))
        if args.until:
            total = nf * n * args.nt * args.years
            print(f"column-steps taken: {taken} of {total} ({100.0 * (1.0 - taken / total):.1f} % not taken)")
        return
    out = run.seasonal_means(args.years, names=("T",))
    profiles = []
    if args.quantiles:
        # per forcing: the members of the other forcings get weight zero (a conditional mean, a conditional quantile)
        for i in range(nf):
            w = (np.arange(nf * n) // n == i).astype(np.float64)
            profiles.append((run.moments(("T", "phi"), w), run.quantiles(("T", "phi"), (0.05, 0.5, 0.95), w)))
    eofs = []
    if args.eofs:
        quad = np.gradient(st.x)                           # trapezoid weights of the grid, up to the halved ends
        quad[[0, -1]] *= 0.5
        for i in range(nf):
            eofs.append(run.eofs("T", args.eofs, (np.arange(nf * n) // n == i).astype(np.float64), quad))
    run.close()
    avgT = out["avg"][0]                                   # [years, members]
    fell = avgT < threshold
    print(f"\n{nf * n} members ({n} per forcing), noise sigma = {args.sigma} W m^-2, tau = {args.tau} y; "
          f"fraction of members on the cold side (annual-mean <T> below the branches' midpoint), by year:")
    print("    F  " + " ".join(f"{y + 1:5d}" for y in range(args.years)))
    for i in range(nf):
        frac = fell[:, i * n:(i + 1) * n].mean(axis=1)
        print(f"{F[i]:5.2f}  " + " ".join(f"{v:5.2f}" for v in frac))
    lats = np.linspace(0, st.nx - 1, min(st.nx, 10)).astype(int)
    for i, (m, q) in enumerate(profiles):
        print(f"\nF = {F[i]:.2f}, end of year {args.years}, across the {n} members:   x     mean     5 %   median    95 %")
        for name in ("T", "phi"):
            for k in lats:
                v = q[name]["value"][:, k]
                print(f"  {name:>3s}  {st.x[k]:5.3f}  {m[name]['mean'][k]:7.3f}  {v[0]:7.3f}  {v[1]:7.3f}  {v[2]:7.3f}")
    for i, e in enumerate(eofs):
        print(f"\nF = {F[i]:.2f}, end of year {args.years}, EOFs of T(x) across the {n} members (explained variance: "
              + ", ".join(f"{v:.3f}" for v in e["explained"]) + "):   x  " + "  ".join(f"EOF {j + 1}" for j in range(args.eofs)))
        for k in lats:
            print(f"       {st.x[k]:5.3f}  " + "  ".join(f"{e['modes'][j, k]:6.3f}" for j in range(args.eofs)))


if __name__ == "__main__":
    main()
