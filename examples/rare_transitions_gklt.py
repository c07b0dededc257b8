#!/usr/bin/env python
"""Rare noise-induced transitions by genealogical cloning (Giardina, Kurchan, Lecomte & Tailleur 2011; applied to climate
models by Ragone, Wouters & Bouchet 2018), on the noisy ensemble of examples/noise_induced_transitions.py: every member
starts on the warm branch at forcing F inside the bistable window and draws its own AR(1) noise on the device.

The run is divided into intervals of `--every` steps.  In each, EnsembleRun.series gives every member's <T> on the device;
the member's score is the time integral of <T> over the interval, its weight exp(k * score) with k < 0 — members that cool
are cloned, members that stay warm die (selection_parents), and EnsembleRun.resample copies the survivors' states on the
device (ebm_resample_columns): a clone keeps its slot's noise stream and so parts from its parent at the next step.  The
genealogy and the product of the mean weights stay on the host (gklt_run); at the end every member's line of descent is
re-weighted by exp(-k * its summed score) (gklt_lineage, gklt_estimate), which undoes the tilt: the printed number
estimates the probability, under the UNTILTED dynamics, that <T> falls below the midpoint between the warm and the cold
branch within the horizon.  Beside it: the direct estimate from an untilted run of the same size (k = 0 through the same
code).  The probabilities are illustrations of the method at a few hundred members, not converged numbers.

    python examples/rare_transitions_gklt.py [--nlat 180] [--nt 2000] [--forcing -2] [--members 256] [--years 4]
        [--every 100] [--sample 10] [--k -20] [--sigma 4.0] [--tau 0.1] [--seed 1] [--max-years 60]
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
    ap.add_argument("--forcing", type=float, default=-2.0, help="forcing F (W m^-2) inside the bistable window")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--years", type=int, default=4, help="the horizon")
    ap.add_argument("--every", type=int, default=100, help="steps per selection interval (must divide nt * years)")
    ap.add_argument("--sample", type=int, default=10, help="<T> is sampled every N steps within an interval (must divide --every)")
    ap.add_argument("--k", type=float, default=-20.0, help="tilt per K year of the time-integrated <T>; < 0 favours cooling")
    ap.add_argument("--sigma", type=float, default=4.0, help="stationary standard deviation of the noise (W m^-2)")
    ap.add_argument("--tau", type=float, default=0.1, help="e-folding time of the noise (years)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-years", type=int, default=60, help="spin-up limit of the warm and cold equilibria")
    args = ap.parse_args()
    nsteps = args.nt * args.years
    if args.every < 1 or nsteps % args.every:
        ap.error("--every must be positive and divide nt * years")
    if args.sample < 1 or args.every % args.sample:
        ap.error("--sample must be positive and divide --every")
    pkg = graft.load_package()
    st = pkg.SpaceTime("sin", args.nlat, args.nt, 1)
    par = pkg.default_parameters("MIZ")
    F = args.forcing

    # the warm and the cold equilibrium at F (examples/noise_induced_transitions.py): started far on either side, spun up
    zero = {k: np.zeros(st.nx) for k in PROG[:-1]}
    far = pkg.EnsembleRun("MIZ", st, par, zero, fcol=np.array([-20.0, 20.0]))
    far.equilibrate(args.max_years)
    ends = far.state(PROG)
    far.close()
    branches = pkg.EnsembleRun("MIZ", st, par, ends, fcol=np.array([F, F]))
    branches.equilibrate(args.max_years)
    eq = branches.state(PROG)
    cold_T, warm_T = branches.engine.hemispheric_mean("T")
    branches.close()
    level = 0.5 * (cold_T + warm_T)
    print(f"F = {F}: cold <T> = {cold_T:.2f}, warm <T> = {warm_T:.2f}" + ("" if warm_T - cold_T > 0.5 else "   (one branch only)"))

    n, nint = args.members, nsteps // args.every

    def cloning(k):
        """One ensemble of n members from the warm equilibrium through gklt_run.  Returns the estimate dict, the share of
        members that were replaced per selection and the number of distinct ancestors the final members descend from."""
        run = pkg.EnsembleRun("MIZ", st, par, {name: np.tile(eq[name][1], (n, 1)) for name in PROG}, fcol=np.full(n, F),
                              noise=dict(sigma=args.sigma, tau=args.tau, seed=args.seed), noise_streams=np.arange(n))
        low = []

        def advance(i):
            T = run.series(args.every, args.sample, names=("T",))[0]    # [every / sample, n]: <T>, sampled on the device
            low.append(T.min(axis=0))
            return T.sum(axis=0) * args.sample * st.dt                  # the time integral of <T> over the interval, K year
        out = pkg.gklt_run(advance, run.resample, n, nint, k, np.random.default_rng(args.seed))
        run.close()
        score_sum = pkg.gklt_lineage(out["parents"], out["scores"])
        lowest = pkg.gklt_lineage(out["parents"], np.array(low), np.minimum)
        est = pkg.gklt_estimate((lowest < level).astype(np.float64), score_sum, k, out["log_norm"])
        replaced = float((out["parents"] != np.arange(n)).mean())
        roots = np.arange(n)
        for p in out["parents"][::-1]:
            roots = p[roots]
        return est, replaced, len(np.unique(roots)), float((lowest < level).mean())

    tilted, replaced, roots, share = cloning(args.k)
    direct, _, _, _ = cloning(0.0)
    print(f"{n} members, {args.years} years in {nint} intervals of {args.every} steps, noise sigma = {args.sigma} W m^-2, "
          f"tau = {args.tau} y")
    print(f"cloning with k = {args.k}: {100 * replaced:.1f} % of the members replaced per selection, the final members descend "
          f"from {roots} of the {n} initial ones; {100 * share:.1f} % of the lines fell below <T> = {level:.2f}")
    print(f"P(<T> falls below {level:.2f} within {args.years} years):")
    print(f"  re-weighted cloning estimate  {tilted['estimate']:.3e}   (effective members {tilted['ess']:.1f}, "
          f"raw normalisation {tilted['norm']:.3f})")
    print(f"  direct estimate, k = 0        {direct['estimate']:.3e}   ({int(round(direct['estimate'] * n))} of {n} members)")


if __name__ == "__main__":
    main()
