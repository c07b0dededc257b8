#!/usr/bin/env python
"""A bootstrap particle filter on the Wagner & Eisenman (2015) model — a twin experiment.  One member with its own
realisation of AR(1) forcing noise is the "truth".  Every `--every` steps its temperature T(x) is observed at every tenth
latitude with Gaussian noise of standard deviation `--obs-sigma`; an ensemble of `--members` members, each with its own
noise stream, is filtered towards these observations: EnsembleRun.assimilate reduces every member's misfit
J = sum (T - obs)^2 / obs_sigma^2 on the device (ebm_column_misfits), turns the J into likelihood weights
(assimilation_weights) and resamples the members on the device (ebm_resample_columns).  A second ensemble with the same
noise streams runs free.  Printed per observation time: the effective sample size before resampling and the RMS distance
over latitude of the ensemble-mean T(x) to the truth, with and without the filter.

THE NUMBERS ARE ILLUSTRATIONS: one short run with one seed at a small size, not a converged or measured result, and no
statement about the skill of particle filters on this model.

    python examples/particle_filter.py [--nlat 180] [--nt 2000] [--members 64] [--cycles 10] [--every 200]
        [--obs-sigma 0.5] [--sigma 4.0] [--tau 0.1] [--seed 1] [--max-years 60]
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
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--cycles", type=int, default=10, help="observation times")
    ap.add_argument("--every", type=int, default=200, help="steps between two observations")
    ap.add_argument("--obs-sigma", type=float, default=0.5, help="standard deviation of the observation error (K)")
    ap.add_argument("--sigma", type=float, default=4.0, help="stationary standard deviation of the forcing noise (W m^-2)")
    ap.add_argument("--tau", type=float, default=0.1, help="e-folding time of the forcing noise (years)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-years", type=int, default=60, help="spin-up limit of the starting equilibrium")
    args = ap.parse_args()
    pkg = graft.load_package()
    st = pkg.SpaceTime("sin", args.nlat, args.nt, 1)
    par = pkg.default_parameters("MIZ")
    n = args.members

    # every member and the truth start from the equilibrium seasonal cycle at F = 0
    spin = pkg.EnsembleRun("MIZ", st, par, {k: np.zeros(st.nx) for k in PROG[:-1]})
    spin.equilibrate(args.max_years)
    eq = spin.state(PROG)
    spin.close()

    noise = dict(sigma=args.sigma, tau=args.tau, seed=args.seed)
    truth = pkg.EnsembleRun("MIZ", st, par, eq, noise=noise, noise_streams=np.array([n]))
    start = {k: np.repeat(eq[k], n, axis=0) for k in PROG}
    filtered = pkg.EnsembleRun("MIZ", st, par, start, noise=noise, noise_streams=np.arange(n))
    free = pkg.EnsembleRun("MIZ", st, par, start, noise=noise, noise_streams=np.arange(n))

    rng = np.random.default_rng(args.seed)
    seen = np.arange(0, st.nx, 10)                       # T is observed at every tenth latitude
    rms = lambda run, T: float(np.sqrt(np.mean((run.moments("T")["T"]["mean"] - T) ** 2)))
    print("illustration only: one seed, a small ensemble; not a converged or measured result")
    print(" time (yr)     ESS / n   resampled   RMS filtered (K)   RMS free (K)")
    for cycle in range(args.cycles):
        for run in (truth, filtered, free):
            run.run(args.every)
        T = truth.engine.get_field("T")[0]
        obs = np.full((1, st.nx), np.nan)
        obs[0, seen] = T[seen] + rng.normal(0.0, args.obs_sigma, len(seen))
        # a bootstrap filter: resample at every observation (ess_fraction = 1), so that the members stay equally weighted
        res = filtered.assimilate("T", obs, args.obs_sigma ** 2, rng, ess_fraction=1.0)
        assert (res["N"] == len(seen)).all()
        print(f"{(cycle + 1) * args.every * st.dt:10.3f}  {res['ess'] / n:10.3f}  {'yes' if res['parents'] is not None else 'no':>10}"
              f"  {rms(filtered, T):17.4f}  {rms(free, T):13.4f}")
    for run in (truth, filtered, free):
        run.close()


if __name__ == "__main__":
    main()
