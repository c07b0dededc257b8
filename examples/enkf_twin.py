#!/usr/bin/env python
"""An ensemble Kalman filter on the Wagner & Eisenman (2015) model — a twin experiment beside particle_filter.py.  One
member with its own realisation of AR(1) forcing noise is the "truth".  Every `--every` steps its temperature T(x) is
observed at every `--stride`-th latitude with Gaussian noise of standard deviation `--obs-sigma`; an ensemble of `--members`
members, each with its own noise stream, is updated towards these observations by EnsembleRun.enkf: the covariances of T with
itself and of Ei, Ew, h, D, phi with T are reduced on the device (ebm_ensemble_covariance), the gains are formed on the host
from nlat^2 numbers (localised with the Gaspari-Cohn taper, `--localize` in x), and every member is moved on the device by the
gain applied to its own innovation (ebm_update_columns) — no field leaves the device.  Where a particle filter has to
resample whenever its effective sample size collapses, which a whole observed profile makes it do at once, the Kalman update
moves every member.  A second ensemble with the same noise streams runs free.  Printed per observation time: the RMS distance
over latitude of the ensemble-mean T(x) to the truth just BEFORE the analysis (the forecast, which carries the earlier
analyses), with and without the filter, and the forecast spread at the observed cells.

THE NUMBERS ARE ILLUSTRATIONS: one short run with one seed at a small size, not a converged or measured result, and no
statement about the skill of ensemble Kalman filters on this model.

    python examples/enkf_twin.py [--nlat 180] [--nt 2000] [--members 64] [--cycles 10] [--every 200] [--stride 10]
        [--obs-sigma 0.5] [--method denkf|perturbed] [--localize 0.3] [--inflation 1.0] [--sigma 4.0] [--tau 0.1] [--seed 1]
        [--max-years 60]
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
    ap.add_argument("--stride", type=int, default=10, help="T is observed at every stride-th latitude")
    ap.add_argument("--obs-sigma", type=float, default=0.5, help="standard deviation of the observation error (K)")
    ap.add_argument("--method", choices=("denkf", "perturbed"), default="denkf")
    ap.add_argument("--localize", type=float, default=0.3, help="half-width in x of the Gaspari-Cohn taper (0: none)")
    ap.add_argument("--inflation", type=float, default=1.0)
    ap.add_argument("--solver", choices=("host", "device"), default="host",
                    help="where the Kalman gain is formed: numpy.linalg.solve on the host, or ebm_kalman_gain_device")
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
    seen = np.arange(0, st.nx, args.stride)
    rms = lambda run, T: float(np.sqrt(np.mean((run.moments("T")["T"]["mean"] - T) ** 2)))
    print("illustration only: one seed, a small ensemble; not a converged or measured result")
    print(" time (yr)   observed   RMS filtered (K)   RMS free (K)   spread at obs (K)")
    for cycle in range(args.cycles):
        for run in (truth, filtered, free):
            run.run(args.every)
        T = truth.engine.get_field("T")[0]
        obs = np.full(st.nx, np.nan)
        obs[seen] = T[seen] + rng.normal(0.0, args.obs_sigma, len(seen))
        before = rms(filtered, T), rms(free, T)              # T goes stale with the analysis, until the next diagnostic step
        res = filtered.enkf(PROG[:-1], "T", obs, args.obs_sigma ** 2, method=args.method, localize=args.localize or None,
                            inflation=args.inflation, solver=args.solver)
        assert res["observed"] == len(seen) and res["gain_shape"] == (5, st.nx, st.nx)
        print(f"{(cycle + 1) * args.every * st.dt:10.3f}  {res['observed']:9d}  {before[0]:17.4f}  {before[1]:13.4f}  {res['prior']['spread']:18.4f}")
    for run in (truth, filtered, free):
        run.close()


if __name__ == "__main__":
    main()
