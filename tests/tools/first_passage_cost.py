#!/usr/bin/env python
"""What stopping each member at its first passage saves and costs (ebm_run_until), on the noisy ensemble of
examples/noise_induced_transitions.py in small: 180 latitudes x `--members` members with AR(1) forcing noise (sigma 4 W m^-2,
tau 0.1 y), nt = 2000, started from one spun-up state, <T> tested every `--every` steps over `--steps` steps against one
level for all members — the lower quartile of all the <T> the ensemble samples over the horizon, going down — so that
members fall at different times.  One EnsembleRun, restored before every timed call:
  (a) series   EnsembleRun.series over the whole horizon (every member steps every step; thresholding is the host's)
  (b) until    EnsembleRun.first_passage with that level
  (c) never    EnsembleRun.first_passage with the level -inf: every member steps every round, so (c) takes the steps of (a)
               round by round, plus a check, a compaction and a stream synchronisation per round
  (d) rounds   the same rounds as plain EnsembleRun.run calls of `every` steps (diag_last), one synchronisation at the end
Reported: wall time (median, min, max of `--rounds` rounds in rotating order after one warm-up of each), the column-steps
taken by (a) and (b), and ((c) - (d)) / rounds: the time per round spent in check + compaction + synchronisation.  (a) and
(b) are also compared: the first passages thresholded from the series must be those of first_passage.

    python tests/tools/first_passage_cost.py [--members 4096] [--every 20] [--steps 2000] [--rounds 3]
        > profiles/r13_first_passage_cost.txt"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

PROG = ("Ei", "Ew", "h", "D", "phi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.steps % args.every:
        ap.error("--every must divide --steps")
    pkg = graft.load_package()
    print(f"# library: {os.environ.get('EBM_LIB') or pkg.LIB_PATH}")
    nlat, nt, spin, n, every, nsteps = 180, 2000, 1000, args.members, args.every, args.steps
    nrounds = nsteps // every
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    par = pkg.default_parameters("MIZ")
    run = pkg.EnsembleRun("MIZ", st, par, {k: np.zeros(st.nx) for k in PROG}, fcol=np.zeros(n),
                          noise=dict(sigma=4.0, tau=0.1, seed=1), noise_streams=np.arange(n))
    run.run(spin)                                     # away from the all-zero start: ice and open water, a noise state
    start = run.engine.get_state(PROG + ("T0",))
    nstate = run.engine.noise_state()

    def restore():
        run.engine.set_state(start)
        run.engine.set_noise_state(nstate)
        run.step_index = spin
        run.engine.sync()

    def series():
        return run.series(nsteps, every, names=("T",))[0]

    restore()
    T = series()
    level = float(np.quantile(T, 0.25))

    def until():
        return run.first_passage(nsteps, every, "T", level=level, direction="down")

    def never():
        return run.first_passage(nsteps, every, "T", level=-np.inf, direction="down")

    def rounds():
        for _ in range(nrounds):
            run.run(every, diag_last=True)
        run.engine.sync()

    modes = {"series": series, "until": until, "never": never, "rounds": rounds}
    got = {}
    for m, fn in modes.items():                       # warm-up
        restore()
        got[m] = fn()
    below = got["series"] <= level
    want = np.where(below.any(axis=0), below.argmax(axis=0) + 1, nrounds)
    same = np.array_equal(want, got["until"]["samples"]) and np.array_equal(below.any(axis=0), got["until"]["crossed"])
    assert (got["never"]["samples"] == nrounds).all() and not got["never"]["crossed"].any()
    res = {m: [] for m in modes}
    order = list(modes)
    for r in range(args.rounds):
        for m in order[r % 4:] + order[:r % 4]:
            restore()
            t0 = time.perf_counter()
            modes[m]()
            res[m].append((time.perf_counter() - t0) * 1e3)
    med = {m: statistics.median(v) for m, v in res.items()}
    taken = int(got["until"]["samples"].sum()) * every
    print(f"180 x {n} members, noise sigma 4 tau 0.1, {nsteps} steps, <T> tested every {every} steps ({nrounds} rounds), 64 steps "
          f"per launch, level {level:.6f} (lower quartile of the sampled <T>), going down; first passages of first_passage == "
          f"those thresholded from the series: {same}")
    print(f"  fell: {int(got['until']['crossed'].sum())} of {n} members; rounds taken by the slowest member: "
          f"{int(got['until']['samples'].max())}")
    print(f"  column-steps: series {n * nsteps}, first_passage {taken} ({100.0 * (1.0 - taken / (n * nsteps)):.1f} % not taken)")
    for m in modes:
        print(f"  {m:6s} median {med[m]:9.3f} ms   min {min(res[m]):9.3f}   max {max(res[m]):9.3f}   "
              f"{['%.3f' % v for v in res[m]]}")
    print(f"  until/series {med['until'] / med['series']:.4f}   never/series {med['never'] / med['series']:.4f}")
    print(f"  check + compaction + synchronisation: (never - rounds) / {nrounds} rounds = "
          f"{(med['never'] - med['rounds']) / nrounds * 1e3:.1f} us per round", flush=True)
    run.close()


if __name__ == "__main__":
    main()
