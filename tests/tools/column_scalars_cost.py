"""What the column scalars cost on an MI355X (not a test, not a gate): python tests/tools/column_scalars_cost.py [out.jsonl]

Per case — 180 latitudes x 4096 members, 1024 x 16384 and 4096 x 2048; one scalar and twelve; integral kind (the mean of T
over the whole meridian) and edge kind (the ice edge: phi >= 0.15 from the equator, on the mid-year state, whose edge lies at
about x = 0.9) — one JSON line with
  call_ms      ebm_column_scalars, the whole synchronous call (one launch, the result down, stream synchronise), HIP events
               on the handle's stream around CALLS calls, median and range of ROUNDS rounds after a dropped warm-up round;
  host_ms      today's way: ebm_get_field of the field plus the vectorised NumPy equivalent below, wall clock, median of 3;
  mean_ms      ebm_hemispheric_mean of the same field, timed as call_ms: what the integral kinds must cost per scalar.
Then one line for first passage on the example's ensemble (examples/noise_induced_transitions.py: 180 latitudes, 3 x 64
members under noise, here from the mid-year state): EnsembleRun.first_passage_scalar on the ice edge against scalar_series
over the same horizon plus host thresholding, wall clock."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from support import midyear_state  # noqa: E402

CALLS, ROUNDS = 10, 3


def timed(eng, call):
    rounds = []
    for _ in range(ROUNDS + 1):
        eng.timer_start()
        for _ in range(CALLS):
            call()
        rounds.append(eng.timer_stop() / CALLS)
    return sorted(rounds[1:])


def host_scalar(f, x, kind, level):
    """The vectorised host equivalent over the whole meridian (same values up to the order of the sum)."""
    if kind == "mean":
        return ((f[:, :-1] + f[:, 1:]) * (x[1:] - x[:-1]) / 2.0).sum(axis=1) / (x[-1] - x[0])
    hit = f >= level
    K = hit.argmax(axis=1)
    c = np.arange(len(f))
    a, b = f[c, np.maximum(K - 1, 0)], f[c, K]
    with np.errstate(all="ignore"):
        v = x[np.maximum(K - 1, 0)] + (level - a) / (b - a) * (x[K] - x[np.maximum(K - 1, 0)])
    return np.where(~hit.any(axis=1), np.inf, np.where(K == 0, x[0], v))


def main():
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    for nlat, ncol in ((180, 4096), (1024, 16384), (4096, 2048)):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
        eng.set_state(midyear_state("MIZ", st, ncol))
        eng.set_field("T", np.random.default_rng(0).normal(0.0, 10.0, (ncol, nlat)))
        for kind, name, level in (("mean", "T", None), ("edge_ge", "phi", 0.15)):
            one = pkg.scalar_spec(st, kind, name, None, level)
            mean = timed(eng, lambda: eng.hemispheric_mean(name))
            for nscal in (1, 12):
                call = timed(eng, lambda: eng.column_scalars([one] * nscal))
                got = eng.column_scalars([one] * nscal)[0]
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref = host_scalar(eng.get_field(name), st.x, kind, level)
                    host.append((time.perf_counter() - t0) * 1e3)
                mid, mmid, hmid = call[len(call) // 2], mean[len(mean) // 2], sorted(host)[1]
                say(dict(nlat=nlat, ncol=ncol, kind=kind, field=name, nscal=nscal, call_ms=round(mid, 5), call_ms_min=round(call[0], 5),
                         call_ms_max=round(call[-1], 5), host_ms=round(hmid, 3), host_over_call=round(hmid / mid, 1),
                         mean_ms=round(mmid, 5), call_over_mean=round(mid / mmid, 3),
                         agrees_with_numpy=bool(np.allclose(got, ref, rtol=1e-9, equal_nan=True))))
        eng.close()
    # first passage on the example's ensemble
    nlat, n, every, years = 180, 64, 100, 2
    st = pkg.SpaceTime("sin", nlat, 2000, 1)
    F = np.repeat(np.array([-2.0, 0.0, 2.0]), n)
    edge = pkg.scalar_spec(st, "edge_ge", "phi", None, 0.15)

    def ensemble():
        init = {k: v for k, v in midyear_state("MIZ", st, 3 * n).items() if k != "T0"}
        return pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), init, fcol=F, noise=dict(sigma=4.0, tau=0.1, seed=1),
                               noise_streams=np.arange(3 * n))
    run = ensemble()
    start = run.ice_edge()
    level = start - 0.02                                     # the edge has come down by 0.02 in x
    run.engine.sync()
    t0 = time.perf_counter()
    series = run.scalar_series(2000 * years, every, [edge])[0]
    below = series <= level[None, :]
    first_series = np.where(below.any(axis=0), below.argmax(axis=0) + 1, -1)
    series_ms = (time.perf_counter() - t0) * 1e3
    run.close()
    run = ensemble()
    run.engine.sync()
    t0 = time.perf_counter()
    fp = run.first_passage_scalar(2000 * years, every, edge, level, "down")
    until_ms = (time.perf_counter() - t0) * 1e3
    run.close()
    first_until = np.where(fp["crossed"], fp["samples"], -1)
    say(dict(case="first_passage_on_the_ice_edge", nlat=nlat, ncol=3 * n, every=every, steps=2000 * years, series_ms=round(series_ms, 2),
             until_ms=round(until_ms, 2), series_over_until=round(series_ms / until_ms, 2), crossed=int(fp["crossed"].sum()),
             column_steps_taken=int(fp["samples"].sum()) * every, column_steps_horizon=3 * n * 2000 * years,
             same_first_passage=bool(np.array_equal(first_series, first_until))))


if __name__ == "__main__":
    main()
