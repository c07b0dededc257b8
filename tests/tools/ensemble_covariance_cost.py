"""What ebm_ensemble_covariance costs on an MI355X (not a test, not a gate): python tests/tools/ensemble_covariance_cost.py [out.jsonl]

Per case — nlat x ncol = 180 x 4096, 1024 x 16384 and 4096 x 2048; symmetric (T with itself about one center: rule 6) and not
(T with phi about two centers); rows pair-split, after one-launch steps — one JSON line with
  call_ms      ebm_ensemble_covariance_device, the whole synchronous call (weights and centers up, two launches, stream
               synchronise), HIP events on the handle's stream around CALLS calls, median and range of ROUNDS rounds after a
               dropped warm-up round;
  tflops       2 * nlat^2 * ncol / call_ms for the full matrix, nlat * (nlat + 1) * ncol for the symmetric one: the useful
               fp64 operations of the definition over the time of the call.  The fp64 MFMA rate of gfx950 is not in the
               project's guides: this is a measurement without a roofline beside it;
  host_ms      today's way in the same process, alternating with the device rounds: ebm_get_field of the fields plus the
               NumPy product (w (x - ca)).T @ (y - cb) with NaN cells zeroed, wall clock, median of 3.  It is a timing
               stand-in, not the definition (no member has weight 0 here); agrees_with_numpy compares the two at rtol 1e-9
               and is informational;
  err_over_bound   at 180 latitudes only (the np.longdouble reference is too slow beyond): the largest |device - reference| /
               derived bound over the matrix, for information.
The kernels alone are timed by running this script under `rocprofv3 --kernel-trace --stats` in a run of its own
(covariance_partials_kernel, covariance_finish_kernel in the trace)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from ensemble_cov_ref import covariance_bound, ensemble_cov_ref  # noqa: E402

CALLS, ROUNDS = 5, 5


def host_product(eng, a, b, w, ca, cb):
    x, y = eng.get_field(a), (eng.get_field(b) if b != a else None)
    da = np.nan_to_num(w[:, None] * (x - ca), nan=0.0)
    db = np.nan_to_num((x if y is None else y) - cb, nan=0.0)
    return da.T @ db


def main():
    import torch
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for nlat, ncol in ((180, 4096), (1024, 16384), (4096, 2048)):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
        eng.set_time_table(st.t)
        eng.set_column_forcing(np.linspace(-1.0, 1.0, ncol))
        w = np.random.default_rng(0).uniform(0.5, 1.5, ncol)
        buf = torch.empty((nlat, nlat), dtype=torch.float64, device="cuda")
        for a, b in (("T", "T"), ("T", "phi")):
            eng.run(0, 2, None, True, 1)
            s = eng.ensemble_sums((a, b) if a != b else (a,), w)
            ca, cb = s[0, 1] / s[0, 0], s[-1, 1] / s[-1, 0]
            conv = eng.state_conversions()
            rounds, host = [], []
            for r in range(ROUNDS + 1):
                eng.timer_start()
                for _ in range(CALLS):
                    eng.ensemble_covariance_device(a, b, w, ca, cb, buf.data_ptr())
                rounds.append(eng.timer_stop() / CALLS)
                if r == 0:
                    assert eng.state_conversions() == conv
                    got = buf.cpu().numpy()
                if r in (1, 2, 3):
                    t0 = time.perf_counter()
                    again = host_product(eng, a, b, w, ca, cb)
                    host.append((time.perf_counter() - t0) * 1e3)
                    if r == 1:
                        ref = again                       # of the state that `got` was taken from: the steps below move it on
                    eng.run(0, 2, None, True, 1)          # get_field has converted the state: pair-split again
            rounds = sorted(rounds[1:])
            call = rounds[len(rounds) // 2]
            sym = a == b
            flops = (nlat * (nlat + 1) if sym else 2 * nlat * nlat) * ncol
            line = dict(nlat=nlat, ncol=ncol, symmetric=sym, call_ms=round(call, 4), call_ms_min=round(rounds[0], 4),
                        call_ms_max=round(rounds[-1], 4), tflops=round(flops / (call * 1e-3) / 1e12, 3), host_ms=round(sorted(host)[1], 2),
                        host_over_call=round(sorted(host)[1] / call, 2),
                        agrees_with_numpy=bool(np.allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())))
            if nlat <= 180:
                eng.ensemble_covariance_device(a, b, w, ca, cb, buf.data_ptr())      # of the state as it is now
                now = buf.cpu().numpy()
                x, y = eng.get_field(a), eng.get_field(b)
                exact, T, n = ensemble_cov_ref(x, y, w, ca, cb, same_field=sym)
                with np.errstate(invalid="ignore", divide="ignore"):
                    line["err_over_bound"] = round(float(np.nanmax(np.where(T > 0.0, np.abs(now - exact) / covariance_bound(T, n, ncol), 0.0))), 4)
            print(json.dumps(line), flush=True)
            if out:
                out.write(json.dumps(line) + "\n")
                out.flush()
        eng.close()


if __name__ == "__main__":
    main()
