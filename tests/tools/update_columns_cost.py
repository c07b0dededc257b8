"""What ebm_update_columns costs on an MI355X (not a test, not a gate): python tests/tools/update_columns_cost.py [out.jsonl]

Per case — nlat x ncol = 180 x 4096, 1024 x 16384 and 4096 x 2048; one field (Ei) and five (Ei, Ew, h, D, phi); obs_field Ew, a
prognostic field, so that no step is needed between calls; the MIZ_IMEX model, whose implicit diffusion is stable at 2000
steps per year at every one of these sizes (the explicit model is not beyond 180 latitudes, and its state would hold NaN);
rows pair-split, after one-launch steps (split_rows records that the state did lie so) — one JSON line with
  host_gain_ms    ebm_update_columns, the whole synchronous call (the gain of every field up through the one pitch^2 buffer,
                  target up, the innovations, one product launch per field, stream synchronise), wall clock around CALLS
                  calls, median and range of ROUNDS rounds after a dropped warm-up round;
  device_gain_ms  ebm_update_columns_device with the gain resident on the device: one product launch over all fields;
  tflops          2 * nlat^2 * ncol * nfields / device_gain_ms: the useful fp64 operations of the definition over the time of
                  the call (tflops_host_gain: over host_gain_ms).  Beside it stand the covariance's 21 - 44 at the two large
                  shapes (profiles/r31_covariance_cost.jsonl): the same instruction fed from LDS the same way;
  host_path_ms    the way it replaces, in the same process: ebm_get_field of the fields and of obs_field, NumPy
                  x + d @ G.T per field, ebm_set_field of the fields; wall clock, median of 3;
  agrees_with_numpy   the device result against that host path at rtol 1e-9, NaN cells equal to NaN cells; nan_cells counts
                  them over the compared fields (0 expected: the state is a stable model's).
A last line times the host part of EnsembleRun.enkf at nlat = 2048, all cells observed: the m x m solve for five fields.
The kernels alone are timed by running this script under `rocprofv3 --kernel-trace --stats` in a run of its own
(update_innovations_kernel, update_product_kernel in the trace)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

CALLS, ROUNDS = 3, 5
PROG = ("Ei", "Ew", "h", "D", "phi")


def median_of_rounds(call):
    rounds = []
    for _ in range(ROUNDS + 1):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        rounds.append((time.perf_counter() - t0) * 1e3 / CALLS)
    rounds = sorted(rounds[1:])
    return rounds[len(rounds) // 2], rounds[0], rounds[-1]


def host_path(eng, names, G, y):
    d = np.nan_to_num(y[None, :] - eng.get_field("Ew"), nan=0.0)
    new = {n: eng.get_field(n) + d @ G[v].T for v, n in enumerate(names)}
    for n, x in new.items():
        eng.set_field(n, x)
    return new


def main():
    import torch
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
    for nlat, ncol in ((180, 4096), (1024, 16384), (4096, 2048)):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
        eng = pkg.Engine("MIZ_IMEX", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
        eng.set_time_table(st.t)
        eng.set_column_forcing(np.linspace(-1.0, 1.0, ncol))
        rng = np.random.default_rng(0)
        y = rng.normal(0.0, 1.0, nlat)
        for names in (("Ei",), PROG):
            G = rng.normal(0.0, 1e-7, (len(names), nlat, nlat))       # small: the state stays in range over the rounds
            Gd = torch.from_numpy(G).cuda()
            eng.run(0, 2, None, True, 1)                              # rows pair-split
            conv = eng.state_conversions()
            host = median_of_rounds(lambda: eng.update_columns(names, "Ew", G, y, 1.0))
            dev = median_of_rounds(lambda: eng.update_columns(names, "Ew", Gd, y, 1.0))
            assert eng.state_conversions() == conv
            eng.get_field("Ei")
            split_rows = eng.state_conversions() == conv + 1          # the rows did lie pair-split during the timed calls
            before = {n: eng.get_field(n) for n in names + ("Ew",)}
            eng.update_columns(names, "Ew", Gd, y, 1.0)
            got = {n: eng.get_field(n) for n in names}
            for n, x in before.items():
                eng.set_field(n, x)
            paths = []
            for r in range(3):
                t0 = time.perf_counter()
                ref = host_path(eng, names, G, y)
                paths.append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    agrees = all(np.allclose(got[n], ref[n], rtol=1e-9, atol=1e-12, equal_nan=True) for n in names)
                    nans = int(sum(np.isnan(got[n]).sum() + np.isnan(ref[n]).sum() for n in names))
            flops = 2.0 * nlat * nlat * ncol * len(names)
            emit(dict(nlat=nlat, ncol=ncol, nfields=len(names), host_gain_ms=round(host[0], 4), host_gain_ms_min=round(host[1], 4),
                      host_gain_ms_max=round(host[2], 4), device_gain_ms=round(dev[0], 4), device_gain_ms_min=round(dev[1], 4),
                      device_gain_ms_max=round(dev[2], 4), tflops=round(flops / (dev[0] * 1e-3) / 1e12, 3),
                      tflops_host_gain=round(flops / (host[0] * 1e-3) / 1e12, 3), host_path_ms=round(sorted(paths)[1], 2),
                      host_path_over_host_gain=round(sorted(paths)[1] / host[0], 2), agrees_with_numpy=bool(agrees), nan_cells=nans, split_rows=bool(split_rows)))
        eng.close()
    # the host part of enkf: S = P_oo + R, G_f = P_fo S^-1 for five fields at nlat = 2048
    m = 2048
    A = np.random.default_rng(1).normal(0.0, 1.0, (m, 256))
    S = A @ A.T / 256 + 0.5 * np.eye(m)
    B = np.random.default_rng(2).normal(0.0, 1.0, (5, m, m))
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        for v in range(5):
            np.linalg.solve(S, B[v].T)
        times.append((time.perf_counter() - t0) * 1e3)
    emit(dict(enkf_host_solve_nlat=m, nfields=5, solve_ms=round(sorted(times)[1], 1)))


if __name__ == "__main__":
    main()
