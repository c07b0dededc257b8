"""What ebm_column_misfits costs on an MI355X (not a test, not a gate): python tests/tools/column_misfits_cost.py [out.jsonl]

Per case — 180 latitudes x 4096 members, 1024 x 16384 and 4096 x 2048; 1 and 3 fields; 1 and 8 targets; rows pair-split, as
one-launch steps leave them — one JSON line with
  call_ms      ebm_column_misfits_device, the whole synchronous call (targets and rw uploaded, one launch, stream
               synchronise), HIP events on the handle's stream around CALLS calls, median and range of ROUNDS rounds after a
               dropped warm-up round;
  host_ms      (a) today's way: ebm_get_field of the same fields plus the vectorised NumPy equivalent
               (tests/column_misfits_ref.py: column_misfits_fast), wall clock, median of 3;
  sums_ms      (b) ebm_ensemble_sums_device over the same fields, timed the same way: it reads the same bytes and is the
               library's measured read-rate yardstick;
  bytes        what the call must move from HBM: ncol * nlat * 8 per field (targets and rw are shared by all columns);
               share_of_peak = bytes / call_ms against 8 TB/s.
The alternation of the ways inside one process keeps them under the same clocks."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
from column_misfits_ref import column_misfits_fast  # noqa: E402

CALLS, ROUNDS = 10, 3
PEAK = 8.0e12


def timed(eng, call):
    rounds = []
    for _ in range(ROUNDS + 1):
        eng.timer_start()
        for _ in range(CALLS):
            call()
        rounds.append(eng.timer_stop() / CALLS)
    return sorted(rounds[1:])


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
        rng = np.random.default_rng(0)
        for names in (("T",), ("Ei", "phi", "T")):
            for ntargets in (1, 8):
                eng.run(0, 2, None, True, 1)             # one-launch steps: the rows lie pair-split
                y = rng.normal(0.0, 1.0, (ntargets, len(names), nlat))
                y[:, :, ::10] = np.nan
                rw = rng.uniform(0.5, 1.5, (len(names), nlat))
                buf = torch.empty((ntargets, 2, ncol), dtype=torch.float64, device="cuda")
                sbuf = torch.empty((len(names), 3, nlat), dtype=torch.float64, device="cuda")
                conv = eng.state_conversions()
                call = timed(eng, lambda: eng.column_misfits_device(names, y, buf.data_ptr(), rw))
                sums = timed(eng, lambda: eng.ensemble_sums_device(names, sbuf.data_ptr()))
                assert eng.state_conversions() == conv
                got = buf.cpu().numpy()
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref = column_misfits_fast(np.stack([eng.get_field(n) for n in names]), y, rw)
                    host.append((time.perf_counter() - t0) * 1e3)
                ok = bool(np.array_equal(got[:, 1], ref[:, 1]) and np.allclose(got[:, 0], ref[:, 0], rtol=1e-9, equal_nan=True))
                nbytes = ncol * nlat * 8 * len(names)
                mid, smid, hmid = call[len(call) // 2], sums[len(sums) // 2], sorted(host)[1]
                line = dict(nlat=nlat, ncol=ncol, nvars=len(names), ntargets=ntargets, call_ms=round(mid, 5),
                            call_ms_min=round(call[0], 5), call_ms_max=round(call[-1], 5), host_ms=round(hmid, 3),
                            host_over_call=round(hmid / mid, 1), sums_ms=round(smid, 5), call_over_sums=round(mid / smid, 3),
                            bytes=nbytes, call_tb_per_s=round(nbytes / (mid * 1e-3) / 1e12, 3),
                            share_of_peak=round(nbytes / (mid * 1e-3) / PEAK, 4), agrees_with_numpy=ok)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        eng.close()


if __name__ == "__main__":
    main()
