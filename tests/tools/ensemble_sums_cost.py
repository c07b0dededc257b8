"""What ebm_ensemble_sums costs on an MI355X (not a test, not a gate): python tests/tools/ensemble_sums_cost.py [out.jsonl]

Per case — 1 and 3 variables; 4096 members x 2048 latitudes and 16384 x 1024; rows pair-split (after one-launch steps) and
natural (after a fused launch) — one JSON line with
  call_ms      ebm_ensemble_sums_device, the whole synchronous call (weights upload, two launches, stream synchronise), HIP
               events on the handle's stream around CALLS calls, median and range of ROUNDS rounds after a dropped warm-up round;
  host_ms      today's way: ebm_get_field of the same fields plus the NumPy reduction (sum of w, w x, w x x over the members),
               wall clock, median of 3 (ebm_get_field is the parent commit's code: this change does not touch it);
  bytes        what the call must move: ncol * nlat * 8 per variable; share_of_peak = bytes / call_ms against 8 TB/s.
The kernels alone are timed by running this script under `rocprofv3 --kernel-trace --stats` in a run of its own
(ensemble_partials_kernel, ensemble_finish_kernel in the trace); the alternation of the two ways inside one process keeps
both under the same clocks."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

CALLS, ROUNDS = 20, 7
PEAK = 8.0e12


def main():
    import torch
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for ncol, nlat in ((4096, 2048), (16384, 1024)):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
        eng.set_time_table(st.t)
        eng.set_column_forcing(np.linspace(-1.0, 1.0, ncol))
        w = np.random.default_rng(0).uniform(0.5, 1.5, ncol)
        for layout in ("pair_split", "natural"):
            eng.run(0, 2, None, True, 1 if layout == "pair_split" else 2)
            for names in (("T",), ("Ei", "phi", "T")):
                buf = torch.empty((len(names), 3, nlat), dtype=torch.float64, device="cuda")
                conv = eng.state_conversions()
                rounds = []
                for r in range(ROUNDS + 1):
                    eng.timer_start()
                    for _ in range(CALLS):
                        eng.ensemble_sums_device(names, buf.data_ptr(), w)
                    rounds.append(eng.timer_stop() / CALLS)
                assert eng.state_conversions() == conv
                rounds = sorted(rounds[1:])
                got = buf.cpu().numpy()
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref = np.empty((len(names), 3, nlat))
                    for i, n in enumerate(names):
                        x = eng.get_field(n)
                        wx = w[:, None] * x
                        ref[i] = (np.full(nlat, w.sum()), wx.sum(axis=0), (wx * x).sum(axis=0))
                    host.append((time.perf_counter() - t0) * 1e3)
                # (get_field has converted the state: step again so that the next case sees the layout it names)
                eng.run(0, 2, None, True, 1 if layout == "pair_split" else 2)
                ok = bool(np.allclose(got[:, 1:], ref[:, 1:], rtol=1e-9, atol=1e-9 * np.abs(ref[:, 1:]).max(), equal_nan=True))
                nbytes = ncol * nlat * 8 * len(names)
                call = rounds[len(rounds) // 2]
                line = dict(ncol=ncol, nlat=nlat, layout=layout, nvars=len(names), call_ms=round(call, 5),
                            call_ms_min=round(rounds[0], 5), call_ms_max=round(rounds[-1], 5), host_ms=round(sorted(host)[1], 3),
                            host_over_call=round(sorted(host)[1] / call, 1), bytes=nbytes,
                            call_tb_per_s=round(nbytes / (call * 1e-3) / 1e12, 3), share_of_peak=round(nbytes / (call * 1e-3) / PEAK, 4),
                            agrees_with_numpy=ok)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
        eng.close()


if __name__ == "__main__":
    main()
