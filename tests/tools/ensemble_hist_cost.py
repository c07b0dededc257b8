"""What ebm_ensemble_range, ebm_ensemble_histogram and EnsembleRun.quantiles cost on an MI355X (not a test, not a gate):
python tests/tools/ensemble_hist_cost.py [out.jsonl]        (EBM_LIB=... selects another build: the A/B of the tile width)

Per case — 4096 members x 2048 latitudes and 16384 x 1024; 1 field (T) and 3 (Ew, phi, T), random bimodal data loaded with
ebm_set_field (natural layout: the kernels' accesses do not depend on the layout); nbins 32 and 64 — one JSON line with
  range_ms, hist_ms, sums_ms   the whole synchronous _device call (weights upload, edges upload, two launches, stream
               synchronise), HIP events on the handle's stream around CALLS calls: median, min and max of ROUNDS rounds after
               a dropped warm-up round.  sums_ms is ebm_ensemble_sums_device over the same fields: the sibling that reads
               the same bytes;
  quantiles_ms a full quantiles(names, (0.05, 0.5, 0.95)) with that nbins and the passes that reach 2^-20 of the range
               (nbins 32: 4, nbins 64: 4 gives 2^-24, 3 gives 2^-18 — both are reported), wall clock, median of QROUNDS;
  host_*_ms    today's way: ebm_get_field of the same fields plus NumPy for the same result (min / max; the slots by the
               definition's arithmetic and np.bincount; np.quantile(method="inverted_cdf")), wall clock, median of 3;
  bytes        what a call must read: ncol * nlat * 8 per field; hist_tb_per_s = bytes / hist_ms."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

CALLS, ROUNDS, QROUNDS = 20, 7, 5
QS = (0.05, 0.5, 0.95)


def stats(rounds, prefix):
    rounds = sorted(rounds)
    return {prefix: round(rounds[len(rounds) // 2], 5), prefix + "_min": round(rounds[0], 5), prefix + "_max": round(rounds[-1], 5)}


def timed(eng, call):
    rounds = []
    for _ in range(ROUNDS + 1):
        eng.timer_start()
        for _ in range(CALLS):
            call()
        rounds.append(eng.timer_stop() / CALLS)
    return rounds[1:]


def wall(call, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        res = call()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2], res


def host_histogram(x, lo, hi, nbins):
    ncol, nlat = x.shape
    s = nbins / (hi - lo)
    t = (x - lo) * s
    slot = np.where(x < lo, 0, np.where(x >= hi, nbins + 1, 1 + np.minimum(np.clip(t, 0, nbins).astype(np.int64), nbins - 1)))
    flat = slot * nlat + np.arange(nlat)
    return np.bincount(flat.ravel(), minlength=(nbins + 2) * nlat).reshape(nbins + 2, nlat).astype(np.float64)


def main():
    import torch
    pkg = graft.load_package()
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]

    class Quantiles(ensemble.EnsembleMoments):
        def __init__(self, eng):
            self.ensemble_range, self.ensemble_histogram = eng.ensemble_range, eng.ensemble_histogram

    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    print(f"# library: {os.environ.get('EBM_LIB') or pkg.LIB_PATH}", flush=True)
    for ncol, nlat in ((4096, 2048), (16384, 1024)):
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0)
        rng = np.random.default_rng(0)
        data = {"Ew": rng.normal(0.0, 5.0, (ncol, nlat)), "phi": rng.uniform(0.0, 1.0, (ncol, nlat)),
                "T": rng.normal(0.0, 2.0, (ncol, nlat)) + 10.0 * (rng.random((ncol, 1)) < 0.4)}     # two branches
        for n in ("Ew", "phi", "T"):
            eng.set_field(n, data[n])
        run = Quantiles(eng)
        for names in (("T",), ("Ew", "phi", "T")):
            nv = len(names)
            x = np.stack([data[n] for n in names])
            lo, hi = x.min(axis=1) - 1e-6, x.max(axis=1) + 1e-6
            rbuf = torch.empty((nv, 3, nlat), dtype=torch.float64, device="cuda")
            sbuf = torch.empty((nv, 3, nlat), dtype=torch.float64, device="cuda")
            conv = eng.state_conversions()
            line = dict(ncol=ncol, nlat=nlat, nvars=nv, bytes=ncol * nlat * 8 * nv)
            line.update(stats(timed(eng, lambda: eng.ensemble_range_device(names, rbuf.data_ptr())), "range_ms"))
            line.update(stats(timed(eng, lambda: eng.ensemble_sums_device(names, sbuf.data_ptr())), "sums_ms"))
            host_range, want_r = wall(lambda: [(f.min(axis=0), f.max(axis=0)) for f in (eng.get_field(n) for n in names)], 3)
            host_q, want_q = wall(lambda: [np.quantile(eng.get_field(n), QS, axis=0, method="inverted_cdf") for n in names], 3)
            got_r = rbuf.cpu().numpy()
            ok = all(np.array_equal(got_r[i, 1], want_r[i][0]) and np.array_equal(got_r[i, 2], want_r[i][1]) for i in range(nv))
            line.update(host_range_ms=round(host_range, 3), host_quantiles_ms=round(host_q, 3), range_agrees_with_numpy=bool(ok))
            for nbins in (32, 64):
                hbuf = torch.empty((nv, nbins + 2, nlat), dtype=torch.float64, device="cuda")
                rec = dict(line, nbins=nbins)
                rec.update(stats(timed(eng, lambda: eng.ensemble_histogram_device(names, lo, hi, nbins, hbuf.data_ptr())), "hist_ms"))
                host_h, want_h = wall(lambda: [host_histogram(eng.get_field(n), lo[i], hi[i], nbins) for i, n in enumerate(names)], 3)
                rec.update(host_hist_ms=round(host_h, 3), hist_agrees_with_numpy=bool(np.array_equal(hbuf.cpu().numpy(), np.stack(want_h))))
                for passes in ((4,) if nbins == 32 else (3, 4)):
                    q_ms, got_q = wall(lambda: run.quantiles(names, QS, nbins=nbins, passes=passes), QROUNDS)
                    inside = all((np.abs(got_q[n]["value"] - want_q[i]) <= got_q[n]["halfwidth"]).all() for i, n in enumerate(names))
                    rec[f"quantiles_ms_passes{passes}"] = round(q_ms, 3)
                    rec[f"quantiles_max_halfwidth_passes{passes}"] = float(max(got_q[n]["halfwidth"].max() for n in names))
                    rec[f"quantiles_within_halfwidth_of_numpy_passes{passes}"] = bool(inside)
                rec.update(hist_tb_per_s=round(rec["bytes"] / (rec["hist_ms"] * 1e-3) / 1e12, 3),
                           sums_tb_per_s=round(rec["bytes"] / (rec["sums_ms"] * 1e-3) / 1e12, 3),
                           hist_over_sums=round(rec["hist_ms"] / rec["sums_ms"], 2),
                           host_over_hist=round(host_h / rec["hist_ms"], 1), host_over_range=round(host_range / rec["range_ms"], 1))
                print(json.dumps(rec), flush=True)
                if out:
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
            assert eng.state_conversions() == conv
        eng.close()


if __name__ == "__main__":
    main()
