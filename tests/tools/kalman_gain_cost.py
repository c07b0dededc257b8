"""What ebm_kalman_gain_device costs on an MI355X (not a test, not a gate): python tests/tools/kalman_gain_cost.py [out.jsonl [nlat ...]]

Per case — nlat = 180, 1024, 2048, 4096; all cells observed and one in four; one field and five — one JSON line with
  gain_ms        the whole synchronous ebm_kalman_gain_device call (index lists and obs_var up, assembly, factor, two solves,
                 scatter, flag down), wall clock, median and range of ROUNDS calls after a dropped warm-up call;
  assembly_ms, factor_ms, solve_ms, scatter_ms   the same calls split by HIP events on the handle's stream
                 (ebm_kalman_gain_phases), the median of each over the same ROUNDS calls;
  tflops_factor, tflops_solve   the useful fp64 operations over those times: m^3 / 3 for the factor, 2 * nrhs * m^2 for the
                 two solves together (nrhs = nfields * nlat); tflops: their sum over factor_ms + solve_ms;
  host_path_ms   the path the call replaces, in the same process: covariances down, NumPy taper and assembly,
                 numpy.linalg.solve per field, gain up; wall clock, the median of ROUNDS passes after a dropped warm-up pass
                 (one pass after a warm-up pass at 2048 and 4096 latitudes, where a pass takes seconds);
  agrees_with_numpy   the device gain against that host gain at rtol 1e-7 of each row's largest entry."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

ROUNDS = 3


def timed(call):
    t = []
    for _ in range(ROUNDS + 1):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    t = sorted(t[1:])
    return t[len(t) // 2], t[0], t[-1]


def main():
    import torch
    pkg = graft.load_package()
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    sizes = [int(a) for a in sys.argv[2:]] or [180, 1024, 2048, 4096]

    def emit(line):
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    for nlat in sizes:
        st = pkg.SpaceTime("sin", nlat, 2000, 1)
        eng = pkg.Engine("MIZ_IMEX", st.grid_kind, st.x, vec, st.dt, 4, device=0)
        x = np.asarray(st.x, dtype=np.float64)
        rng = np.random.default_rng(nlat)
        A = rng.normal(size=(nlat, 256))
        P_oo = torch.from_numpy(A @ A.T / 256).cuda()
        for every in (1, 4):
            obs = np.full(nlat, np.nan)
            obs[::every] = 0.0
            J = np.flatnonzero(~np.isnan(obs))
            m = J.size
            for nf in (1, 5):
                P_fo = [torch.from_numpy(rng.normal(size=(nlat, nlat))).cuda() for _ in range(nf)]
                box, phases = {}, []

                def call():
                    box.update(g=eng.kalman_gain_tensor(obs, 0.5, 0.3, 1.05, P_oo, P_fo))
                    phases.append(eng.kalman_gain_phases())
                gain = timed(call)
                ph = {k: float(np.median([q[k] for q in phases[1:]])) for k in phases[0]}
                nrhs = nf * nlat

                def host():
                    Po = P_oo.cpu().numpy()
                    rho = pkg.gaspari_cohn(np.abs(x[:, None] - x[None, :]) / 0.3)
                    S = rho[np.ix_(J, J)] * Po[np.ix_(J, J)] * 1.05 + 0.5 * np.eye(m)
                    G = np.zeros((nf, nlat, nlat))
                    for v in range(nf):
                        G[v][:, J] = np.linalg.solve(S, (1.05 * rho[:, J] * P_fo[v].cpu().numpy()[:, J]).T).T
                    up = torch.from_numpy(G).cuda()
                    torch.cuda.synchronize()
                    del up
                    box["G"] = G
                passes = []
                for _ in range(2 if nlat >= 2048 else ROUNDS + 1):
                    t0 = time.perf_counter()
                    host()
                    passes.append((time.perf_counter() - t0) * 1e3)
                passes = sorted(passes[1:])
                host_ms = passes[len(passes) // 2]
                got, G = box["g"].cpu().numpy(), box["G"]
                agrees = bool((np.abs(got - G) <= 1e-7 * np.max(np.abs(G), axis=2, keepdims=True)).all())
                f_factor, f_solve = m ** 3 / 3.0, 2.0 * nrhs * m * m
                emit(dict(nlat=nlat, observed=m, nfields=nf, gain_ms=round(gain[0], 3), gain_ms_min=round(gain[1], 3), gain_ms_max=round(gain[2], 3),
                          assembly_ms=round(ph["assembly"], 3), factor_ms=round(ph["factor"], 3), solve_ms=round(ph["solve"], 3),
                          scatter_ms=round(ph["scatter"], 3), tflops_factor=round(f_factor / (ph["factor"] * 1e-3) / 1e12, 3),
                          tflops_solve=round(f_solve / (ph["solve"] * 1e-3) / 1e12, 3),
                          tflops=round((f_factor + f_solve) / ((ph["factor"] + ph["solve"]) * 1e-3) / 1e12, 3),
                          host_path_ms=round(host_ms, 1), host_over_device=round(host_ms / gain[0], 1), agrees_with_numpy=agrees))
                del P_fo, box
        eng.close()


if __name__ == "__main__":
    main()
