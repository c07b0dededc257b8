"""GPU tests (-m gpu) of per-column parameter sets (ebm_set_column_params, include/ebm_hip.h).

The contract is exact: column c of a handle with parameter rows installed gives the BITS a one-column handle created
with row c gives (same model, grid, x, dt and options), in every entry point.  The rows perturb every parameter the
model uses by up to +-20 % (Tm and m2 kept legal) and repeat some rows, so that the deduplication into parameter sets
is exercised as well.
"""
import numpy as np
import pytest

from conftest import load_golden, scaled_err, record_error
from support import CLASSIC_VARS as CLASSIC_ALL, MIZ_PROG as PROG, all_fields, is_miz

pytestmark = pytest.mark.gpu

MIZ_ALL = all_fields("MIZ")
MIZ_USED = ("D", "A", "B", "cw", "S0", "S1", "S2", "a0", "a2", "ai", "Fb", "k", "Lf", "Tm", "m1", "m2", "alpha", "rl",
            "Dmin", "Dmax", "hmin", "kappa")
CLASSIC_USED = ("D", "A", "B", "cw", "S0", "S1", "S2", "a0", "a2", "ai", "Fb", "k", "Lf", "F", "cg", "tau")
TOL_SHORT = 1e-10    # test_gpu_parity.py: trajectories of <= 50 steps


def base_params(pkg, model):
    return pkg.default_parameters("MIZ" if is_miz(model) else "Classic")


def param_rows(pkg, model, n, seed, spread=0.2):
    """n rows: every parameter the model uses scaled by a factor in [1 - spread, 1 + spread] (Tm = 0 moved up by at most
    spread, so that Tm^m2 stays defined), rows 1 and n-1 repeating rows 0 and 2."""
    rng = np.random.default_rng(seed)
    used = MIZ_USED if is_miz(model) else CLASSIC_USED
    base = pkg.engine.param_vector(base_params(pkg, model), pkg.default_parval)
    rows = np.tile(base, (n, 1))
    for c in range(n):
        for name in used:
            i = pkg.engine.PARAM_ORDER.index(name)
            rows[c, i] = rng.uniform(0.0, spread) if name == "Tm" else base[i] * rng.uniform(1.0 - spread, 1.0 + spread)
    rows[1] = rows[0]
    rows[n - 1] = rows[2]
    return rows


def nt_for(model, nlat):
    # its own table, not support.steps_per_year: meridians of 1024 cells, and 4096 stepped by the explicit model
    if not is_miz(model):
        return 2000
    return {180: 2000, 1024: 262144, 4096: 1048576}[nlat]


def initial_state(pkg, model, st, ncol):
    """The golden fixtures' mid-year state (ice edge, open water, a live T0 solve) interpolated onto st.x.
    A new test should take support.midyear_state instead: field-by-field interpolation makes cells no model state has."""
    if is_miz(model):
        g = load_golden(f"miz_{'identity' if st.grid_kind == 'identity' else 'sin'}_180_2000.npz")
        return {k: np.tile(np.interp(st.x, g["x"], g[f"s1000_{k}"]), (ncol, 1)) for k in PROG + ("T0",)}
    g = load_golden("classic_identity_180_2000.npz")
    return {k: np.tile(np.interp(st.x, g["x"], g[f"s522_{k}"]), (ncol, 1)) for k in ("E", "Tg")}


def first_step(st):
    return (st.nt * 1000) // 2000


def engine(pkg, model, st, vec, ncol, **opt):
    return pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, ncol, device=0, **opt)


def prepare(pkg, model, st, eng, state, fcol):
    eng.set_state(state)
    eng.set_column_forcing(fcol)
    eng.set_time_table(st.t)
    eng.set_step_clock(first_step(st))


def compare_with_single_handles(pkg, model, st, rows, drive, state=None, **opt):
    """drive(eng, cols) -> {name: (array, axis)}, `axis` the column axis of the array (None: not per column, not
    compared); `cols` the slice of the columns the handle holds.  Runs it on one handle of len(rows) columns with the
    rows installed (the handle created with the default vector) and on one single-column handle created with each row;
    every per-column entry must agree bit for bit.  Returns the multi-column handle's output."""
    ncol = len(rows)
    state = initial_state(pkg, model, st, ncol) if state is None else state
    fcol = np.linspace(-1.5, 1.5, ncol)
    base = pkg.engine.param_vector(base_params(pkg, model), pkg.default_parval)
    with engine(pkg, model, st, base, ncol, **opt) as eng:
        prepare(pkg, model, st, eng, state, fcol)
        eng.set_column_params(rows)
        whole = drive(eng, slice(0, ncol))
    for c in range(ncol):
        with engine(pkg, model, st, rows[c], 1, **opt) as eng:
            prepare(pkg, model, st, eng, {k: v[c:c + 1] for k, v in state.items()}, fcol[c:c + 1])
            alone = drive(eng, slice(c, c + 1))
        for k, (arr, ax) in whole.items():
            if ax is None:
                continue
            want = np.take(alone[k][0], 0, axis=ax)
            assert np.array_equal(np.take(arr, c, axis=ax), want, equal_nan=True), (model, st.nx, c, k)
    return whole


def state_out(eng, model):
    names = MIZ_ALL if is_miz(model) else CLASSIC_ALL
    out = {k: (v, 0) for k, v in eng.get_state(names).items()}
    out["hm_T"] = (eng.hemispheric_mean("T"), 0)
    out["hm_dev"] = (_hm_device(eng), 0)
    return out


def _hm_device(eng):
    import torch
    t = torch.empty(eng.ncol, dtype=torch.float64, device="cuda:0")
    eng.hemispheric_mean_device("T", t.data_ptr())
    torch.cuda.synchronize()
    return t.cpu().numpy()


def single_steps(eng, st):
    for s in range(first_step(st), first_step(st) + 3):
        eng.step(cos2pit(st, s), cos2pit(st, s + 1), 0.3, True)


def runner(nsteps, k=1):
    return lambda eng, st: eng.run(first_step(st), nsteps, np.linspace(0.0, 1.0, nsteps), True, k)


def drivers(model, nlat):
    """name -> (launch options, how the steps are taken)"""
    d = {
        "step": (dict(), single_steps),
        "run_graph0": (dict(use_graph=False), runner(133)),
        "run_graph1": (dict(use_graph=True), runner(133)),         # >= 2 x 64 steps: graph replay
        "fused_lds0": (dict(fused_state_in_lds=False), runner(130, 64)),
        "fused_lds1": (dict(fused_state_in_lds=True), runner(130, 64)),
        "chains2": (dict(launch_chains=2, use_graph=False), runner(40)),   # the second chain starts at column 3
    }
    if nlat <= 1536 and model != "MIZ_IMEX":
        d["cells2"] = (dict(cells_per_thread=2), runner(40))
    return d


def cos2pit(st, s):
    import math
    return math.cos(2.0 * math.pi * float(st.t[s % st.nt]))


CASES = [(m, k, n) for m in ("MIZ", "MIZ_IMEX", "Classic") for k in ("identity", "sin") for n in (180, 1024)] + \
        [("MIZ", "sin", 4096), ("MIZ_IMEX", "sin", 4096), ("MIZ", "identity", 4096)]


@pytest.mark.parametrize("model,kind,nlat", CASES)
def test_columns_give_the_bits_of_one_column_handles(pkg, model, kind, nlat):
    """ebm_step(write_diag), ebm_run with and without graph replay, ebm_run_fused K = 64 with the state in registers
    and in LDS, two launch chains, two cells per thread: every field, T0, the hemispheric means and the solve counter."""
    st = pkg.SpaceTime(kind, nlat, nt_for(model, nlat), 1)
    rows = param_rows(pkg, model, 6, seed=nlat + len(model) + len(kind))
    for name, (opt, run) in drivers(model, nlat).items():
        solves = []

        def drive(eng, cols):
            before = eng.counters()
            run(eng, st)
            out = state_out(eng, model)
            cnt = eng.counters()
            solves.append(cnt["solves"] - before["solves"])
            out["steps"] = (np.array([[cnt["steps"] - before["steps"]]]), None)
            return out
        compare_with_single_handles(pkg, model, st, rows, drive, **opt)
        assert solves[0] == sum(solves[1:]), (name, solves)       # the counters: each column's solves, once
        if is_miz(model):
            assert solves[0] > 0


@pytest.mark.parametrize("model,kind", [(m, k) for m in ("MIZ", "MIZ_IMEX", "Classic") for k in ("identity", "sin")])
def test_integrate_and_hemispheric_integrate_per_column(pkg, model, kind):
    """ebm_integrate (raw of the last year, winter, summer, annual mean; 64 steps per launch on the fused stretches) and
    ebm_integrate_hemispheric over one year of 180 latitudes, from the reference test's zero state (MIZ) with parameters
    within 5 % of the defaults: a year that stays finite."""
    st = pkg.SpaceTime(kind, 180, 2000, 1)
    rows = param_rows(pkg, model, 5, seed=7 + len(model) + len(kind), spread=0.05)
    state = None if model == "Classic" else {k: np.zeros((5, 180)) for k in PROG}
    names = ("E", "T", "phi") if is_miz(model) else ("E", "T", "h")

    def drive(eng, cols):
        eng.set_step_clock(0)
        out = eng.integrate(st.nt, 1, None, True, st.winter.inx, st.summer.inx, names)
        hm = eng.integrate_hemispheric(st.nt, 1, None, st.winter.inx, st.summer.inx, names)
        res = {f"ig_{k}": (v, 2) for k, v in out.items()}
        res.update({f"hm_{k}": (v, 2) for k, v in hm.items()})
        return res
    compare_with_single_handles(pkg, model, st, rows, drive, state=state, integrate_steps_per_launch=64)


@pytest.mark.parametrize("model,kind,nlat", [(m, k, n) for m in ("MIZ", "MIZ_IMEX") for k in ("identity", "sin")
                                             for n in (180, 1024)])
def test_diffusion_operator_per_column(pkg, model, kind, nlat):
    st = pkg.SpaceTime(kind, nlat, nt_for(model, nlat), 1)
    rows = param_rows(pkg, model, 4, seed=11 + nlat)
    rng = np.random.default_rng(nlat)
    temp = rng.normal(0.0, 10.0, (4, nlat))
    base = rng.normal(0.0, 1.0, (4, nlat))

    def drive(eng, cols):
        return {"with_base": (eng.diffusion(temp[cols], base[cols]), 0), "plain": (eng.diffusion(temp[cols]), 0)}
    compare_with_single_handles(pkg, model, st, rows, drive)


@pytest.mark.parametrize("model,kind", [("MIZ", "sin"), ("MIZ", "identity"), ("Classic", "identity")])
def test_columns_follow_the_oracle_with_their_own_rows(pkg, coracle, model, kind):
    """Columns that differ in D, kappa and A, each against the C oracle run with its own row: 20 steps from the golden
    mid-year state, within test_gpu_parity.py's bar for short trajectories."""
    st = pkg.SpaceTime(kind, 180, 2000, 1)
    par = base_params(pkg, model)
    over = [{}, {"D": 0.5}, {"D": 0.7}, {"A": 196.0}] + ([{"kappa": 0.8 * par["kappa"]}, {"D": 0.66, "kappa": 1.2 * par["kappa"]}]
                                                         if is_miz(model) else [{"D": 0.45, "A": 191.0}])
    rows = pkg.engine.param_matrix(over, par, pkg.default_parval)
    ncol, nsteps, s0 = len(over), 20, first_step(st)
    state = initial_state(pkg, model, st, ncol)
    ct = np.array([pkg.cos2pit(float(t)) for t in st.t])
    idx = np.arange(s0, s0 + nsteps)
    with engine(pkg, model, st, pkg.engine.param_vector(par, pkg.default_parval), ncol) as eng:
        eng.set_state(state)
        eng.set_column_params(rows)
        eng.set_time_table(st.t)
        eng.run(s0, nsteps)
        got = eng.get_state(MIZ_ALL if is_miz(model) else CLASSIC_ALL)
    for c in range(ncol):
        pc = dict(par)
        pc.update(over[c])
        one = {k: np.ascontiguousarray(v[c:c + 1]) for k, v in state.items()}
        if is_miz(model):
            diag, _ = coracle.miz_run(0 if kind == "identity" else 1, st.x, pc, st.dt, ct[idx], np.zeros(nsteps), None, one)
        else:
            diag = coracle.classic_run(st.x, pc, st.dt, ct[idx], ct[(idx + 1) % st.nt], np.zeros(nsteps), None, one)
        one.update(diag)
        for k in got:
            err = scaled_err(got[k][c], one[k][0])
            record_error(f"column params {model} {kind} column {c} {over[c]}", k, err, TOL_SHORT)
            assert err <= TOL_SHORT, (c, over[c], k, err)
    assert not np.array_equal(got["T"][1], got["T"][2])           # the rows did take effect


@pytest.mark.parametrize("model", ["MIZ", "Classic"])
def test_rows_changed_mid_run_and_cleared(pkg, model):
    """n1 steps with rows P1, then rows P2 (same Tm), n2 more steps: equal to one-column handles created with P2 that
    restart from the checkpoint (fields + T0) — with graph replay, so the captured graph must not keep P1.  Then NULL:
    the handle steps as a handle created with its original vector."""
    st = pkg.SpaceTime("sin" if is_miz(model) else "identity", 180, 2000, 1)
    n, n1, n2, n3 = 5, 140, 150, 135
    P1 = param_rows(pkg, model, n, seed=1)
    P2 = param_rows(pkg, model, n, seed=2)
    if is_miz(model):
        Tm = pkg.engine.PARAM_ORDER.index("Tm")
        P2[:, Tm] = P1[:, Tm]
    prog = PROG + ("T0",) if is_miz(model) else ("E", "Tg")
    names = MIZ_ALL if is_miz(model) else CLASSIC_ALL
    base = pkg.engine.param_vector(base_params(pkg, model), pkg.default_parval)
    state = initial_state(pkg, model, st, n)
    s0 = first_step(st)
    with engine(pkg, model, st, base, n, use_graph=True) as eng:
        eng.set_state(state)
        eng.set_time_table(st.t)
        eng.set_column_params(P1)
        eng.run(s0, n1, None, True)
        ck1 = eng.get_state(prog)
        eng.set_column_params(P2)
        assert eng.field_step("T")["current"]                    # validity untouched by the setter
        eng.run(s0 + n1, n2, None, True)
        mid = eng.get_state(names)
        eng.set_column_params(None)
        eng.run(s0 + n1 + n2, n3, None, True)
        end = eng.get_state(names)
    for c in range(n):
        with engine(pkg, model, st, P2[c], 1, use_graph=True) as one:
            one.set_state({k: v[c:c + 1] for k, v in ck1.items()})
            one.set_time_table(st.t)
            one.run(s0 + n1, n2, None, True)
            got = one.get_state(names)
        for k in names:
            assert np.array_equal(mid[k][c], got[k][0], equal_nan=True), (c, k)
    with engine(pkg, model, st, base, n, use_graph=True) as ref:
        ref.set_state({k: mid[k] for k in prog})
        ref.set_time_table(st.t)
        ref.run(s0 + n1 + n2, n3, None, True)
        want = ref.get_state(names)
    for k in names:
        assert np.array_equal(end[k], want[k], equal_nan=True), k


def test_bad_rows_are_refused_and_change_nothing(pkg):
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    rows = param_rows(pkg, "MIZ", 4, seed=3)
    bad = rows.copy()
    Tm, m2 = pkg.engine.PARAM_ORDER.index("Tm"), pkg.engine.PARAM_ORDER.index("m2")
    bad[2, Tm], bad[2, m2] = -0.5, 1.36
    base = pkg.engine.param_vector(base_params(pkg, "MIZ"), pkg.default_parval)
    state = initial_state(pkg, "MIZ", st, 4)
    out = []
    for install_bad in (False, True):
        with engine(pkg, "MIZ", st, base, 4) as eng:
            eng.set_state(state)
            eng.set_time_table(st.t)
            eng.set_column_params(rows)
            if install_bad:
                with pytest.raises(pkg.EBMError, match="column 2"):
                    eng.set_column_params(bad)
                with pytest.raises(ValueError):
                    eng.set_column_params(rows[:3])
            eng.run(first_step(st), 20)
            out.append(eng.get_state(("T", "phi")))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True)
    ok = bad.copy()
    ok[2, m2] = 2.0                                                   # integer m2: legal with Tm < 0, as in ebm_create
    with engine(pkg, "MIZ", st, base, 4) as eng:
        eng.set_column_params(ok)


def test_zonal_operator_needs_one_parameter_set(pkg):
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    nlon, ncol = 8, 16
    rows = param_rows(pkg, "MIZ", 3, seed=5)[[0, 2]]
    T = np.random.default_rng(0).normal(0.0, 12.0, (ncol, 180))
    base = pkg.engine.param_vector(base_params(pkg, "MIZ"), pkg.default_parval)
    with engine(pkg, "MIZ", st, base, ncol) as eng:
        U0, Z0 = eng.zonal_diffusion(T, nlon)
        eng.set_column_params(np.repeat(rows, ncol // 2, axis=0))
        with pytest.raises(pkg.EBMError) as err:
            eng.zonal_diffusion(T, nlon)
        assert err.value.status == -3
        eng.set_column_params(np.tile(rows[1], (ncol, 1)))                 # one distinct row: that row's D and cw
        U1, Z1 = eng.zonal_diffusion(T, nlon)
        eng.set_column_params(None)
        U2, Z2 = eng.zonal_diffusion(T, nlon)
    with engine(pkg, "MIZ", st, rows[1], ncol) as ref:
        Ur, Zr = ref.zonal_diffusion(T, nlon)
    assert np.array_equal(U1, Ur) and np.array_equal(Z1, Zr)
    assert np.array_equal(U2, U0) and np.array_equal(Z2, Z0)
    assert not np.array_equal(U1, U0)


def test_ensemble_member_params_equal_separate_runs(pkg):
    """EnsembleRun(member_params=[{"D": d} ...]) with a forcing ramp per member: seasonal_means per member equal those
    of separate EnsembleRuns with par["D"] = d."""
    Ds = (0.45, 0.55, 0.6, 0.7)
    forcings = [pkg.Forcing(0.0, 4.0, 0.0, (1, 1), (4.0 / k, -4.0 / k)) for k in (1, 2, 1, 2)]
    years = max(f.domain[4] for f in forcings) + 1
    st = pkg.SpaceTime("sin", 48, 400, years)
    par = pkg.default_parameters("MIZ")
    init = {k: np.zeros(st.nx) for k in PROG}
    run = pkg.EnsembleRun("MIZ", st, par, init, forcings=forcings, member_params=[{"D": d} for d in Ds])
    assert run.ncol == len(Ds)
    hm = run.seasonal_means(years, ("T", "phi"))
    run.close()
    for m, d in enumerate(Ds):
        pm = pkg.Collection(dict(par))
        pm["D"] = d
        one = pkg.EnsembleRun("MIZ", st, pm, init, forcings=[forcings[m]])
        h1 = one.seasonal_means(years, ("T", "phi"))
        one.close()
        for k in hm:
            assert np.array_equal(hm[k][:, :, m], h1[k][:, :, 0], equal_nan=True), (m, k)
    assert not np.array_equal(hm["avg"][0, :, 0], hm["avg"][0, :, 3])


def test_sets_leave_no_device_memory_behind(pkg):
    """Install, replace and clear 64 distinct rows on a 4096 x 256 handle, twenty times over: the device's free memory
    returns to where it was (the first cycle pays the kernels' and pools' one-off allocations)."""
    import torch
    st = pkg.SpaceTime("sin", 4096, 1048576, 1)
    rows = param_rows(pkg, "MIZ", 64, seed=9)

    def cycle():
        with engine(pkg, "MIZ", st, rows[0], 256) as eng:
            eng.set_time_table(st.t)
            eng.set_column_params(np.repeat(rows, 4, axis=0))
            eng.run(0, 2, None, True, 2)
            eng.set_column_params(np.tile(rows[::-1], (4, 1)))
            eng.run(2, 2, None, True)
            eng.set_column_params(None)
    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free1 >= free0 - (8 << 20), (free0, free1)
