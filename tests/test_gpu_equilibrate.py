"""GPU tests (-m gpu) of ebm_equilibrate (include/ebm_hip.h): step each column until its seasonal cycle repeats.

The oracle needs no new code.  A second handle with the same configuration steps plain ebm_run_fused one year at a time and
hands every year-end state to the host, where a restatement of the header's criterion (`expected`) gives each column's
equilibrium year, flag and residual, and the state of each column at its own equilibrium year is kept.  ebm_equilibrate
must reproduce all of it bit for bit.  The tolerances are chosen from the oracle's own distances (`choose_tol`) so that the
data are honest: the equilibrium years are not all equal, at least one column converges before max_years, at least one
does not, at least one column's answer depends on `<=` against `<`, and at least one frozen column's state would have moved
on had it kept stepping.  The members differ in D (ebm_set_column_params) and in their forcing offset, and half of them
start from a spun-up state.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from support import MIZ_DIAG as DIAG, MIZ_PROG as PROG, all_fields, is_miz

pytestmark = pytest.mark.gpu

MIZ_ALL = all_fields("MIZ")


def golden_state(pkg, model, st, ncol):
    """The golden fixtures' mid-year state interpolated onto st.x, every column the same.  Not support.midyear_state: that one
    takes whole nearest cells, which are other numbers than these field-by-field interpolations."""
    if is_miz(model):
        g = load_golden(f"miz_{'identity' if st.grid_kind == 'identity' else 'sin'}_180_2000.npz")
        return {k: np.tile(np.interp(st.x, g["x"], g[f"s1000_{k}"]), (ncol, 1)) for k in PROG + ("T0",)}
    g = load_golden("classic_identity_180_2000.npz")
    return {k: np.tile(np.interp(st.x, g["x"], g[f"s522_{k}"]), (ncol, 1)) for k in ("E", "Tg")}


def member_rows(pkg, model, ncol):
    base = pkg.engine.param_vector(pkg.default_parameters("MIZ" if is_miz(model) else "Classic"), pkg.default_parval)
    rows = np.tile(base, (ncol, 1))
    rows[:, pkg.engine.PARAM_ORDER.index("D")] *= np.linspace(0.8, 1.2, ncol)
    return rows


class Setup:
    """Everything two handles need to start identically: options, member rows, offsets, the start state and clock."""

    def __init__(self, pkg, model, grid, nlat, nt, ncol, fcol=None, start=None, **opt):
        self.pkg, self.model, self.ncol, self.opt = pkg, model, ncol, opt
        self.st = pkg.SpaceTime(grid, nlat, nt, 1)
        self.rows = member_rows(pkg, model, ncol)
        self.fcol = np.linspace(-1.5, 1.5, ncol) if fcol is None else fcol
        self.f_year = None
        self.state = golden_state(pkg, model, self.st, ncol) if start is None else start
        self.clock0 = 0
        # half the members start from a state one year further on
        with self.engine() as eng:
            eng.run(0, nt, None, True, 64)
            spun = eng.get_state(self.prognostic())
        for k in spun:
            self.state.setdefault(k, np.zeros_like(spun[k]))[1::2] = spun[k][1::2]

    def prognostic(self):
        return PROG + ("T0",) if is_miz(self.model) else ("E", "Tg")

    def engine(self, cols=None):
        """A handle of the columns `cols` (default all), prepared."""
        cols = slice(None) if cols is None else cols
        rows = self.rows[cols]
        eng = self.pkg.Engine(self.model, self.st.grid_kind, self.st.x, rows[0], self.st.dt, len(rows), device=0, **self.opt)
        eng.set_column_params(rows)
        eng.set_column_forcing(self.fcol[cols])
        eng.set_time_table(self.st.t)
        eng.set_state({k: v[cols] for k, v in self.state.items()})
        eng.set_step_clock(self.clock0)
        return eng


def reference(setup, max_years):
    """Plain ebm_run_fused one year at a time: snaps[name] [max_years + 1, ncol, nlat] (index y: after y years)."""
    nt = setup.st.nt
    names = all_fields(setup.model)
    with setup.engine() as eng:
        snaps = {k: [None] for k in names}
        for y in range(1, max_years + 1):
            eng.run(setup.clock0 + (y - 1) * nt, nt, setup.f_year, True, 64)
            for k in names:
                snaps[k].append(eng.get_field(k))
    return snaps


def distances(snaps, names):
    """d[v][y, c] = max_k |S(y) - S(y-1)| (NaN-propagating), NaN for y < 2."""
    out = []
    for k in names:
        s = snaps[k]
        d = np.full((len(s), s[1].shape[0]), np.nan)
        for y in range(2, len(s)):
            d[y] = np.max(np.abs(s[y] - s[y - 1]), axis=1)
        out.append(d)
    return np.array(out)


def expected(d, tol, max_years, min_years, strict=False):
    """The header's definition, restated: (years, converged, resid[nvars][ncol])."""
    nv, _, ncol = d.shape
    first = max(2, min_years)
    years = np.full(ncol, max_years, dtype=np.int64)
    conv = np.zeros(ncol, dtype=bool)
    resid = np.full((nv, ncol), np.nan)
    for c in range(ncol):
        for y in range(2, max_years + 1):
            r = d[:, y, c]
            resid[:, c] = r
            ok = np.all(r < tol) if strict else np.all(r <= tol)
            if y >= first and ok:
                years[c], conv[c] = y, True
                break
    return years, conv, resid


def honest(years, conv, max_years):
    return len(set(years.tolist())) > 1 and bool((conv & (years < max_years)).any()) and not conv.all()


def choose_tol(d, max_years, min_years):
    """Tolerances under which the data are honest (see the module text).  The first field's tolerance is one of its own
    distances, so that `<=` against `<` decides some column; the others are a quantile of theirs."""
    nv = d.shape[0]
    first = max(2, min_years)
    for q in (0.5, 0.9, 1.0):
        tol = np.array([np.nanquantile(d[v, first:max_years + 1], q) for v in range(nv)])
        best = None
        for cand in np.unique(d[0, first:max_years + 1]):
            if not np.isfinite(cand):
                continue
            tol[0] = cand
            ys, cv, _ = expected(d, tol, max_years, min_years)
            ys2, cv2, _ = expected(d, tol, max_years, min_years, strict=True)
            if honest(ys, cv, max_years) and (np.any(ys != ys2) or np.any(cv != cv2)):
                score = len(set(ys.tolist()))
                if best is None or score > best[0]:
                    best = (score, tol.copy())
        if best is not None:
            return best[1]
    raise AssertionError("no tolerance makes the data honest: the members' equilibrium years do not spread; distances "
                         f"[field][year][column]:\n{np.array2string(d[:, 2:], precision=3)}")


def check_against_reference(setup, names, max_years, min_years=2, snaps=None, tol=None):
    """ebm_equilibrate on a fresh handle against the oracle; returns (result, snaps, tol); result["counters"] are the
    handle's counters after the call."""
    nt = setup.st.nt
    snaps = reference(setup, max_years) if snaps is None else snaps
    d = distances(snaps, names)
    tol = choose_tol(d, max_years, min_years) if tol is None else np.asarray(tol, dtype=np.float64)
    want_y, want_c, want_r = expected(d, tol, max_years, min_years)
    with setup.engine() as eng:
        eng.reset_counters()
        got = eng.equilibrate(nt, max_years, setup.f_year, dict(zip(names, tol)), min_years)
        assert np.array_equal(got["years"], want_y), (got["years"], want_y)
        assert np.array_equal(got["converged"], want_c), (got["converged"], want_c)
        for i, k in enumerate(names):
            assert np.array_equal(got["resid"][k], want_r[i], equal_nan=True), k
            assert np.array_equal(got["resid"][k].view(np.int64)[np.isfinite(want_r[i])],
                                  want_r[i].view(np.int64)[np.isfinite(want_r[i])]), k
        ymax = int(want_y.max())
        last = setup.clock0 + nt * ymax - 1
        for k in all_fields(setup.model):
            fs = eng.field_step(k)
            assert fs["current"] and fs["state_step"] == last and fs["written_step"] == last, (k, fs)
            field = eng.get_field(k)
            for c in range(setup.ncol):
                assert np.array_equal(field[c], snaps[k][want_y[c]][c], equal_nan=True), (k, c, want_y[c])
        got["counters"] = eng.counters()
        assert got["counters"]["steps"] == nt * ymax
    return got, snaps, tol


def assert_honest(got, snaps, setup, max_years):
    y, c = got["years"], got["converged"]
    assert len(set(y.tolist())) > 1, "the equilibrium years are all equal"
    assert (c & (y < max_years)).any(), "no column converges before max_years"
    assert not c.all(), "every column converges"
    moved = [i for i in range(setup.ncol) if c[i] and y[i] < max_years and
             any(not np.array_equal(snaps[k][max_years][i], snaps[k][y[i]][i]) for k in all_fields(setup.model))]
    assert moved, "no frozen column would have moved on: a build that keeps stepping frozen columns would pass"


MAX_YEARS = 8


@pytest.mark.parametrize("K", [1, 64])
@pytest.mark.parametrize("chains", [1, 2])
@pytest.mark.parametrize("in_lds", [0, 1])
@pytest.mark.parametrize("cells", [2, 4])
@pytest.mark.parametrize("grid", ["identity", "sin"])
def test_miz_matrix(pkg, grid, cells, in_lds, chains, K):
    setup = Setup(pkg, "MIZ", grid, 180, 2000, 12, cells_per_thread=cells, fused_state_in_lds=bool(in_lds),
                  launch_chains=chains, use_graph=False, integrate_steps_per_launch=K)
    got, snaps, _ = check_against_reference(setup, ("T",), MAX_YEARS)
    assert_honest(got, snaps, setup, MAX_YEARS)


@pytest.mark.parametrize("nlat", [1024, 4096])
def test_imex_long_meridians(pkg, nlat):
    """Warm open water under strong forcing (test_gpu_imex.py: the extension is stable there at the reference test's time
    step on any meridian), members started from open water of 10 ... 60 degrees."""
    cw = pkg.default_parameters("MIZ")["cw"]
    start = {k: np.zeros((8, nlat)) for k in PROG}
    start["Ew"] = np.outer(np.linspace(10.0, 60.0, 8), np.full(nlat, cw))
    setup = Setup(pkg, "MIZ_IMEX", "sin", nlat, 2000, 8, fcol=np.linspace(50.0, 60.0, 8), start=start, launch_chains=2,
                  use_graph=False)
    got, snaps, _ = check_against_reference(setup, ("T",), MAX_YEARS)
    assert_honest(got, snaps, setup, MAX_YEARS)


@pytest.mark.parametrize("K", [1, 64])
def test_classic(pkg, K):
    setup = Setup(pkg, "Classic", "identity", 180, 2000, 12, integrate_steps_per_launch=K)
    got, snaps, _ = check_against_reference(setup, ("T",), MAX_YEARS)
    assert_honest(got, snaps, setup, MAX_YEARS)


@pytest.mark.parametrize("names", [("Ei", "h"), ("T", "n"), ("phi", "Ew", "T")], ids=["prognostic", "diagnostic", "both"])
def test_criteria(pkg, names):
    setup = Setup(pkg, "MIZ", "sin", 180, 2000, 12)
    got, snaps, _ = check_against_reference(setup, names, MAX_YEARS)
    assert_honest(got, snaps, setup, MAX_YEARS)


def test_one_year_and_min_years(pkg):
    setup = Setup(pkg, "MIZ", "identity", 180, 2000, 12)
    snaps = reference(setup, MAX_YEARS)
    got, _, _ = check_against_reference(setup, ("T",), 1, snaps=snaps, tol=[1e9])
    assert (got["years"] == 1).all() and not got["converged"].any() and np.isnan(got["resid"]["T"]).all()
    # min_years = 5: every column would converge at year 2 with a huge tolerance; none may stop before year 5
    got, _, _ = check_against_reference(setup, ("T",), MAX_YEARS, min_years=5, snaps=snaps, tol=[1e9])
    assert (got["years"] == 5).all() and got["converged"].all()
    d = distances(snaps, ("T",))
    got, _, _ = check_against_reference(setup, ("T",), MAX_YEARS, min_years=5, snaps=snaps, tol=[np.nanmedian(d[0, 5])])
    assert got["years"].min() >= 5 and got["converged"].any()


def test_model_time_continues_from_the_step_clock(pkg):
    """Every other case here starts at step 0.  From a step clock of three years the years of the call are steps
    clock0 + (y - 1) nt onwards, as the second handle's plain runs take them: the fields are as of step
    clock0 + nt * years - 1 (check_against_reference asks field_step for it)."""
    setup = Setup(pkg, "MIZ", "sin", 16, 200, 4)
    setup.clock0 = 3 * 200
    got, _, _ = check_against_reference(setup, ("T",), 3, tol=[1e9])
    assert (got["years"] == 2).all() and got["converged"].all()


# nlat -> the row of each column's one ice cell.  The check kernel walks a column with 256 threads, four waves whose maxima
# meet in LDS: 65 rows are one wave and one lane of the second; 193 reach the fourth wave with one lane (row 192); 257 are one
# full stride and row 256, the first of the second; 513 two full strides and one row.  Rows 200 and 255 lie in the fourth
# wave's 192 .. 255, rows 256, 300 and 511 in the second stride, 512 in the third.
CHECK_ROWS = {65: (0, 33, 63, 64), 193: (10, 100, 191, 192), 257: (100, 200, 255, 256), 513: (200, 300, 511, 512)}


@pytest.mark.parametrize("nlat", sorted(CHECK_ROWS))
def test_residuals_are_the_max_of_the_year_end_differences(pkg, nlat):
    """The residuals against NumPy's max |cur - prev| over the fields a second handle gives at two consecutive year ends, bit
    for bit: a max of exact differences does not depend on the order of the reduction.  Which rows differ is chosen, not
    drawn: every column is warm open water (h = Ei = 0 in every row, and they stay exactly 0 while nothing freezes) but for
    ONE cell of pack ice, in a different row per column (CHECK_ROWS), so h and Ei differ between the two year ends in that
    row alone — the test asserts it — while T differs in every row.  A "year" is 16 steps of 5e-7 years: real steps, and the
    ice cell neither melts away nor spreads in 32 of them."""
    rows = CHECK_ROWS[nlat]
    ncol, nt, names = len(rows), 16, ("T", "h", "Ei")
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    g = load_golden("miz_sin_180_2000.npz")
    state = {k: np.zeros((ncol, nlat)) for k in PROG + ("T0",)}
    state["Ew"][:] = 21.0
    for c, r in enumerate(rows):
        for k in state:
            state[k][c, r] = g[f"s1000_{k}"][-1]                     # the fixture's polar cell: phi = 1, h = 1.9 m
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)

    def engine():
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, 5e-7, ncol, device=0)
        eng.set_time_table(st.t)
        eng.set_state(state)
        return eng
    with engine() as ref:
        ref.run(0, nt, None, True, 64)
        prev = {k: ref.get_field(k) for k in names}
        ref.run(nt, nt, None, True, 64)
        cur = {k: ref.get_field(k) for k in names}
    for c, r in enumerate(rows):
        for k in ("h", "Ei"):
            assert list(np.flatnonzero(cur[k][c] != prev[k][c])) == [r], (k, c, r)
        assert np.count_nonzero(cur["T"][c] != prev["T"][c]) >= nlat - 1
    with engine() as eng:
        got = eng.equilibrate(nt, 2, None, {k: 1e9 for k in names})
    assert (got["years"] == 2).all() and got["converged"].all()
    for k in names:
        want = np.max(np.abs(cur[k] - prev[k]), axis=1)
        assert (want > 0.0).all(), k
        assert np.array_equal(got["resid"][k].view(np.int64), want.view(np.int64)), (k, got["resid"][k], want)


def test_sharding_invariance(pkg):
    setup = Setup(pkg, "MIZ", "sin", 180, 2000, 12)
    got, snaps, tol = check_against_reference(setup, ("T",), MAX_YEARS)
    halves = [slice(0, 6), slice(6, 12)]
    for h in halves:
        with setup.engine(h) as eng:
            part = eng.equilibrate(setup.st.nt, MAX_YEARS, None, {"T": tol[0]})
            assert np.array_equal(part["years"], got["years"][h])
            assert np.array_equal(part["converged"], got["converged"][h])
            assert np.array_equal(part["resid"]["T"], got["resid"]["T"][h], equal_nan=True)
            for k in MIZ_ALL:
                f = eng.get_field(k)
                for i, c in enumerate(range(12)[h]):
                    assert np.array_equal(f[i], snaps[k][got["years"][c]][c], equal_nan=True), (k, c)


def test_nan_column(pkg):
    """A NaN column reports converged = 0 and NaN residuals; the others give the bits they give without it."""
    setup = Setup(pkg, "MIZ", "sin", 16, 200, 4)
    good = {k: v.copy() for k, v in setup.state.items()}
    for k in setup.state:
        setup.state[k][1] = np.nan
    with setup.engine() as eng:
        got = eng.equilibrate(200, 2, None, {"T": 1e9, "Ei": 1e9})
        bad_state = eng.get_state(MIZ_ALL)
    assert list(got["converged"]) == [True, False, True, True]
    assert list(got["years"]) == [2, 2, 2, 2]
    for k in ("T", "Ei"):
        assert np.isnan(got["resid"][k][1]) and np.isfinite(got["resid"][k][[0, 2, 3]]).all()
    setup.state = good
    with setup.engine() as eng:
        ref = eng.equilibrate(200, 2, None, {"T": 1e9, "Ei": 1e9})
        good_state = eng.get_state(MIZ_ALL)
    for k in ("T", "Ei"):
        assert np.array_equal(got["resid"][k][[0, 2, 3]], ref["resid"][k][[0, 2, 3]])
    for k in MIZ_ALL:
        assert np.array_equal(bad_state[k][[0, 2, 3]], good_state[k][[0, 2, 3]], equal_nan=True), k


def test_fields_readable_and_natural_afterwards(pkg):
    """Entered with the diagnostic fields pair-split by a one-launch-per-step step: afterwards every field is current and
    the zero-copy view shows the natural layout."""
    import torch
    hip = C.CDLL("libamdhip64.so")
    setup = Setup(pkg, "MIZ", "identity", 180, 2000, 12, cells_per_thread=4)
    snaps = reference(setup, 2)
    with setup.engine() as eng:
        eng.run(0, 1, None, True, 1)                       # (ebm_run: the step kernel stores the diagnostics split)
        eng.set_state(setup.state)                         # the start state again: prognostics and T0 only
        eng.set_step_clock(0)
        got = eng.equilibrate(2000, 2, None, {"T": 1e9})
        assert (got["years"] == 2).all() and got["converged"].all()
        for k in DIAG + ("T0",):
            assert eng.field_step(k)["current"], k
            ptr, pitch = eng.field_device_ptr(k)
            view = np.empty((12, pitch))
            torch.cuda.synchronize()
            assert hip.hipMemcpy(view.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(view.nbytes), 2) == 0
            assert np.array_equal(view[:, :180], snaps[k][2], equal_nan=True), k
            assert not view[:, 180:].any()
        assert np.array_equal(eng.hemispheric_mean("T"), pkg.hemispheric_mean(snaps["T"][2], setup.st.x))
        for k in PROG:
            assert np.array_equal(eng.get_field(k), snaps[k][2]), k


def test_refusals_leave_the_handle_alone(pkg):
    setup = Setup(pkg, "MIZ", "sin", 16, 200, 4)
    import sys
    F = sys.modules[pkg.__name__ + "._lib"].FIELD
    with setup.engine() as eng:
        lib = eng.lib
        eng.run(0, 200, None, True, 64)
        before = eng.get_state(MIZ_ALL)
        steps = {k: eng.field_step(k) for k in MIZ_ALL}
        count = eng.counters()
        ip = C.POINTER(C.c_int)
        years = np.zeros(4, dtype=np.int32)
        conv = np.zeros(4, dtype=np.int32)

        def call(nt, max_years, fields, tol):
            f = (C.c_int * len(fields))(*fields)
            t = np.asarray(tol, dtype=np.float64)
            return lib.ebm_equilibrate(eng._h, nt, max_years, 2, None, len(fields), f, t.ctypes.data_as(C.POINTER(C.c_double)),
                                       years.ctypes.data_as(ip), conv.ctypes.data_as(ip), None)
        cases = [(199, 5, [F["T"]], [1.0], -1), (200, 0, [F["T"]], [1.0], -1), (200, 5, [F["T"]], [-1.0], -1),
                 (200, 5, [F["T"]], [np.nan], -1), (200, 5, [F["T0"]], [1.0], -1), (200, 5, [F["Tg"]], [1.0], -1),
                 (200, 5, [F["T"], F["Ei"], F["T"]], [1.0, 1.0, 1.0], -1), (200, 5, [99], [1.0], -1)]
        for nt, my, fields, tol, rc in cases:
            assert call(nt, my, fields, tol) == rc, (nt, my, fields, tol)
        eng.set_column_schedules([pkg.Forcing(0.0)] * 4)
        assert call(200, 5, [F["T"]], [1.0]) == -3
        assert b"schedules" in lib.ebm_last_error()
        eng.set_column_schedules(None)
        assert (years == 0).all() and (conv == 0).all()
        assert eng.counters() == count
        for k in MIZ_ALL:
            assert eng.field_step(k) == steps[k], k
            assert np.array_equal(eng.get_field(k), before[k], equal_nan=True), k
        # and the handle still works
        got = eng.equilibrate(200, 3, None, {"T": 1e9})
        assert (got["years"] == 2).all()


def test_engine_and_ensemble_surfaces(pkg):
    """EnsembleRun.equilibrate (constant forcing, member parameters, offsets) gives the bits of Engine.equilibrate."""
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    par = pkg.default_parameters("MIZ")
    g = golden_state(pkg, "MIZ", st, 1)
    init = {k: v[0] for k, v in g.items() if k != "T0"}
    mp = [{"D": d} for d in np.linspace(0.5, 0.7, 6)]
    fcol = np.linspace(-1.0, 1.0, 6)
    run = pkg.EnsembleRun("MIZ", st, par, init, fcol=fcol, member_params=mp)
    try:
        with pytest.raises(ValueError, match="constant forcing"):
            run.equilibrate(4, {"T": 1e-2}, forcing=pkg.Forcing(0.0, 10.0, -10.0, (1, 1), (1.0, -1.0)))
        out = run.equilibrate(4, {"T": 1e-2}, forcing=pkg.Forcing(0.5))
        assert run.step_index == st.nt * int(out["years"].max())
        ens_state = run.state(MIZ_ALL)
    finally:
        run.close()
    rows = pkg.engine.param_matrix(mp, par, pkg.default_parval)
    with pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, 6) as eng:
        eng.set_state({k: np.tile(v, (6, 1)) for k, v in init.items()})
        eng.set_column_forcing(fcol)
        eng.set_time_table(st.t)
        eng.set_column_params(rows)
        got = eng.equilibrate(st.nt, 4, np.full(st.nt, 0.5), {"T": 1e-2})
        eng_state = eng.get_state(MIZ_ALL)
    assert np.array_equal(out["years"], got["years"]) and np.array_equal(out["converged"], got["converged"])
    assert np.array_equal(out["resid"]["T"], got["resid"]["T"], equal_nan=True)
    for k in MIZ_ALL:
        assert np.array_equal(ens_state[k], eng_state[k], equal_nan=True), k
    with pytest.raises(ValueError, match="built with forcings="):
        run2 = pkg.EnsembleRun("MIZ", st, par, init, forcings=[pkg.Forcing(0.0)] * 2)
        try:
            run2.equilibrate(2)
        finally:
            run2.close()
