"""GPU tests (-m gpu) of the state-only one-step kernel that derives phi from Ei and h instead of loading and storing it
(csrc/ebm_miz_step.h, PHI_DERIVED; FieldBook::phi_stored / phi_consistent, csrc/ebm_fieldbook.h).

After any step phi is concentration(Ei, h) of the stored fields, so nothing a caller can see may change: every comparison
here is bitwise (uint64 views, NaN patterns included) and sets no tolerance.  The partner is always a path that stores phi:
the same calls on a second handle with every `run` taken as ebm_run_fused with K = 2, whose kernels keep the natural layout
and write all five prognostic fields.

Start state: the golden mid-year state (ice, open water, an ice edge, cells with phi == 1) spread onto the grid by nearest
cell (support.midyear_state); the first step after it loads the caller's phi, every later one derives it.  The C
oracle steps the same state once per shape (shared) to show that the trajectories compared are finite, not NaN against NaN.

Shapes, at four cells per thread: 258 x 3 (128 threads, padding in the last thread), 1025 x 2 (320 threads, a lone cell in
a pair), 4096 x 2 (1024 threads: the headline kernel), 180 x 5 (64 threads).  Both grids.
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, assert_same_bits as same, forcing_of as forcing, midyear_state

pytestmark = pytest.mark.gpu

SHAPES = [(258, 3), (1025, 2), (4096, 2), (180, 5)]
THREADS = {258: 128, 1025: 320, 4096: 1024, 180: 64}
# steps per year, nt >= nlat^2 / 4: its own table, not support.steps_per_year, because 4096 cells are stepped by the explicit model here
NT = {180: 2000, 258: 20000, 1025: 270000, 4096: 4200000}
TABLE = 256            # time-table entries from mid-year on: every test takes fewer steps than that
MAX_STEPS = 134        # the most steps any test here takes from the start state


class Space:
    """The grid of SpaceTime(grid, nlat, NT[nlat], 1), its time step, and the TABLE mid-year entries of its st.t (a
    SpaceTime of millions of steps takes seconds to build)."""

    def __init__(self, pkg, grid, nlat):
        st = pkg.SpaceTime(grid, nlat, 2000, 1)
        self.x, self.grid_kind, self.dt = st.x, st.grid_kind, 1.0 / NT[nlat]
        self.t = np.array([(2 * i + 1) / (2.0 * NT[nlat]) for i in range(NT[nlat] // 2, NT[nlat] // 2 + TABLE)])


@functools.lru_cache(maxsize=None)
def space(pkg, grid, nlat):
    st = Space(pkg, grid, nlat)
    return st, st.t


def offsets(ncol):
    return np.linspace(-1.5, 1.5, ncol)


@functools.lru_cache(maxsize=None)
def start_state(pkg, grid, nlat):
    """One column of support.midyear_state on this file's grid."""
    st, _ = space(pkg, grid, nlat)
    state = {k: np.ascontiguousarray(v[0]) for k, v in midyear_state("MIZ", st, 1).items()}
    # (open water, h == 0, on the sin grid only: the identity fixture has ice in every cell)
    assert (state["phi"] == 1.0).any() and ((state["phi"] > 0) & (state["phi"] < 1)).any()
    assert grid == "identity" or (state["h"] == 0.0).any()
    return state


@functools.lru_cache(maxsize=None)
def oracle_is_finite(pkg, coracle, grid, nlat, ncol):
    """MAX_STEPS steps of the C oracle from the start state with the tests' forcing: every prognostic field stays finite."""
    st, tab = space(pkg, grid, nlat)
    state = {k: np.ascontiguousarray(np.tile(v, (ncol, 1))) for k, v in start_state(pkg, grid, nlat).items()}
    ct = np.array([pkg.cos2pit(float(t)) for t in tab[:MAX_STEPS]])
    with np.errstate(all="ignore"):
        coracle.miz_run(0 if grid == "identity" else 1, st.x, dict(pkg.default_parameters("MIZ")), st.dt, ct,
                        forcing(0, MAX_STEPS), offsets(ncol), state)
    return all(np.isfinite(state[k]).all() for k in PROG)


def open_engine(pkg, grid, nlat, ncol, setup=None, **opt):
    st, tab = space(pkg, grid, nlat)
    par = pkg.default_parameters("MIZ")
    opt.setdefault("use_graph", False)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0, **opt)
    info = eng.launch_info()
    assert info["threads"] == THREADS[nlat] and info["cells_per_thread"] == 4
    eng.set_column_forcing(offsets(ncol))
    eng.set_time_table(tab)
    if setup is not None:
        setup(eng)
    eng.set_state({k: np.tile(v, (ncol, 1)) for k, v in start_state(pkg, grid, nlat).items()})
    return eng


class Pair:
    """Two handles at the same state: `one` steps with one launch per step (the kernel under test), `two` with ebm_run_fused
    at K = 2.  Every other call goes to both."""

    def __init__(self, pkg, grid, nlat, ncol, setup=None, **opt):
        self.one = open_engine(pkg, grid, nlat, ncol, setup, **opt)
        self.two = open_engine(pkg, grid, nlat, ncol, setup, **{k: v for k, v in opt.items() if k != "use_graph"})
        self.pos = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.one.close()
        self.two.close()
        return False

    def run(self, n, diag=False, fused_too=False):
        f = forcing(self.pos, n)
        self.one.run(self.pos, n, f, diag, steps_per_launch=2 if fused_too else 1)
        self.two.run(self.pos, n, f, diag, steps_per_launch=2)
        self.pos += n

    def both(self, call):
        a, b = call(self.one), call(self.two)
        if a is not None:
            same(a, b)
        return a

    def check(self, what=""):
        same(self.one.get_state(PROG), self.two.get_state(PROG), what)


GRIDS = ["sin", "identity"]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_start_state_steps_to_finite_values(pkg, coracle, grid, nlat, ncol):
    assert oracle_is_finite(pkg, coracle, grid, nlat, ncol)


@pytest.mark.parametrize("nsteps,graph", [(1, False), (2, False), (7, False), (130, False), (130, True)])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_steps_equal_the_steps_that_store_phi(pkg, grid, nlat, ncol, nsteps, graph):
    """1, 2, 7 and 130 steps of ebm_run (130: graph replay of 64 steps and direct steps, or direct steps only) against the
    fused path, all five prognostic fields with phi read back."""
    with Pair(pkg, grid, nlat, ncol, use_graph=graph) as p:
        p.run(nsteps)
        p.check()
        got = p.one.get_state(PROG)
        assert all(np.isfinite(v).all() for v in got.values())
        assert not np.array_equal(got["Ew"], np.tile(start_state(pkg, grid, nlat)["Ew"], (ncol, 1)))


# what a caller writes over one field: values that break phi == f(Ei, h) and from which the model still steps to finite
# values (a phi BELOW -Ei / (Lf h), e.g. phi * 0.5, turns the reference's step into NaN within three steps, and NaN against
# NaN compares payloads that no contract fixes; checked below with the oracle)
PERTURB = {"phi": lambda v: np.where(v < 0.8, v * 1.25, v), "h": lambda v: v * 1.25, "Ei": lambda v: v * 0.5}
CALLER_SHAPES = [("sin", 258, 3), ("identity", 180, 5), ("sin", 4096, 2)]


@functools.lru_cache(maxsize=None)
def oracle_after_a_callers_field(pkg, coracle, grid, nlat, ncol, name):
    """4 steps, the field overwritten, 3 steps with the C oracle: (the field differs from what it was, all finite)"""
    st, tab = space(pkg, grid, nlat)
    state = {k: np.ascontiguousarray(np.tile(v, (ncol, 1))) for k, v in start_state(pkg, grid, nlat).items()}
    par, kind = dict(pkg.default_parameters("MIZ")), 0 if grid == "identity" else 1
    ct = np.array([pkg.cos2pit(float(t)) for t in tab[:7]])
    with np.errstate(all="ignore"):
        coracle.miz_run(kind, st.x, par, st.dt, ct[:4], forcing(0, 4), offsets(ncol), state)
        new = PERTURB[name](state[name])
        changed = not np.array_equal(new, state[name])
        state[name] = np.ascontiguousarray(new)
        coracle.miz_run(kind, st.x, par, st.dt, ct[4:], forcing(4, 3), offsets(ncol), state)
    return changed, all(np.isfinite(state[k]).all() for k in PROG)


@pytest.mark.parametrize("name", sorted(PERTURB))
@pytest.mark.parametrize("grid,nlat,ncol", CALLER_SHAPES)
def test_a_callers_field_keeps_the_oracle_finite(pkg, coracle, grid, nlat, ncol, name):
    assert oracle_after_a_callers_field(pkg, coracle, grid, nlat, ncol, name) == (True, True)


@pytest.mark.parametrize("nsteps", [1, 3])
@pytest.mark.parametrize("name", sorted(PERTURB))
@pytest.mark.parametrize("grid,nlat,ncol", CALLER_SHAPES)
def test_a_callers_field_is_honoured(pkg, grid, nlat, ncol, name, nsteps):
    """After steps that derived phi, one of phi, h, Ei is overwritten with values that break phi == f(Ei, h): the next step
    uses the phi that is stored, as the fused path does from the same uploaded state."""
    with Pair(pkg, grid, nlat, ncol) as p:
        p.run(4)
        new = PERTURB[name](p.two.get_field(name))
        p.both(lambda e: e.set_field(name, new))
        p.run(nsteps)
        p.check(name)
        got = p.one.get_state(PROG)
        assert all(np.isfinite(v).all() for v in got.values())
        assert not np.array_equal(got["phi"], np.zeros((ncol, nlat)))


def parents_of(ncol):
    return np.array([(c + 1) % ncol if c % 2 == 0 else c for c in range(ncol)], dtype=np.int32)


READERS = {
    "get_field": lambda e, pos: e.get_field("phi"),
    "hemispheric_mean": lambda e, pos: e.hemispheric_mean("phi"),
    "resample": lambda e, pos: e.resample_columns(parents_of(e.ncol)),
}


@pytest.mark.parametrize("reader", sorted(READERS) + ["series", "diag_last"])
@pytest.mark.parametrize("grid,nlat,ncol", [("sin", 258, 3), ("identity", 180, 5), ("sin", 4096, 2)])
def test_readers_see_the_current_phi(pkg, grid, nlat, ncol, reader):
    """After steps that did not store phi: the field, its hemispheric mean, a series of it, a diagnostic last step (E, T,
    T0 need the new phi) and a resampling give what they give on the handle that stored it; then the stepping goes on."""
    with Pair(pkg, grid, nlat, ncol) as p:
        p.run(5)
        if reader == "series":
            f = forcing(p.pos, 4)
            a = p.one.run_series(p.pos, 4, 2, ("phi", "Ei"), f, 1)
            b = p.two.run_series(p.pos, 4, 2, ("phi", "Ei"), f, 2)
            same(a, b)
            p.pos += 4
        elif reader == "diag_last":
            p.run(3, diag=True)
            same(p.one.get_state(("E", "T", "T0")), p.two.get_state(("E", "T", "T0")))
        else:
            p.both(lambda e: READERS[reader](e, p.pos))
        p.check("after the reader")
        p.run(3)
        p.check("stepping on")


@pytest.mark.parametrize("grid,nlat,ncol", [("sin", 258, 3), ("identity", 1025, 2)])
def test_interleaved_calls(pkg, grid, nlat, ncol):
    """run(5), get_field, run(5), run_fused(4, K = 2), run(3), set_field(h), run(2) against the same calls with every run
    fused."""
    with Pair(pkg, grid, nlat, ncol) as p:
        p.run(5)
        p.both(lambda e: e.get_field("phi"))
        p.run(5)
        p.run(4, fused_too=True)
        p.run(3)
        new = p.two.get_field("h") * 1.25
        p.both(lambda e: e.set_field("h", new))
        p.run(2)
        p.check()


def two_latent_heats(pkg):
    def setup(eng):
        par = pkg.default_parameters("MIZ")
        # (the larger Lf in the even columns, which parents_of fills from odd ones: a phi made under the smaller Lf lies above
        # -Ei / (Lf h) of its new column, from where the model steps on to finite values; the other way round it gives NaN)
        rows = [{"Lf": par["Lf"] * (1.25 if c % 2 == 0 else 1.0)} for c in range(eng.ncol)]
        eng.set_column_params(pkg.engine.param_matrix(rows, par, pkg.default_parval))
    return setup


@pytest.mark.parametrize("variant", ["two_chains", "two_Lf", "noise"])
@pytest.mark.parametrize("grid,nlat", [("sin", 258), ("identity", 180), ("sin", 4096)])
def test_launch_and_parameter_variants(pkg, grid, nlat, variant):
    """Two launch chains (7 columns, 3 / 4), per-column parameter sets with two latent heats Lf (phi = -Ei / (Lf h) takes
    the column's own), forcing noise: 5 steps against the fused path, then phi's readers."""
    ncol = 7 if nlat < 4096 else 3
    opt, setup = {}, None
    if variant == "two_chains":
        opt = {"launch_chains": 2}
    elif variant == "two_Lf":
        setup = two_latent_heats(pkg)
    else:
        setup = lambda eng: eng.set_column_noise(0.8, rho=0.9, seed=11)       # noqa: E731
    with Pair(pkg, grid, nlat, ncol, setup, **opt) as p:
        p.run(5)
        p.check(variant)
        assert all(np.isfinite(v).all() for v in p.one.get_state(PROG).values())
        if variant == "two_Lf":
            # phi moves with its column, made under the parent's Lf, to a column of the other set
            p.both(lambda e: e.resample_columns(parents_of(ncol)))
            p.check("resampled")
            p.run(3)
            p.check("stepping on")
            assert all(np.isfinite(v).all() for v in p.one.get_state(PROG).values())


def test_a_restore_with_nothing_stale_does_nothing(pkg):
    """The first read of phi after derived steps restores it inside the one un-split pass (one conversion); a second read
    returns the same bits, converts nothing and launches no step.  (An in-place restore moves neither counter: that a
    redundant one is not launched rests on restore_phi returning at once when phi_stored is set.)"""
    with open_engine(pkg, "sin", 258, 3) as eng:
        eng.run(0, 6, None, False)
        before = eng.state_conversions()
        a = eng.get_field("phi")
        launches, conversions = eng.counters()["launches"], eng.state_conversions()
        b = eng.get_field("phi")
        same(a, b)
        assert eng.counters()["launches"] == launches and eng.state_conversions() == conversions == before + 1
        eng.hemispheric_mean("phi")
        assert eng.state_conversions() == conversions
