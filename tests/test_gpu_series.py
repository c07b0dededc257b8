"""GPU tests (-m gpu) of ebm_run_series (include/ebm_hip.h): the time series of per-column hemispheric means sampled on the
device between fused launches.

The definition is an identity with entry points the library already has, so no test here needs an oracle: sample j of the
series is bit for bit what ebm_hemispheric_mean returns after ebm_run_fused of (j+1)*every steps, and the handle ends as
after one ebm_run_fused of all the steps.  A second handle is advanced sample by sample through those two calls (once per
case, shared by the tests) and everything is compared on the bit patterns, NaN sentinels included.

Shapes: the kernel walks the nlat - 1 terms of a meridian in tiles of 512 with one wave of 64 lanes, so nlat = 2 (one
term), 3, 65 (one term per lane), 180, 258, 513 (exactly one tile), 1025 (exactly two) and 4096 (the largest meridian; eight
tiles, the last one short).  Meridians of more than 180 cells step with the explicit model only where its time step is
stable (nt >= nlat^2 / 4); the 4096-cell cases use the implicit-diffusion extension, which has no such limit.
"""
import ctypes
import functools

import numpy as np
import pytest

import support
from support import (CLASSIC_VARS, MIZ_DIAG as DIAG, MIZ_PROG as PROG, assert_same_snapshot, forcing_of, is_diagnostic, is_miz,
                     midyear_state, same_bits, snapshot)

pytestmark = pytest.mark.gpu

MIZ_VARS = PROG + DIAG


def make_engine(pkg, model, grid, nlat, ncol, cells=4, setup=None, **opt):
    """support.make_engine with a single column's forcing offset at 0.25, as these tests have always had it."""
    return support.make_engine(pkg, model, grid, nlat, ncol, cells, setup=setup, single_offset=0.25, **opt)


def names_of(model, kind):
    if kind == "all":
        return MIZ_VARS if is_miz(model) else CLASSIC_VARS
    if kind == 2:
        return ("T", "phi") if is_miz(model) else ("T", "Tg")
    return ("phi",) if is_miz(model) else ("E",)          # prognostic only: no diagnostic step is taken


def first_step(st):
    return st.nt // 2


def by_hand(pkg, eng, st, model, first, nsteps, every, K, names, f):
    """The host loop the definition names: ebm_run_fused for `every` steps, then ebm_hemispheric_mean per variable; and the
    NumPy restatement of the mean applied to the downloaded fields."""
    diag = any(is_diagnostic(model, n) for n in names)
    ns = nsteps // every
    dev = np.empty((len(names), ns, eng.ncol))
    host = np.empty_like(dev)
    for j in range(ns):
        eng.run(first + j * every, every, f[j * every:(j + 1) * every], diag, K)
        for v, n in enumerate(names):
            dev[v, j] = eng.hemispheric_mean(n)
            host[v, j] = pkg.hemispheric_mean(eng.get_field(n), st.x)
    return dev, host


# model, grid, nlat, ncol, cells per thread, every, steps per launch, variables, nsteps
CASES = [
    ("MIZ", "identity", 180, 70, 4, 7, 16, 2, 70),
    ("MIZ", "sin", 180, 1, 2, 1, 1, "all", 24),
    ("MIZ_IMEX", "identity", 4096, 3, 4, 64, 1, "all", 128),          # split layout, eight tiles, every variable
    ("MIZ_IMEX", "sin", 4096, 3, 4, 100, 64, 1, 200),
    ("MIZ", "sin", 1025, 70, 4, 100, 64, "all", 200),                 # two launches per sample, two full tiles
    ("MIZ", "identity", 513, 1, 2, 64, 64, 1, 128),
    ("MIZ", "identity", 65, 1, 2, 64, 1, "all", 64),
    ("MIZ_IMEX", "sin", 258, 70, 4, 100, 16, "all", 400),             # one term into the second tile
    ("MIZ", "identity", 2, 1, 4, 1, 64, 2, 8),
    ("MIZ", "sin", 3, 70, 4, 1, 1, "all", 12),                        # split layout at the smallest workgroup
    ("Classic", "identity", 65, 70, 4, 7, 1, "all", 42),
    ("Classic", "identity", 3, 1, 2, 1, 16, 2, 10),
    ("Classic", "identity", 180, 70, 4, 64, 64, 1, 128),
]
IDS = ["-".join(str(x) for x in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def run_case(pkg, case):
    """One ebm_run_series on a first handle, the loop by hand on a second: computed once per case, read by every test."""
    model, grid, nlat, ncol, cells, every, K, kind, nsteps = case
    names = names_of(model, kind)
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells)
    first = first_step(st)
    f = forcing_of(first, nsteps)
    with eng:
        series = eng.run_series(first, nsteps, every, names, f, K)
        after = snapshot(eng, model)
    ref, _ = make_engine(pkg, model, grid, nlat, ncol, cells)
    with ref:
        dev, host = by_hand(pkg, ref, st, model, first, nsteps, every, K, names, f)
        ref_after = snapshot(ref, model)
    return dict(series=series, after=after, dev=dev, host=host, ref_after=ref_after, names=names)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_series_is_the_loop_of_existing_calls(pkg, case):
    r = run_case(pkg, case)
    assert r["series"].shape == (len(r["names"]), case[8] // case[5], case[3])
    for v, n in enumerate(r["names"]):
        assert same_bits(r["series"][v], r["dev"][v]), (case, n)
    assert_same_snapshot(r["after"], r["ref_after"], case)
    if case[7] == "all" and is_miz(case[0]):
        assert np.isnan(r["series"]).any(), "the mid-year state has NaN sentinels in Ti / Tw: their means are NaN"
    prognostic = [v for v, n in enumerate(r["names"]) if n in PROG + ("E", "Tg", "T")]
    assert np.isfinite(r["series"][prognostic]).all(), "the state has blown up: the comparison is of NaNs"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_series_is_the_numpy_mean_of_the_fields(pkg, case):
    r = run_case(pkg, case)
    assert same_bits(r["series"], r["host"]), case


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_launch_and_step_counters(pkg, case):
    model, grid, nlat, ncol, cells, every, K, kind, nsteps = case
    c = run_case(pkg, case)["after"]["counters"]
    assert c["steps"] == nsteps
    assert c["launches"] == (nsteps // every) * -(-every // K)


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[10]], ids=[IDS[0], IDS[4], IDS[10]])
def test_two_calls_compose(pkg, case):
    model, grid, nlat, ncol, cells, every, K, kind, nsteps = case
    r = run_case(pkg, case)
    half = nsteps // 2
    assert half % every == 0
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells)
    first = first_step(st)
    f = forcing_of(first, nsteps)
    with eng:
        a = eng.run_series(first, half, every, r["names"], f[:half], K)
        b = eng.run_series(first + half, half, every, r["names"], f[half:], K)
        after = snapshot(eng, model)
    assert same_bits(np.concatenate([a, b], axis=1), r["series"])
    assert_same_snapshot(after, r["after"], case)


# ---- the one-field entry points walk the same tiles -----------------------------------------------------------------------

@pytest.mark.parametrize("nlat", [2, 3, 65, 513, 514, 1025, 1026])
def test_hemispheric_mean_at_tile_boundaries(pkg, nlat):
    """ebm_hemispheric_mean and ebm_hemispheric_mean_device go through the mean kernel of the series, which walks the
    nlat - 1 terms in tiles of 512: 1, 2 and 64 terms, exactly one tile, one tile plus one term, exactly two tiles, two
    tiles plus one term.  Fields the caller set — T, a diagnostic field, and Ei, a prognostic one (the un-split path) — of
    seeded normal values, with a NaN in column 1 at cell 512 where it exists (it enters the last term of tile 1 and the
    first of tile 2) and +inf in column 2 at cell 0; against the host's sequential loop, bit for bit."""
    import torch
    ncol = 3
    st = pkg.SpaceTime("sin", nlat, 2000, 1)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    rng = np.random.default_rng(nlat)
    with pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0) as eng:
        for name in ("T", "Ei"):
            field = rng.standard_normal((ncol, nlat))
            if nlat > 512:
                field[1, 512] = np.nan
            field[2, 0] = np.inf
            eng.set_field(name, field)
            want = pkg.hemispheric_mean(field, st.x)
            assert np.isfinite(want[0]) and np.isnan(want[1]) == (nlat > 512) and want[2] == np.inf
            assert np.array_equal(eng.hemispheric_mean(name), want, equal_nan=True), (nlat, name)
            out = torch.empty(ncol, dtype=torch.float64, device="cuda:0")
            eng.hemispheric_mean_device(name, out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), (nlat, name, "device output")


@pytest.mark.parametrize("nlat", [257, 258])
def test_both_mean_kernels_at_the_launcher_rule(pkg, nlat):
    """The launcher gives ONE field of a meridian of more than 256 terms (nlat - 1 > 256) to the 256-lane kernel and everything
    else to the 64-lane one: 257 latitudes are the last shape the small kernel takes with one field, 258 the first the large
    one takes.  The series of each of three fields alone, and of the three together (always 64 lanes), against the
    reference's sequential sum restated in NumPy on the downloaded fields, bit for bit — and so the same bits from both
    kernels.  test_hemispheric_mean_at_tile_boundaries already holds the 256-lane kernel to that sum at 513 latitudes and
    more, through ebm_hemispheric_mean; it runs neither side of the rule's threshold and never several fields."""
    model, grid, ncol, cells, every, K, nsteps, names = "MIZ", "sin", 3, 4, 4, 4, 8, ("T", "phi", "Ei")

    def series(which):
        eng, st = make_engine(pkg, model, grid, nlat, ncol, cells)
        first = first_step(st)
        with eng:
            return eng.run_series(first, nsteps, every, which, forcing_of(first, nsteps), K)
    ref, st = make_engine(pkg, model, grid, nlat, ncol, cells)
    first = first_step(st)
    with ref:
        _, host = by_hand(pkg, ref, st, model, first, nsteps, every, K, names, forcing_of(first, nsteps))
    assert np.isfinite(host).all()
    together = series(names)
    assert together.shape == host.shape == (3, nsteps // every, ncol)
    for v, n in enumerate(names):
        alone = series((n,))
        assert same_bits(alone[0], host[v]), (nlat, n, "one field")
        assert same_bits(together[v], host[v]), (nlat, n, "three fields")
        assert same_bits(alone[0], together[v]), (nlat, n)


# ---- options and per-column settings -------------------------------------------------------------------------------------

def install_members(pkg, model, ncol_total):
    """setup(eng, cols): parameter rows, schedules and noise of the members `cols` of an ensemble of ncol_total."""
    base = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    rng = np.random.default_rng(11)
    rows = np.tile(base, (ncol_total, 1))
    iD = pkg.engine.PARAM_ORDER.index("D")
    iA = pkg.engine.PARAM_ORDER.index("A")
    rows[:, iD] *= rng.uniform(0.9, 1.1, ncol_total)
    rows[:, iA] *= rng.uniform(0.98, 1.02, ncol_total)
    rows[1] = rows[0]
    ramps = [pkg.Forcing(0.0, float(c + 1), 0.0, (0, 0), (float(c + 1), -float(c + 1))) for c in range(ncol_total)]
    fcol = np.linspace(-1.5, 1.5, ncol_total)

    def setup(eng, cols):
        eng.set_column_forcing(fcol[cols])
        eng.set_column_params(rows[cols])
        eng.set_column_schedules(ramps[cols])
        eng.set_column_noise(np.linspace(0.5, 2.0, ncol_total)[cols], rho=np.full(ncol_total, 0.9)[cols], seed=2024,
                             streams=(100 + np.arange(ncol_total, dtype=np.uint64))[cols])
    return setup


# option keywords, every, steps per launch, nsteps, launches per sample and chain
VARIANTS = {
    "noise_cap": (dict(), 100, 128, 200, 2),
    "chains": (dict(launch_chains=2, use_graph=False), 7, 16, 70, 1),
    "graph": (dict(use_graph=True), 200, 1, 400, 200),
}


@pytest.mark.parametrize("nlat, ncol", [(180, 8), (1025, 4)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_options_and_columns_alone(pkg, nlat, ncol, variant):
    opt, every, K, nsteps, per_sample = VARIANTS[variant]
    model, grid, names = "MIZ", "sin", ("T", "phi", "Ti")
    setup = install_members(pkg, model, ncol)
    eng, st = make_engine(pkg, model, grid, nlat, ncol, 4, setup, **opt)
    first = first_step(st)
    f = forcing_of(first, nsteps)
    with eng:
        series = eng.run_series(first, nsteps, every, names, f, K)
        after = snapshot(eng, model)
    chains = 2 if variant == "chains" else 1
    assert after["counters"]["steps"] == nsteps
    assert after["counters"]["launches"] == (nsteps // every) * per_sample * chains
    # the loop by hand with the same settings
    ref, _ = make_engine(pkg, model, grid, nlat, ncol, 4, setup, **opt)
    with ref:
        dev, host = by_hand(pkg, ref, st, model, first, nsteps, every, K, names, f)
        ref_after = snapshot(ref, model)
    assert same_bits(series, dev) and same_bits(series, host)
    assert_same_snapshot(after, ref_after, variant)
    if variant == "noise_cap":          # the noise caps a launch at 64 steps; fewer steps per launch change no bit
        other, _ = make_engine(pkg, model, grid, nlat, ncol, 4, setup, **opt)
        with other:
            s16 = other.run_series(first, nsteps, every, names, f, 16)
            c16 = other.counters()
        assert same_bits(s16, series)
        assert c16["launches"] == (nsteps // every) * -(-every // 16)
    # every member alone: its row, forcing, schedule and stream id in a one-column handle
    state = midyear_state(model, st, ncol)
    for c in range(ncol):
        one, _ = make_engine(pkg, model, grid, nlat, 1, 4, None, **opt)
        with one:
            setup(one, slice(c, c + 1))
            one.set_state({k: v[c:c + 1] for k, v in state.items()})
            alone = one.run_series(first, nsteps, every, names, f, K)
            fields = {k: one.get_field(k) for k in PROG + ("T",)}
            noise = one.noise_state()
        assert same_bits(alone[:, :, 0], series[:, :, c]), (variant, c)
        assert same_bits(noise[0], after["noise"][c])
        for k, v in fields.items():
            assert same_bits(v[0], after["fields"][k][c]), (variant, c, k)


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    model = "MIZ"
    eng, st = make_engine(pkg, model, "sin", 180, 3)
    lib, F, dptr = eng.lib, pkg.engine.FIELD, pkg.engine.dptr
    first = first_step(st)
    out = np.full((12, 8, 3), 7.0)

    def call(nsteps=8, every=2, K=4, names=("T", "phi"), series=out, fields=True, h=None):
        ids = (ctypes.c_int * max(1, len(names)))(*[n if isinstance(n, int) else F[n] for n in names])
        return lib.ebm_run_series(eng._h if h is None else h, first, nsteps, None, every, K, len(names),
                                  ids if fields else None, dptr(series))
    with eng:
        eng.run(first, 4, None, True, 2)
        before = snapshot(eng, model)
        bad = [dict(every=0), dict(every=-1), dict(nsteps=7, every=2), dict(names=()), dict(names=MIZ_VARS + ("Ei", "Ew", "h")),
               dict(names=("Tg",)), dict(names=("T0",)), dict(names=(99,)), dict(names=(-1,)), dict(names=("T", "phi", "T")),
               dict(series=None), dict(fields=False)]
        for kw in bad:
            assert call(**kw) == -1, kw
            assert b"ebm_run_series" in lib.ebm_last_error()
            assert_same_snapshot(snapshot(eng, model), before, kw)
        assert np.all(out == 7.0)
        assert call() == 0                                   # and the call itself is fine
        assert eng.counters()["steps"] == before["counters"]["steps"] + 8
    # a handle without a time table
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    with pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, 3, device=0) as bare:
        ids = (ctypes.c_int * 1)(F["phi"])
        assert lib.ebm_run_series(bare._h, 0, 8, None, 2, 4, 1, ids, dptr(out)) == -1
        assert b"ebm_set_time_table" in lib.ebm_last_error()
        assert bare.counters()["steps"] == 0 and bare.field_step("phi")["state_step"] == -1


# ---- Python surfaces -----------------------------------------------------------------------------------------------------

def test_ensemble_series_is_independent_of_sharding(pkg):
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    par = pkg.default_parameters("MIZ")
    members, nsteps, every = 6, 60, 20
    init = {k: v for k, v in midyear_state("MIZ", st, members).items() if k != "T0"}
    fcol = np.linspace(-2.0, 2.0, members)
    noise = dict(sigma=1.5, tau=0.01, seed=5)
    forcing = pkg.Forcing(0.75)

    def shard(cols):
        run = pkg.EnsembleRun("MIZ", st, par, {k: v[cols] for k, v in init.items()}, fcol=fcol[cols], noise=noise,
                              noise_streams=np.arange(members)[cols])
        run.run(10, forcing)
        a = run.series(nsteps, every, forcing=forcing)
        b = run.series(nsteps, every, names=("Ei",), forcing=forcing, steps_per_launch=1)
        steps = run.step_index
        hm = run.engine.hemispheric_mean("Ei")
        run.close()
        return a, b, steps, hm
    a, b, steps, hm = shard(slice(0, members))
    assert a.shape == (2, 3, members) and b.shape == (1, 3, members) and steps == 10 + 2 * nsteps
    assert same_bits(b[0, -1], hm)
    a0, b0, s0, _ = shard(slice(0, 3))
    a1, b1, s1, _ = shard(slice(3, members))
    assert s0 == s1 == steps
    assert same_bits(np.concatenate([a0, a1], axis=2), a) and same_bits(np.concatenate([b0, b1], axis=2), b)
    assert len(np.unique(a[0, -1])) == members
