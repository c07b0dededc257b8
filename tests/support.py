"""The scaffolding the test files share: names of the fields, bit-pattern comparison, the grid and time table of a meridian
length, the mid-year start state, handles prepared at it, the per-step forcing, snapshots of a handle, and the stand-ins
and program builds of the host tests.  One definition of each.

A plain module, imported like conftest (`from support import ...`; the tests directory is on the path): no fixtures, no
hooks, no pytest settings.  A NEW GPU TEST FILE STARTS FROM HERE — it takes its start state, handles and comparisons from
this module and defines only what is its own: its cases, its reference and its claims.  No test module imports scaffolding
from another test module; what stays importable from a test file is what that file tests or states as a reference
(first_crossing of test_host_until.py, the criterion restatement of test_gpu_equilibrate.py, the crafted data of
test_gpu_ensemble_sums.py, ...).

An edit here changes the inputs of every file that imports the edited name: tests/tools/README.md says how that is checked.
"""
import functools
import os
import subprocess
from importlib import import_module

import numpy as np

from conftest import ROOT, load_golden

# ---- names and predicates ----------------------------------------------------------------------------------------------------

MIZ_PROG = ("Ei", "Ew", "h", "D", "phi")
MIZ_DIAG = ("Tw", "Ti", "n", "E", "T")
CLASSIC_VARS = ("E", "Tg", "T", "h")


def is_miz(model):
    return model.startswith("MIZ")


def prognostic(model):
    return MIZ_PROG if is_miz(model) else ("E", "Tg")


def all_fields(model):
    return MIZ_PROG + ("T0",) + MIZ_DIAG if is_miz(model) else CLASSIC_VARS


def is_diagnostic(model, name):
    return name in (MIZ_DIAG if is_miz(model) else ("T", "h"))


# ---- bit patterns ------------------------------------------------------------------------------------------------------------

def bits(a):
    """The doubles as uint64 (int64 would give the same equality): NaN payloads and signs of zero count."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def assert_same_bits(a, b, what=""):
    """Arrays, or dicts of arrays: the same keys, equal shapes, equal bit for bit."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            assert_same_bits(a[k], b[k], (what, k))
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), what


# ---- grid and time -----------------------------------------------------------------------------------------------------------

# steps per year: the explicit model is stable for nt >= nlat^2 / 4; 4096 is stepped by the implicit extension only
_STEPS_PER_YEAR = {2: 2000, 3: 2000, 65: 2000, 180: 2000, 257: 20000, 258: 20000, 513: 70000, 1025: 270000, 4096: 2000}


def steps_per_year(nlat):
    return _STEPS_PER_YEAR[nlat]


@functools.lru_cache(maxsize=None)
def space_time(pkg, grid, nlat):
    """(SpaceTime(grid, nlat, steps_per_year(nlat), 1), its cos(2 pi t) table)"""
    st = pkg.SpaceTime(grid, nlat, steps_per_year(nlat), 1)
    tab = np.array([pkg.cos2pit(float(t)) for t in st.t], dtype=np.float64)
    return st, tab


def forcing_of(first, nsteps):
    return 0.5 * np.sin(0.37 * (first + np.arange(nsteps)))


# ---- the start state ---------------------------------------------------------------------------------------------------------

def midyear_state(model, st, ncol):
    """The golden fixtures' mid-year state (ice, open water, a live T0 solve) resampled onto st.x (st: anything with x and
    grid_kind): every cell takes the WHOLE state of the nearest golden cell.  Interpolating each field linearly on its own,
    as tests/test_gpu_column_params.py does, mixes neighbouring cells' ice thickness, floe size and concentration into cells
    no model state has (ice concentration without thickness), and on every grid but the golden one the T0 solve of the
    second step returns NaN everywhere (seen with the CPU oracle as well): bits would still compare equal, but of nothing.
    Every column is the same; they differ through their forcing offsets."""
    if is_miz(model):
        g = load_golden(f"miz_{'identity' if st.grid_kind == 'identity' else 'sin'}_180_2000.npz")
        names, step = MIZ_PROG + ("T0",), "s1000"
    else:
        g = load_golden("classic_identity_180_2000.npz")
        names, step = ("E", "Tg"), "s522"
    nearest = np.abs(st.x[:, None] - g["x"][None, :]).argmin(axis=1)
    return {k: np.tile(g[f"{step}_{k}"][nearest], (ncol, 1)) for k in names}


# ---- handles -----------------------------------------------------------------------------------------------------------------

def member_installer(pkg, ncol_total, what):
    """setup(eng, cols): the per-member settings named in `what` ("params", "sched", "noise") of the members `cols` of an
    ensemble of ncol_total — distinct parameter rows, ramps, noise streams and sigmas."""
    base = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    rng = np.random.default_rng(11)
    rows = np.tile(base, (ncol_total, 1))
    rows[:, pkg.engine.PARAM_ORDER.index("D")] *= rng.uniform(0.9, 1.1, ncol_total)
    rows[:, pkg.engine.PARAM_ORDER.index("A")] *= rng.uniform(0.98, 1.02, ncol_total)
    ramps = [pkg.Forcing(0.0, float(c % 5 + 1), 0.0, (0, 0), (float(c % 5 + 1), -float(c % 5 + 1))) for c in range(ncol_total)]

    def setup(eng, cols):
        if "params" in what:
            eng.set_column_params(rows[cols])
        if "sched" in what:
            eng.set_column_schedules(ramps[cols])
        if "noise" in what:
            eng.set_column_noise(np.linspace(0.5, 2.0, ncol_total)[cols], rho=np.full(ncol_total, 0.9)[cols], seed=2024,
                                 streams=(100 + np.arange(ncol_total, dtype=np.uint64))[cols])
    return setup


def make_engine(pkg, model, grid, nlat, ncol, cells=4, what=(), setup=None, single_offset=None, **opt):
    """(eng, st): a handle at the mid-year state with the time table and the forcing offsets linspace(-1.5, 1.5, ncol) — a
    single column at -1.5, or at single_offset where given — then the member settings of `what` (member_installer), then
    setup(eng, cols) for anything more."""
    st, tab = space_time(pkg, grid, nlat)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ" if is_miz(model) else "Classic"), pkg.default_parval)
    eng = pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, ncol, device=0, cells_per_thread=cells, **opt)
    eng.set_state(midyear_state(model, st, ncol))
    eng.set_column_forcing(np.array([single_offset]) if ncol == 1 and single_offset is not None else np.linspace(-1.5, 1.5, ncol))
    eng.nt, eng.ttab = len(tab), tab
    pkg.engine.check(eng.lib.ebm_set_time_table(eng._h, len(tab), pkg.engine.dptr(tab)), "ebm_set_time_table")
    if what:
        member_installer(pkg, ncol, what)(eng, slice(0, ncol))
    if setup is not None:
        setup(eng, slice(0, ncol))
    return eng, st


def step_by(eng, path, first, n, f):
    """n steps from `first` by one of the stepping entry points, the diagnostics written at the end."""
    if path == "run_1":
        eng.run(first, n, f, True, 1)
    elif path == "fused_7":
        eng.run(first, n, f, True, 7)
    elif path == "series":
        eng.run_series(first, n, n, ("T",), f, 4)        # diag = 1: T is a diagnostic field of both models
    else:                                                 # "until": one round of ebm_run_until that nobody leaves early
        out = eng.run_until(first, 1, n, "T", np.full(eng.ncol, np.inf), np.ones(eng.ncol, dtype=np.int64), f, 4)
        assert not out["crossed"].any()
        eng.run(first + n, 1, None, True, 1)              # ... and a diagnostic step, so that every field can be compared


# ---- snapshots ---------------------------------------------------------------------------------------------------------------

def snapshot(eng, model):
    """What a call's definition says it leaves behind: the fields that may be read, the validity bookkeeping of every
    field (it holds the last step taken: the step clock minus one), the noise state and the counters."""
    out = {"field_step": {k: eng.field_step(k) for k in all_fields(model)}, "noise": eng.noise_state(),
           "counters": eng.counters(), "fields": {}}
    for k in all_fields(model):
        if out["field_step"][k]["current"]:
            out["fields"][k] = eng.get_field(k)
    return out


def assert_same_snapshot(a, b, what):
    assert a["field_step"] == b["field_step"], what
    assert a["counters"] == b["counters"], (what, a["counters"], b["counters"])
    assert same_bits(a["noise"], b["noise"]), what
    assert a["fields"].keys() == b["fields"].keys(), what
    for k in a["fields"]:
        assert same_bits(a["fields"][k], b["fields"][k]), (what, k)


def assert_snapshot_by_column(got, want, what):
    """assert_same_snapshot that names the columns that differ."""
    assert got["field_step"] == want["field_step"], (what, got["field_step"], want["field_step"])
    assert got["counters"] == want["counters"], (what, got["counters"], want["counters"])
    bad = np.flatnonzero(bits(got["noise"]) != bits(want["noise"]))
    assert bad.size == 0, f"{what}: the noise state differs in columns {bad[:10]}"
    assert got["fields"].keys() == want["fields"].keys(), (what, sorted(got["fields"]), sorted(want["fields"]))
    for k in want["fields"]:
        bad = np.flatnonzero((bits(got["fields"][k]) != bits(want["fields"][k])).any(axis=1))
        assert bad.size == 0, f"{what}: field {k} differs in columns {bad[:10]}"


# ---- column maps (parent[c]: the column whose state column c takes) ----------------------------------------------------------

def make_maps(n):
    """name -> parent map of n columns; map_claims asserts in NumPy alone that each is what its name says."""
    c = np.arange(n)
    if n == 1:
        return {"identity": c.copy()}
    swap = c.copy()
    swap[0], swap[1] = 1, 0
    rnd = np.random.default_rng(77 + n).integers(0, n, n)
    if n >= 5:
        rnd[0] = 0                                     # a fixed point
        rnd[1], rnd[2] = 2, 1                          # a 2-cycle
        rnd[3], rnd[4] = 1, 3                          # a chain 1 -> 3 -> 4 hanging off the cycle
        if n >= 65:
            rnd[10:30:3] = np.arange(10, 30, 3)        # more fixed points
            rnd[40], rnd[41], rnd[42] = 41, 42, 40     # a 3-cycle
    else:
        rnd = np.array([0, 2, 1])                      # three columns: a fixed point and a cycle
    return {"identity": c.copy(), "swap": swap, "shift": (c - 1) % n, "chain": np.maximum(c - 1, 0),
            "fanout": np.full(n, n - 1), "random": rnd}


def orbit_returns(p, c):
    """Is column c on a cycle of p (does following the parents from c come back to c)?"""
    x = p[c]
    for _ in range(len(p)):
        if x == c:
            return True
        x = p[x]
    return False


def map_claims(name, p):
    n = len(p)
    c = np.arange(n)
    assert p.shape == (n,) and ((p >= 0) & (p < n)).all()
    if name == "identity":
        assert (p == c).all()
    elif name == "swap":
        assert p[0] == 1 and p[1] == 0 and (p[2:] == c[2:]).all()
    elif name == "shift":
        assert sorted(p.tolist()) == c.tolist() and (p != c).all(), "a permutation without a fixed point"
        x, steps = 0, 0
        while True:
            x, steps = p[x], steps + 1
            if x == 0:
                break
        assert steps == n, "one cycle through every column"
        assert (p[1:] < c[1:]).all() and p[0] > 0, "ascending order overwrites parents 0 .. n-2 before they are read, " \
                                                   "descending order overwrites n-1 before column 0 reads it"
    elif name == "chain":
        assert p[0] == 0 and (p[1:] == c[1:] - 1).all() and not any(orbit_returns(p, k) for k in range(1, n))
    elif name == "fanout":
        assert (p == n - 1).all()
    elif name == "random":
        moved = p != c
        assert (~moved).any(), "a fixed point"
        assert any(moved[k] and orbit_returns(p, k) for k in range(n)), "a cycle of moved columns"
        if n >= 5:
            assert any(moved[k] and moved[p[k]] and not orbit_returns(p, k) for k in range(n)), \
                "a chain: a moved column off every cycle whose parent is itself overwritten"


# ---- the forcing noise -------------------------------------------------------------------------------------------------------

def noise_module(pkg):
    return import_module(pkg.__name__ + ".noise")


def noise_args(ncol):
    return dict(sigma=np.linspace(0.5, 3.0, ncol), rho=np.linspace(0.0, 0.95, ncol), seed=0x5EED_0001_2345_6789)


def host_N(pkg, eng, args, first, nsteps, N0=None):
    """N_c after each of the steps first .. first + nsteps - 1, from the device's innovations (exact recurrence)."""
    return noise_module(pkg).ar1(eng.noise_innovations(first, nsteps), args["sigma"], args["rho"], N0)


def assert_same_values(a, b, what):
    """Dicts of arrays equal as numbers, NaN positions coinciding (the keys of a)."""
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---- the host tests ----------------------------------------------------------------------------------------------------------

class NoDevice:
    """Stands in for the library: any call is a device call the checks should have prevented."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached before the argument checks refused the call")


def bare_engine(pkg, model="MIZ", ncol=3, **attrs):
    """An Engine that was never created on a device: 18 latitudes, NoDevice for a library, and `attrs` set on it."""
    engine = import_module(pkg.__name__ + ".engine")
    eng = engine.Engine.__new__(engine.Engine)
    eng.model, eng.ncol, eng.nlat, eng.lib, eng._h = model, ncol, 18, NoDevice(), None
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


def compile_host_program(main_cpp, out, flags=()):
    """g++ -O2 -std=c++17 of tests/<main_cpp> (plain C++, no HIP) with the caller's flags; returns `out`."""
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, "-o", out, os.path.join(ROOT, "tests", main_cpp)], check=True)
    return out
