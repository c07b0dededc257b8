"""GPU tests (-m gpu) of the forcing noise in workgroups of more than one wave, in the 768-thread kernel of two cells per
thread and in the LDS-resident kernels (csrc/ebm_noise.h, ebm_miz_fused.h, ebm_miz_resident.h, launch_miz_step).

tests/test_gpu_noise.py steps 180 cells: one wave of 64 threads at four cells per thread and two waves at two, where "every
wave evaluates the same sequence" and "thread 0 stores N_c after the last barrier" hold trivially or between two waves only,
and "the kernel reads its row of nseq because of its size" is never reached.  Here one smallest shape per kernel family,
each pinning launch_info's threads and cells per thread:

    MIZ       4 cells/thread   258 x 3   128 threads   two waves, padding in the last thread; N_c sequence in registers
    MIZ       4               1025 x 2   320           five waves, a lone cell in a pair; registers
    MIZ       4               2050 x 2   576           the smallest LDS-resident-by-size kernel; N_c sequence in memory
    MIZ       4               4096 x 2  1024           the headline kernels; memory
    MIZ       2                258 x 3   192           three waves; registers
    MIZ       2               1025 x 2   768           miz_fused_kernel<2, ..., 768>: memory inside the register kernel
    MIZ_IMEX  4                258 x 3,  1025 x 2      128, 320: resident kernel; memory
    Classic   4 and 2          258 x 3,  1025 x 2      128, 320 and 192, 768: fused classic kernel; memory

The reference is the one of tests/test_gpu_noise.py, unchanged: the device's innovations (eng.noise_innovations), N_c(n) from
them on the host by the exact recurrence (noise.ar1), and a NOISE-FREE handle of the same geometry stepped one step at a
time with set_column_forcing(N[:, i]).  Every comparison is bitwise (np.array_equal, NaN == NaN); no tolerance anywhere.
Per shape the reference is computed once and shared, and shown to be finite and to differ from the run without noise.

Grid, dt and time table as tests/test_gpu_phi_derived.py: the explicit step wants nt >= nlat^2 / 4 steps a year, a table of
256 mid-year entries stands in for a SpaceTime of millions of steps, and the golden mid-year state is spread by nearest
cell.  The classic model (implicit step) keeps the fixture's 2000 steps a year from its step 522.
"""
import functools

import numpy as np
import pytest

from conftest import load_golden
from support import (MIZ_PROG as PROG, all_fields as names, assert_same_values as assert_same, host_N, is_miz, noise_args,
                     noise_module as _noise, prognostic)

pytestmark = pytest.mark.gpu

MIZ_ALL = names("MIZ")

# steps per year of the MIZ shapes (>= nlat^2 / 4); the classic model: 2000.  Its own table: 2050 cells, and 4096 stepped explicitly
NT = {180: 2000, 258: 20000, 1025: 270000, 2050: 1100000, 4096: 4200000}
TABLE = 256
FIRST = 40 * TABLE               # global index of the first step: entry 0 of the table, a step clock that is not 0
NSTEPS = 130                     # 64 + 64 + 2: two full fused launches and a ragged one
CLASSIC_FIRST_ENTRY = 522        # the classic fixture's state is that of its step 522


class Shape:
    def __init__(self, model, cells, nlat, ncol, threads):
        self.model, self.cells, self.nlat, self.ncol, self.threads = model, cells, nlat, ncol, threads

    def __repr__(self):
        return f"{self.model}-{self.cells}cells-{self.nlat}x{self.ncol}"

    def __hash__(self):
        return hash(repr(self))

    def __eq__(self, other):
        return repr(self) == repr(other)


SHAPES = [
    Shape("MIZ", 4, 258, 3, 128), Shape("MIZ", 4, 1025, 2, 320), Shape("MIZ", 4, 2050, 2, 576), Shape("MIZ", 4, 4096, 2, 1024),
    Shape("MIZ", 2, 258, 3, 192), Shape("MIZ", 2, 1025, 2, 768),
    Shape("MIZ_IMEX", 4, 258, 3, 128), Shape("MIZ_IMEX", 4, 1025, 2, 320),
    Shape("Classic", 4, 258, 3, 128), Shape("Classic", 4, 1025, 2, 320),
    Shape("Classic", 2, 258, 3, 192), Shape("Classic", 2, 1025, 2, 768),
]
REGISTERS = Shape("MIZ", 4, 258, 3, 128)       # N_c sequence in registers, two waves
MEMORY = Shape("MIZ", 2, 1025, 2, 768)         # N_c sequence in memory, inside the register kernel


def forcing(n):
    return 0.5 * np.sin(0.37 * np.arange(n))


@functools.lru_cache(maxsize=None)
def space(pkg, model, nlat):
    """x, grid kind, dt and the TABLE-entry time table (entry i: step i of the test, mid-year on)"""
    if is_miz(model):
        st, nt, entry0 = pkg.SpaceTime("sin", nlat, 2000, 1), NT[nlat], NT[nlat] // 2
    else:
        st, nt, entry0 = pkg.SpaceTime("identity", nlat, 2000, 1), 2000, CLASSIC_FIRST_ENTRY
    t = np.array([(2 * i + 1) / (2.0 * nt) for i in range(entry0, entry0 + TABLE)])
    return st.x, st.grid_kind, 1.0 / nt, t


@functools.lru_cache(maxsize=None)
def start_state(pkg, model, nlat):
    x = space(pkg, model, nlat)[0]
    if is_miz(model):
        g, keys, step = load_golden("miz_sin_180_2000.npz"), PROG + ("T0",), 1000
    else:
        g, keys, step = load_golden("classic_identity_180_2000.npz"), ("E", "Tg"), 522
    nearest = np.abs(x[:, None] - g["x"][None, :]).argmin(axis=1)
    return {k: np.ascontiguousarray(g[f"s{step}_{k}"][nearest]) for k in keys}


def open_engine(pkg, shape, table=None, clock=FIRST, **opt):
    """A handle of the shape at the start state, without noise; the launch geometry is the one the shape states."""
    x, grid_kind, dt, t = space(pkg, shape.model, shape.nlat)
    par = pkg.default_parameters("Classic" if shape.model == "Classic" else "MIZ")
    eng = pkg.Engine(shape.model, grid_kind, x, pkg.engine.param_vector(par, pkg.default_parval), dt, shape.ncol, device=0,
                     cells_per_thread=shape.cells, **opt)
    info = eng.launch_info()
    assert (info["threads"], info["cells_per_thread"]) == (shape.threads, shape.cells), (shape, info)
    eng.set_state({k: np.tile(v, (shape.ncol, 1)) for k, v in start_state(pkg, shape.model, shape.nlat).items()})
    eng.set_time_table(t if table is None else table)
    eng.set_step_clock(clock)
    return eng


def single_steps(pkg, shape, first, N, f, table=None):
    """The reference: a noise-free handle, one launch per step, N[:, i] as the column forcing of step first + i.  Returns the
    state after the last step (every field; the last step writes the diagnostic ones)."""
    n = N.shape[1]
    with open_engine(pkg, shape, table, first, use_graph=False) as ref:
        for i in range(n):
            ref.set_column_forcing(N[:, i])
            ref.run(first + i, 1, f[i:i + 1], diag_last=(i == n - 1))
        return ref.get_state(names(shape.model))


@functools.lru_cache(maxsize=None)
def reference(pkg, shape):
    """(N [ncol, NSTEPS], the reference state after NSTEPS steps, the state after NSTEPS steps without noise)"""
    args, f = noise_args(shape.ncol), forcing(NSTEPS)
    with open_engine(pkg, shape) as eng:
        eng.set_column_noise(**args)
        N = host_N(pkg, eng, args, FIRST, NSTEPS)
    want = single_steps(pkg, shape, FIRST, N, f)
    with open_engine(pkg, shape) as eng:
        eng.set_column_noise(0.0, rho=args["rho"], seed=args["seed"])
        eng.run(FIRST, NSTEPS, f, diag_last=True, steps_per_launch=64)
        quiet = eng.get_state(names(shape.model))
    for v in (N, *want.values(), *quiet.values()):
        v.setflags(write=False)
    return N, want, quiet


# ---- the comparisons are not empty -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=repr)
def test_the_reference_is_finite_and_feels_the_noise(pkg, shape):
    """(noise_args' sigma, up to 3 W m^-2, keeps every shape finite: no shape needed a smaller one)"""
    N, want, quiet = reference(pkg, shape)
    assert np.isfinite(N).all() and (N[:, -1] != 0.0).all()
    for k in prognostic(shape.model):
        assert np.isfinite(want[k]).all(), k
        assert np.isfinite(quiet[k]).all(), k
    # every column: the least noisy one (sigma = 0.5) too
    for c in range(shape.ncol):
        assert any(not np.array_equal(want[k][c], quiet[k][c]) for k in prognostic(shape.model)), c


# ---- 1. stepping paths ---------------------------------------------------------------------------------------------------

PATHS = ("run", "graph", "fused", "fused_lds", "chains2")


def applies(shape, path):
    if path == "fused_lds":         # the option chooses between two kernels only here
        return shape.model == "MIZ" and shape.cells == 4 and shape.threads <= 512
    if path == "chains2":           # an odd column count: chains of 1 and 2 columns
        return shape.ncol == 3
    return True


@pytest.mark.parametrize("shape,path", [(s, p) for s in SHAPES for p in PATHS if applies(s, p)], ids=lambda v: str(v))
def test_noisy_stepping_equals_single_steps_with_the_noise_as_column_forcing(pkg, shape, path):
    N, want, _ = reference(pkg, shape)
    opt = {"run": dict(use_graph=False), "graph": dict(use_graph=True), "fused": dict(use_graph=False),
           "fused_lds": dict(use_graph=False, fused_state_in_lds=True),
           "chains2": dict(use_graph=False, launch_chains=2)}[path]       # (graph replay has one chain)
    if path == "fused" and shape.model == "MIZ":
        opt["fused_state_in_lds"] = False
    spl = 1 if path in ("run", "graph") else 64
    with open_engine(pkg, shape, **opt) as eng:
        eng.set_column_noise(**noise_args(shape.ncol))
        before = eng.counters()["launches"]
        eng.run(FIRST, NSTEPS, forcing(NSTEPS), diag_last=True, steps_per_launch=spl)
        launches = eng.counters()["launches"] - before
        got = eng.get_state(names(shape.model))
        assert np.array_equal(eng.noise_state(), N[:, -1]), (shape, path)
    # launches of 64, 64 and 2 steps, per chain; one per step otherwise
    assert launches == {"run": NSTEPS, "graph": NSTEPS, "chains2": 6}.get(path, 3), (shape, path)
    assert_same(got, want, (shape, path))


# ---- 2. fused launch lengths ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spl,launches", [(2, 65), (63, 3), (64, 3), (100, 3)])
@pytest.mark.parametrize("shape", [REGISTERS, MEMORY], ids=repr)
def test_fused_launch_lengths(pkg, shape, spl, launches):
    """2, 63 and 64 steps to a launch, and a request of 100 that the runtime caps to kNoiseMaxFused = 64 (three launches,
    not two)."""
    N, want, _ = reference(pkg, shape)
    with open_engine(pkg, shape, use_graph=False) as eng:
        eng.set_column_noise(**noise_args(shape.ncol))
        before = eng.counters()["launches"]
        eng.run(FIRST, NSTEPS, forcing(NSTEPS), diag_last=True, steps_per_launch=spl)
        assert eng.counters()["launches"] - before == launches
        got = eng.get_state(names(shape.model))
        assert np.array_equal(eng.noise_state(), N[:, -1])
    assert_same(got, want, (shape, spl))


# ---- 3. chunked calls ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [REGISTERS, MEMORY], ids=repr)
def test_chunked_fused_calls_hand_the_noise_state_on(pkg, shape):
    """1 + 64 + 65 steps in three fused calls: N_c written back by one launch and read by the next, several waves."""
    N, want, _ = reference(pkg, shape)
    f = forcing(NSTEPS)
    with open_engine(pkg, shape, use_graph=False) as eng:
        eng.set_column_noise(**noise_args(shape.ncol))
        done = 0
        for n in (1, 64, 65):
            eng.run(FIRST + done, n, f[done:done + n], diag_last=(done + n == NSTEPS), steps_per_launch=64)
            done += n
            assert np.array_equal(eng.noise_state(), N[:, done - 1]), (shape, done)
        got = eng.get_state(names(shape.model))
    assert_same(got, want, shape)


# ---- 4. the step counter's carry into its second 32-bit word ---------------------------------------------------------------

CARRY_FIRST, CARRY_STEPS = 2 ** 32 - 3, 8
CARRY_SHAPES = [Shape("MIZ", 4, 180, 2, 64), REGISTERS]


def carry_table(pkg, shape):
    """The time table laid out so that step CARRY_FIRST + i (entry (CARRY_FIRST + i) % TABLE = 253, 254, 255, 0, ...) finds
    the i-th mid-year entry."""
    return np.roll(space(pkg, shape.model, shape.nlat)[3], CARRY_FIRST % TABLE)


@functools.lru_cache(maxsize=None)
def carry_reference(pkg, shape):
    args, f = noise_args(shape.ncol), forcing(CARRY_STEPS)
    with open_engine(pkg, shape, carry_table(pkg, shape), CARRY_FIRST) as eng:
        eng.set_column_noise(**args)
        xi = eng.noise_innovations(CARRY_FIRST, CARRY_STEPS)
        low_words_only = eng.noise_innovations(0, CARRY_STEPS - 3)
    N = _noise(pkg).ar1(xi, args["sigma"], args["rho"])
    want = single_steps(pkg, shape, CARRY_FIRST, N, f, carry_table(pkg, shape))
    return xi, low_words_only, N, want


@pytest.mark.parametrize("shape", CARRY_SHAPES, ids=repr)
def test_the_carry_reference_sees_the_second_counter_word(pkg, shape):
    """Steps 2^32 .. 2^32 + 4 and steps 0 .. 4 share their low counter word: the innovations the reference is made from
    differ, and its state is finite."""
    xi, low_words_only, N, want = carry_reference(pkg, shape)
    assert not np.any(xi[:, 3:] == low_words_only)
    assert all(np.isfinite(want[k]).all() for k in PROG)


@pytest.mark.parametrize("how", ["steps", "one_launch", "three_and_five"])
@pytest.mark.parametrize("shape", CARRY_SHAPES, ids=repr)
def test_stepping_across_step_2_to_the_32(pkg, shape, how):
    """8 steps from step 2^32 - 3: one launch per step, one launch of 8 (the carry inside the launch's lanes), and calls of 3
    and 5 (the second starts at 2^32)."""
    xi, _, N, want = carry_reference(pkg, shape)
    f = forcing(CARRY_STEPS)
    with open_engine(pkg, shape, carry_table(pkg, shape), CARRY_FIRST, use_graph=False) as eng:
        eng.set_column_noise(**noise_args(shape.ncol))
        if how == "steps":
            eng.run(CARRY_FIRST, CARRY_STEPS, f, diag_last=True, steps_per_launch=1)
        elif how == "one_launch":
            eng.run(CARRY_FIRST, CARRY_STEPS, f, diag_last=True, steps_per_launch=8)
        else:
            eng.run(CARRY_FIRST, 3, f[:3], diag_last=False, steps_per_launch=64)
            assert np.array_equal(eng.noise_state(), N[:, 2])
            eng.run(CARRY_FIRST + 3, 5, f[3:], diag_last=True, steps_per_launch=64)
        got = eng.get_state(MIZ_ALL)
        assert np.array_equal(eng.noise_state(), N[:, -1]), (shape, how)
    assert_same(got, want, (shape, how))


# ---- 5. ebm_integrate ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cells,threads", [(4, 128), (2, 192)])
def test_integrate_with_noise_beyond_one_wave(pkg, cells, threads):
    """One year of 20000 steps (>= 258^2 / 4) on 258 x 2, lastonly.  Four cells per thread: the fused stretches run
    miz_resident_kernel<SAVE> (N_c sequence in memory); two: miz_fused_kernel<2, ..., SAVE> (registers).  64 steps to a
    launch and one give the same winter, summer, annual mean and final state; the final state is that of 20000 single
    noise-free steps with N as the column forcing.  Measured on an MI355X: 1.4 s (four cells per thread) and 1.3 s (two)
    for the whole case — the two integrations and the 20000 single launches of the reference — so the year stays whole."""
    nlat, ncol, nt = 258, 2, NT[258]
    st = pkg.SpaceTime("sin", nlat, nt, 1)
    args = noise_args(ncol)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    state = {k: np.tile(v, (ncol, 1)) for k, v in start_state(pkg, "MIZ", nlat).items()}

    def engine(**opt):
        eng = pkg.Engine("MIZ", st.grid_kind, st.x, vec, st.dt, ncol, device=0, cells_per_thread=cells, **opt)
        info = eng.launch_info()
        assert (info["threads"], info["cells_per_thread"]) == (threads, cells)
        eng.set_state(state)
        eng.set_time_table(st.t)
        eng.set_step_clock(0)
        return eng

    out = {}
    for spl in (64, 1):
        with engine(integrate_steps_per_launch=spl) as eng:
            eng.set_column_noise(**args)
            before = eng.counters()["launches"]
            out[spl] = eng.integrate(nt, 1, None, True, st.winter.inx, st.summer.inx, ("T", "Ei"), want_raw=False)
            out[spl]["launches"] = eng.counters()["launches"] - before
            out[spl]["state"] = eng.get_state(MIZ_ALL)
            out[spl]["N"] = eng.noise_state()
            if spl == 64:
                N = host_N(pkg, eng, args, 0, nt)
    assert out[1]["launches"] == nt and out[64]["launches"] < nt // 32       # (the stretches were fused)
    for k in ("winter", "summer", "avg"):
        assert np.array_equal(out[64][k], out[1][k], equal_nan=True), k
        assert np.isfinite(out[64][k][1]).all(), k                          # Ei
    assert_same(out[64]["state"], out[1]["state"], "64 steps to a launch and one")
    with engine(use_graph=False) as ref:
        for i in range(nt):
            ref.set_column_forcing(N[:, i])
            ref.run(i, 1, None, diag_last=(i == nt - 1))
        want = ref.get_state(MIZ_ALL)
    assert all(np.isfinite(want[k]).all() for k in PROG)
    assert np.array_equal(out[64]["N"], N[:, -1]) and np.array_equal(out[1]["N"], N[:, -1])
    assert_same(out[64]["state"], want, "integrate and single steps")
