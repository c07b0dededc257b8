"""GPU tests (-m gpu) of the plans that need more dynamic LDS than the 64 KiB default (csrc/ebm_plan.h: plan_step,
needs_raised_lds; prepare_kernels, csrc/ebm_launch.hip): every such plan launches, at the smallest geometry that needs it, and
gives the bits of plain single steps.  A kernel whose limit ebm_create did not raise fails its first launch
(hipErrorInvalidValue), so a plan missing from the walk of prepare_kernels is an error here, on these shapes only:

* 1732 latitudes (448 threads x 4 cells): the one-step kernels take 63 KiB, only the resident fused-K kernels (70 KiB) cross
  the limit — with and without savesol!'s sums, the reference's step (resident on request: fused_state_in_lds) and the extension;
* 1796 latitudes (512 threads x 4 cells): the one-step kernels cross it (72 KiB) — state only, with diagnostics, deriving phi,
  eliding zero lines, both models;
* 1026 latitudes at two cells per thread (768 threads): its one-step kernels (72 KiB); its fused kernel stays below.

3 columns, 12 steps, both grids.  Every case is compared bitwise, over all eleven fields, with the same handle stepped one
ebm_step at a time with diagnostics — and ebm_integrate's annual mean with the sequential sum of those steps' fields / nt.
From the zero state the first steps take ice from the pole down to a column's own edge (its forcing offset), the later ones
warm the water south of it: with the C oracle, every shape, grid and model here ends finite, the first column covered, the
other two with an edge, water above freezing in a third to a half of the cells."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROG = ("Ei", "Ew", "h", "D", "phi")
ALL = PROG + ("T0", "Tw", "Ti", "n", "E", "T")
MIZ_VARS = ("E", "T", "h", "Ei", "Ew", "Ti", "Tw", "D", "phi", "n")
NCOL, NSTEPS, K = 3, 12, 4
NT = 1000000                                      # steps per year: the explicit step is stable for nt >= nlat^2 / 4
FORCING = np.array([30.0, -150.0, -150.0, 100.0, 150.0, -100.0, 50.0, 100.0, -50.0, 100.0, 50.0, 80.0])      # W m^-2 per step
OFFSETS = np.linspace(-40.0, 40.0, NCOL)
GRIDS = ["sin", "identity"]
MODELS = ["MIZ", "MIZ_IMEX"]


def open_engine(pkg, model, grid, nlat, cells=4, **opt):
    st = pkg.SpaceTime(grid, nlat, 2000, 1)
    par = pkg.default_parameters("MIZ")
    opt.setdefault("use_graph", False)
    eng = pkg.Engine(model, st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), 1.0 / NT, NCOL, device=0,
                     cells_per_thread=cells, **opt)
    eng.set_column_forcing(OFFSETS)
    eng.set_time_table(np.array([(2 * i + 1) / (2.0 * NT) for i in range(NSTEPS)]))     # 12 entries: step 12's successor is step 1
    return eng


@functools.lru_cache(maxsize=None)
def single_steps(pkg, model, grid, nlat, cells=4):
    """The reference: NSTEPS calls of ebm_step with diagnostics; every field after every step [NSTEPS] of dicts."""
    out = []
    with open_engine(pkg, model, grid, nlat, cells) as eng:
        for s in range(NSTEPS):
            eng.step(eng.ttab[s], eng.ttab[(s + 1) % NSTEPS], FORCING[s], True)
            out.append(eng.get_state(ALL))
    last = out[-1]
    assert all(np.isfinite(last[k]).all() for k in PROG), "the scenario left the prognostic state not finite"
    assert (last["phi"] > 0).any() and (last["phi"] == 0).any() and (last["Ew"] != 0).any(), "no ice edge at the end"
    return out


def same_as_single_steps(eng, ref, what):
    got = eng.get_state(ALL)
    for k in ALL:
        assert got[k].shape == ref[-1][k].shape and np.array_equal(got[k], ref[-1][k], equal_nan=True), (what, k)


def geometry(eng, threads, cells, one_step_lds):
    info = eng.launch_info()
    assert (info["threads"], info["cells_per_thread"], info["lds_bytes"]) == (threads, cells, one_step_lds), info


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("model", MODELS)
def test_resident_kernels_at_448_threads(pkg, model, grid):
    """Only the resident kernels (20 x 8 x 448 = 71 680 B) are above 64 KiB; the one-step kernels (64 512 B) are not."""
    ref = single_steps(pkg, model, grid, 1732)
    with open_engine(pkg, model, grid, 1732, fused_state_in_lds=True) as eng:
        geometry(eng, 448, 4, 64512)
        eng.run(0, NSTEPS, FORCING, True, steps_per_launch=K)
        assert eng.counters()["launches"] == NSTEPS // K
        same_as_single_steps(eng, ref, "run, 4 steps per launch, state in LDS")
    with open_engine(pkg, model, grid, 1732, integrate_steps_per_launch=K) as eng:
        out = eng.integrate(NSTEPS, 1, FORCING, True, 3, 7, MIZ_VARS, want_raw=False, want_seasonal=False)
        assert eng.counters()["launches"] == -(-(NSTEPS - 1) // K) + 1        # the year's last step is launched on its own
        same_as_single_steps(eng, ref, "integrate, 4 steps per launch")
        for v, name in enumerate(MIZ_VARS):
            acc = np.zeros((NCOL, 1732))
            with np.errstate(invalid="ignore"):
                for fields in ref:
                    acc = acc + fields[name]
                mean = acc / float(NSTEPS)
            assert np.array_equal(out["avg"][v, 0], mean, equal_nan=True), ("annual mean", name)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("model", MODELS)
def test_one_step_kernels_at_512_threads(pkg, model, grid):
    """18 x 8 x 512 = 73 728 B: the state-only step, the step with diagnostics, and (the reference's step) the one that derives
    phi, without and with zero-line elision."""
    ref = single_steps(pkg, model, grid, 1796)
    with open_engine(pkg, model, grid, 1796) as eng:
        geometry(eng, 512, 4, 73728)
        for s in range(NSTEPS):
            eng.step(eng.ttab[s], eng.ttab[(s + 1) % NSTEPS], FORCING[s], s == NSTEPS - 1)
        same_as_single_steps(eng, ref, "step without diagnostics, the last with")
    for elide in (True, False):
        with open_engine(pkg, model, grid, 1796, elide_zero_lines=elide) as eng:
            eng.run(0, NSTEPS, FORCING, True)
            assert eng.counters()["launches"] == NSTEPS
            same_as_single_steps(eng, ref, f"run, elide_zero_lines = {elide}")


@pytest.mark.parametrize("grid", GRIDS)
def test_two_cells_at_768_threads(pkg, grid):
    """12 x 8 x 768 = 73 728 B for the one-step kernels; the fused register kernel takes 6 x 8 x 768 B."""
    ref = single_steps(pkg, "MIZ", grid, 1026, 2)
    with open_engine(pkg, "MIZ", grid, 1026, 2) as eng:
        geometry(eng, 768, 2, 73728)
        eng.run(0, NSTEPS, FORCING, True)
        same_as_single_steps(eng, ref, "run")
    with open_engine(pkg, "MIZ", grid, 1026, 2) as eng:
        eng.run(0, NSTEPS, FORCING, True, steps_per_launch=K)
        assert eng.counters()["launches"] == NSTEPS // K
        same_as_single_steps(eng, ref, "run, 4 steps per launch")
