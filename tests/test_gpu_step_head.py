"""GPU tests (-m gpu) of the order in which the one-step kernels (csrc/ebm_miz_step.h) request their inputs: the scalar words of
the head in one batch (StepHead, csrc/ebm_device.h), then phase A's state, the mask word and the tables, then the forcing and the
noise record.  None of it may change anything a caller can see.

Reference: the same steps through ebm_run_fused, one step per call with diagnostics — the fused kernels, which share the
physics and keep their own head.  Every comparison is bitwise and sets no tolerance; the solve and cap-hit counters must equal
the reference's.

Shapes, the smallest at which each thing can go wrong: 200 x 3 (one wave, padding), 1026 x 3 (five waves, odd tail), 180 x 300
(more columns than the prefetch distance of 256: the successor's flag words are read, and the last columns have no successor),
1796 x 3 (512 threads, the plan above 64 KiB of LDS).  Both grids.  Each with and without the per-column forcing offsets, with a
per-column Forcing schedule, with forcing noise, with two parameter sets per ensemble; by ebm_step and ebm_run (the step's scalars in the
launch arguments) and by ebm_run replayed as a graph (the scalars in the schedule table); a diagnostic step in the middle; eliding zero
lines and not.

State: the golden mid-year state resampled by nearest-cell copy (support.midyear_state); in every column pair 0 of wave 0's
lanes (cells 4 t, 4 t + 1, t < 64) takes the whole state of an ice cell and pair 1 (cells 4 t + 2, 4 t + 3) that of an open-water
cell, so that one wave holds pairs that are flagged (Ei, h, D of pair 1) and pairs that are not.  At these time steps
(nt >= nlat^2 / 4) six steps move no ice edge.
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, assert_same_bits as same, bits, forcing_of, member_installer, midyear_state

pytestmark = pytest.mark.gpu

ALL = ("Ei", "Ew", "h", "D", "phi", "E", "T", "Ti", "Tw", "n", "T0")
SHAPES = [(200, 3), (1026, 3), (180, 300), (1796, 3)]
THREADS = {200: 64, 1026: 320, 180: 64, 1796: 512}
NT = {200: 20000, 1026: 270000, 180: 20000, 1796: 1000000}       # steps per year, nt >= nlat^2 / 4
GRIDS = ["sin", "identity"]
NSTEPS, MID = 6, 2                                               # a diagnostic step at MID and at the end
NGRAPH = 131          # ebm_run replays its captured graph of 64 launches from 128 steps on: two replays, then single launches
NTABLE = NGRAPH + 1                                              # entries of the time table
# the member settings of a case: "nofcol" leaves the per-column offsets out, the others are support.member_installer's
SETTINGS = [(), ("nofcol",), ("sched",), ("noise",), ("params",)]
SETTING_IDS = ["fcol", "no_fcol", "forcing_schedule", "forcing_noise", "two_parameter_sets"]


class Space:
    def __init__(self, pkg, grid, nlat):
        st = pkg.SpaceTime(grid, nlat, 2000, 1)
        self.x, self.grid_kind, self.dt = st.x, st.grid_kind, 1.0 / NT[nlat]
        self.t = np.array([(2 * i + 1) / (2.0 * NT[nlat]) + 0.5 for i in range(NTABLE)])
        self.ct = np.array([pkg.cos2pit(float(t)) for t in self.t])


@functools.lru_cache(maxsize=None)
def space(pkg, grid, nlat):
    return Space(pkg, grid, nlat)


@functools.lru_cache(maxsize=None)
def start_state(pkg, grid, nlat, ncol):
    st = space(pkg, grid, nlat)
    base = {k: v[0].copy() for k, v in midyear_state("MIZ", st, 1).items()}
    icy = base["h"] > 0
    ice = {k: base[k][int(np.flatnonzero(icy & (base["Ew"] != 0))[0])] for k in base}
    open_water = np.flatnonzero(~icy & (base["Ew"] != 0))
    # (the identity grid's golden state has ice everywhere: the ice taken off)
    water = {k: base[k][int(open_water[0])] for k in base} if open_water.size else dict(ice, Ei=0.0, h=0.0, D=0.0, phi=0.0)
    k = np.arange(nlat)
    for f in base:
        base[f][(k < 256) & ((k % 4) // 2 == 0)] = ice[f]
        base[f][(k < 256) & ((k % 4) // 2 == 1)] = water[f]
    return {f: np.tile(v, (ncol, 1)) for f, v in base.items()}


def open_engine(pkg, grid, nlat, ncol, what, **opt):
    st = space(pkg, grid, nlat)
    opt.setdefault("use_graph", False)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval), st.dt,
                     ncol, device=0, cells_per_thread=4, **opt)
    info = eng.launch_info()
    assert info["threads"] == THREADS[nlat] and info["cells_per_thread"] == 4
    eng.set_state(start_state(pkg, grid, nlat, ncol))
    if "nofcol" not in what:
        eng.set_column_forcing(np.linspace(-1.5, 1.5, ncol))
    eng.set_time_table(st.t)
    rest = tuple(w for w in what if w != "nofcol")
    if rest:
        member_installer(pkg, ncol, rest)(eng, slice(0, ncol))
    return eng


@functools.lru_cache(maxsize=None)
def fused_steps(pkg, grid, nlat, ncol, what):
    """The reference, computed once per case and left unchanged: every field after step MID and after the last, each step taken
    by ebm_run_fused with diagnostics; the counters; with forcing noise, N_c after the last."""
    out = {}
    f = forcing_of(0, NSTEPS)
    with open_engine(pkg, grid, nlat, ncol, what) as eng:
        for s in range(NSTEPS):
            eng.run(s, 1, f[s:s + 1], True, 2)
            if s in (MID, NSTEPS - 1):
                out[s] = eng.get_state(ALL)
        counters = eng.counters()
        noise = eng.noise_state() if "noise" in what else None
    for s, fields in out.items():
        for k in PROG:
            assert np.isfinite(fields[k]).all(), (s, k)
    if what in ((), ("nofcol",)):
        # wave 0 holds a flagged pair (Ei, h, D of pair 1: zero bits) beside an unflagged one, from the first step to the last
        last = out[NSTEPS - 1]
        n = min(nlat, 256)
        pair = (np.arange(n) % 4) // 2
        for k in ("Ei", "h", "D"):
            assert (bits(last[k])[:, :n][:, pair == 1] == 0).all() and (bits(last[k])[:, :n][:, pair == 0] != 0).all(), k
    assert counters["solves"] >= ncol * NSTEPS
    return out, counters, noise


def check_end(eng, ref, counters, noise, what):
    got = eng.get_state(ALL)
    same(got, ref, what)
    c = eng.counters()
    assert (c["steps"], c["solves"], c["cap_hits"]) == (counters["steps"], counters["solves"], counters["cap_hits"]), (what, c, counters)
    if noise is not None:
        same(eng.noise_state(), noise, (what, "N_c"))


@pytest.mark.parametrize("path", ["step", "run"])
@pytest.mark.parametrize("what", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_single_steps(pkg, grid, nlat, ncol, what, path):
    """Six one-step launches with the step's scalars in the launch arguments — ebm_step (the handle's step clock) and ebm_run
    — and a diagnostic step in the middle; eliding zero lines (the flags are trusted from the second launch on) and not."""
    ref, counters, noise = fused_steps(pkg, grid, nlat, ncol, what)
    st = space(pkg, grid, nlat)
    f = forcing_of(0, NSTEPS)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, what, elide_zero_lines=elide) as eng:
            if path == "step":
                for s in range(NSTEPS):
                    eng.step(st.ct[s], st.ct[(s + 1) % NSTEPS], f[s], s in (MID, NSTEPS - 1))
                    if s == MID:
                        same(eng.get_state(ALL), ref[MID], (path, elide, "middle"))
            else:
                eng.run(0, MID + 1, f[:MID + 1], True)
                same(eng.get_state(ALL), ref[MID], (path, elide, "middle"))
                eng.run(MID + 1, NSTEPS - MID - 1, f[MID + 1:], True)
            assert eng.counters()["launches"] == NSTEPS
            check_end(eng, ref[NSTEPS - 1], counters, noise, (path, elide))


@functools.lru_cache(maxsize=None)
def fused_run(pkg, grid, nlat, ncol, what):
    """The graph test's reference: NGRAPH steps by ebm_run_fused, 11 steps per launch, diagnostics at the end."""
    with open_engine(pkg, grid, nlat, ncol, what) as eng:
        eng.run(0, NGRAPH, forcing_of(0, NGRAPH), True, 11)
        return eng.get_state(ALL), eng.counters(), eng.noise_state() if "noise" in what else None


@pytest.mark.parametrize("what", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_graph_replay(pkg, grid, nlat, ncol, what):
    """ebm_run replayed as a graph: every launch reads the step's scalars from its entry of the schedule table."""
    ref, counters, noise = fused_run(pkg, grid, nlat, ncol, what)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, what, elide_zero_lines=elide, use_graph=True) as eng:
            eng.run(0, NGRAPH, forcing_of(0, NGRAPH), True)
            check_end(eng, ref, counters, noise, ("graph", elide))
