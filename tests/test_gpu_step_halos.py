"""GPU tests (-m gpu) of the halo exchanges of the one-step kernels' first Newton pass (csrc/ebm_miz_step.h, the kernels of the
batched head): r and the masked g go round behind ONE barrier (halo_exchange_two), and the Tbar halo is published before the
active-set vote and read after it (publish_then_vote), so that phase D starts with its halo in hand — the latter in the kernels
above 256 threads (1026 x 3 and 4096 x 2 below; at 200 and 258 cells phase D exchanges Tbar itself).  None of it may change
anything a caller can see.

Reference: the same steps through ebm_run_fused, one step per call with diagnostics — the fused kernels, which share the
physics, exchange r, g and Tbar one after the other and form Tbar after the vote.  Every comparison is bitwise and sets no
tolerance; the solve and cap-hit counters must equal the reference's.

Shapes, the smallest that have in turn no wave boundary (200 x 3: 64 threads), one wave boundary (258 x 3: 128 threads, the
second wave holds one live lane), a partial last wave (1026 x 3: 320 threads) and the full workgroup (4096 x 2: 1024 threads).
Both grids.

Starts.  What the vote decides is only exercised by column-steps that solve more than once: the words published under a vote
that said "again" must be dropped, the second pass must exchange g on its own, and the halo that phase D uses must be the last
pass's.  Three starts, each checked with the CPU oracle (oracle/c_oracle.py, miz_run's solve counter) to re-iterate at every
shape on both grids within the six steps taken here — solves per 6 x ncol column-steps, sin / identity grid:
    the golden mid-year state at the shape's stable time step   200: 23 / 23 of 18   258: 28 / 24 of 18   1026: 45 / 46 of 18   4096: 66 / 116 of 12
    the golden mid-year state at nt = 2000                       200: 27 / 23         258: 39 / 24         1026: 168 / 50        4096: 324 / 132
    the all-zero state at nt = 2000                              200: 25 / 24         258: 25 / 30         1026: 39 / 36         4096: 24 / 24
(nt = 2000 is far above the explicit limit at the longer shapes; six steps stay finite there, which the reference asserts.)
Every case asserts from the handle's own counters that its solves exceed steps x columns.  (The all-zero start changes sets
but grows no ice within these steps: phi = 0, so g and Tbar do not depend on the set or the solution there.  The mid-year
starts are the ones that see a wrong g halo or a Tbar halo kept from a pass that voted "again" —
tests/tools/mutants_step_halos.py.)  The 131-step replays of 1026 and 4096 cells start from the stable time step only: at
nt = 2000 those shapes leave the finite numbers within 131 steps, in the reference as well.

Entry points: ebm_step and ebm_run (a diagnostic step in the middle, whose T0 store must see the same values), ebm_run
replayed as a graph.  Handles: eliding zero lines and not; with and without the per-column forcing offsets, with two parameter
sets, with forcing noise (N_c compared).  The mask is compared through the next steps' results and, on diagnostic steps, T0.
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, assert_same_bits as same, forcing_of, member_installer, midyear_state

pytestmark = pytest.mark.gpu

ALL = ("Ei", "Ew", "h", "D", "phi", "E", "T", "Ti", "Tw", "n", "T0")
SHAPES = [(200, 3), (258, 3), (1026, 3), (4096, 2)]
THREADS = {200: 64, 258: 128, 1026: 320, 4096: 1024}
STABLE_NT = {200: 20000, 258: 20000, 1026: 270000, 4096: 4200000}      # steps per year, nt >= nlat^2 / 4
GRIDS = ["sin", "identity"]
STARTS = ["midyear", "midyear_2000", "zero_2000"]
NSTEPS, MID = 6, 2                                               # a diagnostic step at MID and at the end
NGRAPH = 131          # ebm_run replays its captured graph of 64 launches from 128 steps on: two replays, then single launches
NTABLE = NGRAPH + 1
# (start, member settings): every start with the column forcing; the other handle variants at the start that re-iterates most
CASES = [(s, ()) for s in STARTS] + [("midyear_2000", w) for w in (("nofcol",), ("params",), ("noise",))]
CASE_IDS = ["-".join((s,) + (w or ("fcol",))) for s, w in CASES]


class Space:
    def __init__(self, pkg, grid, nlat, nt):
        st = pkg.SpaceTime(grid, nlat, 2000, 1)
        self.x, self.grid_kind, self.dt = st.x, st.grid_kind, 1.0 / nt
        self.t = np.array([(2 * i + 1) / (2.0 * nt) + 0.5 for i in range(NTABLE)])
        self.ct = np.array([pkg.cos2pit(float(t)) for t in self.t])


@functools.lru_cache(maxsize=None)
def space(pkg, grid, nlat, start):
    return Space(pkg, grid, nlat, STABLE_NT[nlat] if start == "midyear" else 2000)


@functools.lru_cache(maxsize=None)
def start_state(pkg, grid, nlat, ncol, start):
    if start == "zero_2000":
        return {k: np.zeros((ncol, nlat)) for k in PROG + ("T0",)}
    return midyear_state("MIZ", space(pkg, grid, nlat, start), ncol)


def open_engine(pkg, grid, nlat, ncol, start, what, **opt):
    st = space(pkg, grid, nlat, start)
    opt.setdefault("use_graph", False)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval), st.dt,
                     ncol, device=0, cells_per_thread=4, **opt)
    info = eng.launch_info()
    assert info["threads"] == THREADS[nlat] and info["cells_per_thread"] == 4
    eng.set_state(start_state(pkg, grid, nlat, ncol, start))
    if "nofcol" not in what:
        eng.set_column_forcing(np.linspace(-1.5, 1.5, ncol))
    eng.set_time_table(st.t)
    rest = tuple(w for w in what if w != "nofcol")
    if rest:
        member_installer(pkg, ncol, rest)(eng, slice(0, ncol))
    return eng


@functools.lru_cache(maxsize=None)
def fused_steps(pkg, grid, nlat, ncol, start, what):
    """The reference, computed once per case and left unchanged: every field after step MID and after the last, each step taken
    by ebm_run_fused with diagnostics; the counters; with forcing noise, N_c after the last."""
    out = {}
    f = forcing_of(0, NSTEPS)
    with open_engine(pkg, grid, nlat, ncol, start, what) as eng:
        for s in range(NSTEPS):
            eng.run(s, 1, f[s:s + 1], True, 2)
            if s in (MID, NSTEPS - 1):
                out[s] = eng.get_state(ALL)
        counters = eng.counters()
        noise = eng.noise_state() if "noise" in what else None
    for s, fields in out.items():
        for k in PROG:
            assert np.isfinite(fields[k]).all(), (s, k)
    assert counters["solves"] > ncol * NSTEPS and counters["cap_hits"] == 0, counters      # column-steps that solved again
    return out, counters, noise


def check_end(eng, ref, counters, noise, steps, what):
    same(eng.get_state(ALL), ref, what)
    c = eng.counters()
    print(what, "solves", c["solves"], "of", steps * eng.ncol, "column-steps")
    assert c["solves"] > steps * eng.ncol, (what, c)
    assert (c["steps"], c["solves"], c["cap_hits"]) == (counters["steps"], counters["solves"], counters["cap_hits"]), (what, c, counters)
    if noise is not None:
        same(eng.noise_state(), noise, (what, "N_c"))


@pytest.mark.parametrize("path", ["step", "run"])
@pytest.mark.parametrize("start,what", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_single_steps(pkg, grid, nlat, ncol, start, what, path):
    """Six one-step launches by ebm_step and by ebm_run, a diagnostic step in the middle and at the end; eliding zero lines and
    not."""
    ref, counters, noise = fused_steps(pkg, grid, nlat, ncol, start, what)
    st = space(pkg, grid, nlat, start)
    f = forcing_of(0, NSTEPS)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, start, what, elide_zero_lines=elide) as eng:
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
            check_end(eng, ref[NSTEPS - 1], counters, noise, NSTEPS, (path, elide))


@functools.lru_cache(maxsize=None)
def fused_run(pkg, grid, nlat, ncol, start, what):
    """The graph test's reference: NGRAPH steps by ebm_run_fused, 11 steps per launch, diagnostics at the end."""
    with open_engine(pkg, grid, nlat, ncol, start, what) as eng:
        eng.run(0, NGRAPH, forcing_of(0, NGRAPH), True, 11)
        return eng.get_state(ALL), eng.counters(), eng.noise_state() if "noise" in what else None


# (1026 and 4096 cells at nt = 2000 do not stay finite for 131 steps, in the reference either: those shapes replay from the
# stable start, which re-iterates as well — the oracle's solves of 393 and 262 column-steps: 494 / 635 and 393 / 396)
GRAPH_CASES = [(nlat, ncol, s, w) for nlat, ncol in SHAPES for s, w in CASES if nlat <= 258 or s == "midyear"]


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol,start,what", GRAPH_CASES, ids=[f"{c[0]}-{c[1]}-" + "-".join((c[2],) + (c[3] or ("fcol",))) for c in GRAPH_CASES])
def test_graph_replay(pkg, grid, nlat, ncol, start, what):
    """ebm_run replayed as a graph over 131 steps: set changes in the middle of a replay."""
    ref, counters, noise = fused_run(pkg, grid, nlat, ncol, start, what)
    for k in PROG:
        assert np.isfinite(ref[k]).all(), k
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, start, what, elide_zero_lines=elide, use_graph=True) as eng:
            eng.run(0, NGRAPH, forcing_of(0, NGRAPH), True)
            check_end(eng, ref, counters, noise, NGRAPH, ("graph", elide))
