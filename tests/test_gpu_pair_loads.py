"""GPU tests (-m gpu) of phase D's input loads in the one-step kernels (csrc/ebm_miz_step.h): where a lane's two pairs of Ei and D
are requested relative to the pairs' stores must change nothing a caller can see.

Reference: the same steps through ebm_run_fused, one step per call with diagnostics — the register / resident fused kernels,
which share the physics and none of the one-step kernel's load and store order.  Every comparison is bitwise (uint64 views:
signs of zero and NaN payloads of the diagnostics count) and sets no tolerance.  The one-step kernels are also run on a second
handle with elide_zero_lines = 0 (the kernel that loads and stores every line).

Shapes, the smallest at which each thing can go wrong: 258 x 3 (128 threads, padding in the last chunk), 1025 x 2 (320
threads, one valid cell in the last pair), 1796 x 3 (512 threads, the plan above 64 KiB), 4096 x 2 (1024 threads, the
headline's instantiation).  Both grids.

States: the golden mid-year state resampled by nearest-cell copy (support.midyear_state), then, in every column, the cells of
wave 0 (cells 0 .. 255; lane t owns cells 4 t .. 4 t + 3, pair j of it cells 4 t + 2 j and 4 t + 2 j + 1) take the WHOLE state
of one of three donor cells of that resampled state — `ice` (ice over water above freezing: nothing zero), `frozen` (ice, Ew =
+0.0) and `water` (no ice: Ei = h = D = phi = +0.0) — so that after the launch that sets the flags, pair 0 and pair 1 of that
wave carry different flags:

  edge_in_pair0   pair 0: ice in lanes 0 .. 31, water in lanes 32 .. 63 (no flag);  pair 1: water (Ei, h, D flagged)
  edge_in_pair1   the reverse
  no_ice          the whole column water (every Ei, h, D line flagged)
  all_ice_Ew0     the whole column frozen (every Ew line flagged)
  pair1_no_ice    pair 0: ice (no flag);  pair 1: water (Ei, h, D flagged, Ew not)
  pair1_Ew0       pair 0: ice (no flag);  pair 1: frozen (Ew flagged, Ei, h, D not)

At these time steps (1 / nt of a year, nt >= nlat^2 / 4) twelve steps move no ice edge: the patterns stand throughout, which
the tests assert on the reference's fields.  With the C oracle every state steps on finitely for the twelve steps
(test_the_states_step_finitely, on the CPU).
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, assert_same_bits as same, bits, forcing_of, member_installer, midyear_state

pytestmark = pytest.mark.gpu

TEN = ("Ei", "Ew", "h", "D", "phi", "E", "T", "Ti", "Tw", "n")
ALL = TEN + ("T0",)
FLAGGED = ("Ei", "Ew", "h", "D")                 # bit 4 j + f of a wave's word: pair j of FLAGGED[f]
SHAPES = [(258, 3), (1025, 2), (1796, 3), (4096, 2)]
THREADS = {258: 128, 1025: 320, 1796: 512, 4096: 1024}
NT = {258: 20000, 1025: 270000, 1796: 1000000, 4096: 4200000}     # steps per year, nt >= nlat^2 / 4
GRIDS = ["sin", "identity"]
STATES = ["edge_in_pair0", "edge_in_pair1", "no_ice", "all_ice_Ew0", "pair1_no_ice", "pair1_Ew0"]
NSTEPS = 12
# what pair 0 / pair 1 of wave 0 must be flagged for, of (Ei, Ew, h, D)
PATTERN = {"edge_in_pair0": ((0, 0, 0, 0), (1, 0, 1, 1)), "edge_in_pair1": ((1, 0, 1, 1), (0, 0, 0, 0)),
           "no_ice": ((1, 0, 1, 1), (1, 0, 1, 1)), "all_ice_Ew0": ((0, 1, 0, 0), (0, 1, 0, 0)),
           "pair1_no_ice": ((0, 0, 0, 0), (1, 0, 1, 1)), "pair1_Ew0": ((0, 0, 0, 0), (0, 1, 0, 0))}


class Space:
    def __init__(self, pkg, grid, nlat):
        st = pkg.SpaceTime(grid, nlat, 2000, 1)
        self.x, self.grid_kind, self.dt = st.x, st.grid_kind, 1.0 / NT[nlat]
        self.t = np.array([(2 * i + 1) / (2.0 * NT[nlat]) + 0.5 for i in range(NSTEPS)])     # mid-year; step 12's successor is step 1
        self.ct = np.array([pkg.cos2pit(float(t)) for t in self.t])


@functools.lru_cache(maxsize=None)
def space(pkg, grid, nlat):
    return Space(pkg, grid, nlat)


def offsets(ncol):
    return np.linspace(-1.5, 1.5, ncol)


@functools.lru_cache(maxsize=None)
def start_state(pkg, grid, nlat, ncol, name):
    """{field: [ncol][nlat]} of PROG + T0, every column the same."""
    st = space(pkg, grid, nlat)
    base = {k: v[0].copy() for k, v in midyear_state("MIZ", st, 1).items()}
    icy = base["h"] > 0
    donors = {"ice": int(np.flatnonzero(icy & (base["Ew"] != 0))[0]), "frozen": int(np.flatnonzero(icy & (base["Ew"] == 0))[0])}
    cell = {d: {k: base[k][i] for k in base} for d, i in donors.items()}
    open_water = np.flatnonzero(~icy & (base["Ew"] != 0))
    if open_water.size:
        cell["water"] = {k: base[k][int(open_water[0])] for k in base}
    else:                                          # (the identity grid's golden state has ice everywhere: the ice taken off)
        cell["water"] = dict(cell["ice"], Ei=0.0, h=0.0, D=0.0, phi=0.0)
    k = np.arange(nlat)
    lane, pair, wave0 = (k // 4) % 64, (k % 4) // 2, k < 256
    donor = np.full(nlat, "", dtype=object)
    if name in ("edge_in_pair0", "edge_in_pair1"):
        edge = int(name[-1])
        donor[wave0 & (pair == edge)] = "water"
        donor[wave0 & (pair == edge) & (lane < 32)] = "ice"
        donor[wave0 & (pair != edge)] = "water"
    elif name == "no_ice":
        donor[:] = "water"
    elif name == "all_ice_Ew0":
        donor[:] = "frozen"
    else:
        donor[wave0 & (pair == 0)] = "ice"
        donor[wave0 & (pair == 1)] = "water" if name == "pair1_no_ice" else "frozen"
    for d in cell:
        for f in base:
            base[f][donor == d] = cell[d][f]
    return {f: np.tile(v, (ncol, 1)) for f, v in base.items()}


def wave0_flags(fields, nlat):
    """[ncol][pair][field of FLAGGED]: wave 0's cells of that pair hold only zero bits (cells beyond nlat are padding: zero)."""
    ncol = fields["Ei"].shape[0]
    out = np.zeros((ncol, 2, 4), dtype=bool)
    for f, name in enumerate(FLAGGED):
        padded = np.zeros((ncol, 256), dtype=np.uint64)
        n = min(nlat, 256)
        padded[:, :n] = bits(fields[name])[:, :n]
        out[:, :, f] = (padded.reshape(ncol, 64, 2, 2) == 0).all(axis=(1, 3))
    return out


def assert_pattern(fields, nlat, name, what):
    got = wave0_flags(fields, nlat)
    want = np.array(PATTERN[name], dtype=bool)
    assert (got == want[None]).all(), (what, name, got[0].astype(int).tolist())


def assert_finite(fields, what):
    for k in PROG:
        assert np.isfinite(fields[k]).all(), (what, k)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_states_step_finitely(pkg, coracle, grid, nlat, ncol, state):
    """With the oracle, on the CPU: every prognostic field finite after each of the twelve steps, and wave 0's pairs flagged
    as the state's name says after the first step and after the last."""
    st = space(pkg, grid, nlat)
    s = {k: v.copy() for k, v in start_state(pkg, grid, nlat, ncol, state).items()}
    f = forcing_of(0, NSTEPS)
    with np.errstate(all="ignore"):
        for i in range(NSTEPS):
            coracle.miz_run(0 if grid == "identity" else 1, st.x, dict(pkg.default_parameters("MIZ")), st.dt, st.ct[i:i + 1], f[i:i + 1],
                            offsets(ncol), s)
            assert_finite(s, f"step {i}")
            if i in (0, NSTEPS - 1):
                assert_pattern(s, nlat, state, f"step {i}")


def open_engine(pkg, grid, nlat, ncol, state, what=(), **opt):
    st = space(pkg, grid, nlat)
    par = pkg.default_parameters("MIZ")
    opt.setdefault("use_graph", False)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0,
                     cells_per_thread=4, **opt)
    info = eng.launch_info()
    assert info["threads"] == THREADS[nlat] and info["cells_per_thread"] == 4
    eng.set_state(start_state(pkg, grid, nlat, ncol, state))
    eng.set_column_forcing(offsets(ncol))
    eng.set_time_table(st.t)
    if what:
        member_installer(pkg, ncol, what)(eng, slice(0, ncol))
    return eng


@functools.lru_cache(maxsize=None)
def fused_steps(pkg, grid, nlat, ncol, state, what=()):
    """The reference, computed once per case and left unchanged: every field after each of the twelve steps, each taken by
    ebm_run_fused with diagnostics; with forcing noise, N_c after the last."""
    out = []
    f = forcing_of(0, NSTEPS)
    with open_engine(pkg, grid, nlat, ncol, state, what) as eng:
        for s in range(NSTEPS):
            eng.run(s, 1, f[s:s + 1], True, 2)
            out.append(eng.get_state(ALL))
        noise = eng.noise_state() if "noise" in what else None
    for s, fields in enumerate(out):
        assert_finite(fields, f"reference, step {s}")
    if "params" not in what and "noise" not in what:
        assert_pattern(out[0], nlat, state, "reference, first step")
        assert_pattern(out[-1], nlat, state, "reference, last step")
    return out, noise


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_twelve_single_steps(pkg, grid, nlat, ncol, state, graph):
    """ebm_run, one launch per step, the last with diagnostics: eliding zero lines (the flags are trusted from the second
    launch on) and not."""
    ref, _ = fused_steps(pkg, grid, nlat, ncol, state)
    f = forcing_of(0, NSTEPS)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, state, elide_zero_lines=elide, use_graph=graph) as eng:
            eng.run(0, NSTEPS, f, True)
            assert eng.counters()["launches"] == NSTEPS
            got = eng.get_state(ALL)
        assert_finite(got, "ebm_run")
        same(got, ref[-1], f"ebm_run, elide_zero_lines = {elide}")


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_a_diagnostic_step_every_third(pkg, grid, nlat, ncol, state):
    """ebm_step, every third one with diagnostics: all ten fields and T0 there."""
    ref, _ = fused_steps(pkg, grid, nlat, ncol, state)
    st = space(pkg, grid, nlat)
    f = forcing_of(0, NSTEPS)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, state, elide_zero_lines=elide) as eng:
            for s in range(NSTEPS):
                eng.step(st.ct[s], st.ct[(s + 1) % NSTEPS], f[s], s % 3 == 2)
                if s % 3 == 2:
                    got = eng.get_state(ALL)
                    assert_finite(got, f"step {s}")
                    same(got, ref[s], f"ebm_step {s}, elide_zero_lines = {elide}")


MIZ_VARS = ("E", "T", "h", "Ei", "Ew", "Ti", "Tw", "D", "phi", "n")


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_a_year_of_twelve_steps_with_sums(pkg, grid, nlat, ncol, state):
    """ebm_integrate, one launch per step (the kernel that also adds to savesol!'s sums): the fields at the end, and the
    annual mean against the sequential sum of the reference's fields / 12."""
    ref, _ = fused_steps(pkg, grid, nlat, ncol, state)
    with open_engine(pkg, grid, nlat, ncol, state, integrate_steps_per_launch=1) as eng:
        out = eng.integrate(NSTEPS, 1, forcing_of(0, NSTEPS), True, 3, 7, MIZ_VARS, want_raw=False, want_seasonal=False)
        got = eng.get_state(ALL)
    assert_finite(got, "ebm_integrate")
    same(got, ref[-1], "ebm_integrate")
    for v, name in enumerate(MIZ_VARS):
        acc = np.zeros((ncol, nlat))
        with np.errstate(invalid="ignore"):
            for fields in ref:
                acc = acc + fields[name]
            mean = acc / float(NSTEPS)
        same(out["avg"][v, 0], mean, ("annual mean", name))


@pytest.mark.parametrize("what,grid,nlat,ncol,state", [(("noise",), "sin", 4096, 2, "edge_in_pair1"),
                                                      (("params",), "identity", 1025, 2, "pair1_no_ice")],
                         ids=["forcing_noise", "two_parameter_sets"])
def test_with_member_settings(pkg, what, grid, nlat, ncol, state):
    """Forcing noise drawn on the device, and a parameter set per column."""
    ref, noise = fused_steps(pkg, grid, nlat, ncol, state, what)
    for elide in (True, False):
        with open_engine(pkg, grid, nlat, ncol, state, what, elide_zero_lines=elide) as eng:
            eng.run(0, NSTEPS, forcing_of(0, NSTEPS), True)
            got = eng.get_state(ALL)
            if noise is not None:
                same(eng.noise_state(), noise, "N_c")
        assert_finite(got, what)
        same(got, ref[-1], (what, elide))
