"""GPU tests (-m gpu) of zero-line elision in the state-only one-step kernel that derives phi (csrc/ebm_miz_step.h, ZERO_LINES;
FieldBook::zero_flags_trusted, csrc/ebm_fieldbook.h): a KiB of Ei, Ew, h or D that holds only zero bits is
neither loaded nor stored, on the word of one flag per (column, wave, pair, field).

Nothing a caller can see may change, so every comparison is bitwise (uint64 views) and sets no tolerance: a handle with
ebm_options.elide_zero_lines on against one with it off, the same calls on both — all five prognostic fields after phi is
restored, and the ten solution variables after one diagnostic step.  The flags read back (ebm_zero_line_flags) must EQUAL the
per-line "all zero bits" computed in numpy from the fields: set over a line that is not zero is a wrong result, clear over a
zero line a lost gain.

Scenario (SCENARIO steps from the zero state, checked with the C oracle once per shape — finite, and with the transitions
named below): the forcing falls (freeze-up: Ei, h, D of the lines that take ice go zero -> non-zero, their Ew goes non-zero
-> zero), then rises (the water under the ice warms: Ew goes zero -> non-zero); the columns' own offsets put their ice edges
at different latitudes, so that one edge crosses a wave's boundary while another stays inside a wave.

Melt-through (MELT steps from the zero state, checked with the oracle for every shape): at the time steps these shapes need
(1 / nt of a year, nt >= nlat^2 / 4) a few hundred W m^-2 neither form nor melt ice that the next steps could remove, so this
scenario's forcing is scaled with nt (0.3 nt W m^-2 warm, -0.15 nt cold: the same enthalpy per step on every shape) — one warm
step from zero (no ice: Ei, h, D lines zero), two cold steps (freeze-up), nine warm ones, within which the ice melts through:
an Ei, an h and a D line each go zero -> non-zero -> zero, an Ew line the reverse.

Shapes, the smallest per size class as in tests/test_gpu_noise_sizes.py: 258 x 3 (128 threads: the second wave holds one pair
of real cells, its other lines are padding and count as zero), 1025 x 2 (320 threads) and 4096 x 2 (1024 threads: the
headline kernel).  Both grids.
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, assert_same_bits as same, bits

pytestmark = pytest.mark.gpu

FLAGGED = ("Ei", "Ew", "h", "D")                 # bit 4 j + f of a wave's word: pair j of FLAGGED[f]
TEN = ("Ei", "Ew", "h", "D", "phi", "E", "T", "Ti", "Tw", "n")
SHAPES = [(258, 3), (1025, 2), (4096, 2)]
THREADS = {258: 128, 1025: 320, 4096: 1024}
NT = {258: 20000, 1025: 270000, 4096: 4200000}   # steps per year, nt >= nlat^2 / 4; its own: 4096 cells step explicitly here
GRIDS = ["sin", "identity"]
SCENARIO = 16                                    # steps
CHECKPOINTS = (1, 2, 3, 5, 8, 12, 16)            # where the step-by-step test reads flags and fields


# W m^-2 per step: cold, colder (the ice edge advances), the same again (it stays where it is), then warmer and warmer
FORCING = np.array([-40.0, -80.0, -80.0, 0.0, 60.0, 120.0, 180.0, 240.0, 300.0, 360.0, 420.0, 480.0, 540.0, 600.0, 600.0, 600.0])


def forcing(first, n):
    """Steps first .. first + n - 1 of the scenario's forcing; its last value from then on."""
    return FORCING[np.minimum(first + np.arange(n), SCENARIO - 1)]


MELT = 12                                        # steps of the melt-through scenario


def melt_forcing(nlat):
    table = np.array([0.3] + [-0.15] * 2 + [0.3] * (MELT - 3)) * NT[nlat]
    return lambda first, n: table[np.minimum(first + np.arange(n), MELT - 1)]


def offsets(ncol):
    return np.linspace(-40.0, 40.0, ncol)


class Space:
    def __init__(self, pkg, grid, nlat):
        st = pkg.SpaceTime(grid, nlat, 2000, 1)
        self.x, self.grid_kind, self.dt = st.x, st.grid_kind, 1.0 / NT[nlat]
        self.t = np.array([(2 * i + 1) / (2.0 * NT[nlat]) for i in range(256)])       # (winter: the year's first steps)


@functools.lru_cache(maxsize=None)
def space(pkg, grid, nlat):
    return Space(pkg, grid, nlat)


def line_flags(fields, nlat):
    """The flag words [ncol][threads / 64] that the fields call for: bit 4 j + f set iff cells 4 t + 2 j and 4 t + 2 j + 1 of
    the wave's threads t hold only zero bits in FLAGGED[f] (cells beyond nlat are padding: zero)."""
    T = THREADS[nlat]
    ncol = fields["Ei"].shape[0]
    words = np.zeros((ncol, T // 64), dtype=np.uint32)
    for f, name in enumerate(FLAGGED):
        padded = np.zeros((ncol, 4 * T), dtype=np.uint64)
        padded[:, :nlat] = bits(fields[name])
        per_pair = padded.reshape(ncol, T // 64, 64, 2, 2)            # [col][wave][thread][pair][cell]
        zero = (per_pair == 0).all(axis=(2, 4))                        # [col][wave][pair]
        for j in range(2):
            words |= (zero[:, :, j].astype(np.uint32) << np.uint32(4 * j + f))
    return words


@functools.lru_cache(maxsize=None)
def oracle_scenario(pkg, coracle, grid, nlat, ncol, melt=False):
    """A scenario with the C oracle: (all finite, the flag words after every step [steps][ncol][waves])."""
    st = space(pkg, grid, nlat)
    state = {k: np.zeros((ncol, nlat)) for k in PROG + ("T0",)}
    nsteps = MELT if melt else SCENARIO
    ct = np.array([pkg.cos2pit(float(t)) for t in st.t[:nsteps]])
    f = (melt_forcing(nlat) if melt else forcing)(0, nsteps)
    finite, words = True, []
    with np.errstate(all="ignore"):
        for s in range(nsteps):
            coracle.miz_run(0 if grid == "identity" else 1, st.x, dict(pkg.default_parameters("MIZ")), st.dt, ct[s:s + 1], f[s:s + 1],
                            offsets(ncol), state)
            finite = finite and all(np.isfinite(state[k]).all() for k in PROG)
            assert not any((np.signbit(state[k]) & (state[k] == 0.0)).any() for k in FLAGGED)      # no negative zero
            words.append(line_flags(state, nlat))
    return finite, np.array(words)


def bit(j, name):
    return np.uint32(1 << (4 * j + FLAGGED.index(name)))


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_scenario_has_the_transitions(pkg, coracle, grid, nlat, ncol):
    """With the oracle, on the CPU: finite; flags both set and clear at some step; an Ew line non-zero -> zero and zero ->
    non-zero between consecutive steps, an Ei line zero -> non-zero, an ice edge that crosses a wave boundary (one wave's
    Ei lines change while another's keep differing from them) and a step across which a column has ice and open water and no
    Ei line changes (the edge stays inside a wave)."""
    finite, w = oracle_scenario(pkg, coracle, grid, nlat, ncol)
    assert finite
    assert w.any() and (w != 0xFF).any()                              # a flag set and a flag clear at some step
    if nlat < 4096:
        return                                                         # (few waves: the transitions below are the long shape's)
    was, now = w[:-1], w[1:]
    b = bit(0, "Ew")
    assert ((was & b != 0) & (now & b == 0)).any() and ((was & b == 0) & (now & b != 0)).any(), "Ew"
    b = bit(0, "Ei")
    assert ((was & b != 0) & (now & b == 0)).any(), "no line takes ice"
    e0 = (w & b) != 0                                                  # [step][col][wave]
    mixed = e0.any(axis=2) & ~e0.all(axis=2)                           # the column has an ice edge between two waves
    assert (mixed[:-1] & mixed[1:] & (e0[:-1] != e0[1:]).any(axis=2)).any(), "no edge crosses a wave boundary"
    assert (mixed[:-1] & mixed[1:] & (e0[:-1] == e0[1:]).all(axis=2)).any(), "no edge stays inside a wave"


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_melt_scenario_melts_through(pkg, coracle, grid, nlat, ncol):
    """With the oracle, on the CPU: finite, and some line's flag of each of Ei, h and D goes set -> clear -> set (no ice, ice,
    melted through) while an Ew flag goes clear -> set -> clear."""
    finite, w = oracle_scenario(pkg, coracle, grid, nlat, ncol, melt=True)
    assert finite

    def goes(seq, first):
        """some line's flag is `first`, later the opposite, later `first` again"""
        a = seq == first
        seen_first = np.logical_or.accumulate(a, axis=0)
        seen_other = np.logical_or.accumulate(seen_first & ~a, axis=0)
        return (seen_other & a).any()
    for name in ("Ei", "h", "D"):
        assert goes((w & bit(0, name)) != 0, True), name
    assert goes((w & bit(0, "Ew")) != 0, False), "Ew"


def open_engine(pkg, grid, nlat, ncol, elide, **opt):
    st = space(pkg, grid, nlat)
    par = pkg.default_parameters("MIZ")
    opt.setdefault("use_graph", False)
    eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0,
                     elide_zero_lines=elide, **opt)
    info = eng.launch_info()
    assert info["threads"] == THREADS[nlat] and info["cells_per_thread"] == 4
    eng.set_column_forcing(offsets(ncol))
    eng.set_time_table(st.t)
    return eng


class Pair:
    """Two handles from the zero state: `on` elides zero lines, `off` does not.  Every call goes to both."""

    def __init__(self, pkg, grid, nlat, ncol, forcing=forcing, **opt):
        self.nlat, self.forcing = nlat, forcing
        self.on = open_engine(pkg, grid, nlat, ncol, True, **opt)
        self.off = open_engine(pkg, grid, nlat, ncol, False, **opt)
        self.pos = 0
        self.seen_set = self.seen_clear = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.on.close()
        self.off.close()
        return False

    def run(self, n, diag=False, **kw):
        f = self.forcing(self.pos, n)
        for e in (self.on, self.off):
            e.run(self.pos, n, f, diag, **kw)
        self.pos += n

    def both(self, call):
        return call(self.on), call(self.off)

    def check(self, what="", flags=True):
        """The flags first — reading a field un-splits, after which they are not trusted — then the fields, bit for bit."""
        if flags:
            words, trusted = self.on.zero_line_flags()
            assert trusted, what
        got, ref = self.on.get_state(PROG), self.off.get_state(PROG)
        same(got, ref, what)
        if flags:
            want = line_flags(ref, self.nlat)
            assert np.array_equal(words, want), (what, words, want)
            nbits = 8 * words.size
            nset = int(sum(bin(int(v)).count("1") for v in words.ravel()))
            self.seen_set |= nset > 0
            self.seen_clear |= nset < nbits
        words, trusted = self.on.zero_line_flags()
        assert not trusted or not words.any(), "flags trusted after the fields were moved"
        return ref

    def assert_flags_were_seen(self):
        assert self.seen_set and self.seen_clear


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_scenario_step_by_step(pkg, grid, nlat, ncol, graph):
    """Flags and fields at every checkpoint of the scenario (between two checkpoints the flags are trusted from the second
    step on), then one diagnostic step: the ten variables.  graph: the same through ebm_run's replay path, 130 more steps."""
    with Pair(pkg, grid, nlat, ncol, use_graph=graph) as p:
        for c in CHECKPOINTS:
            p.run(c - p.pos)
            p.check(f"step {c}")
        if graph:
            p.run(130)
            p.check("after a replay")
        p.run(1, diag=True)
        same(p.on.get_state(TEN), p.off.get_state(TEN), "diagnostic step")
        p.assert_flags_were_seen()
        assert all(np.isfinite(v).all() for v in p.off.get_state(PROG).values())


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_the_scenario_in_one_run(pkg, grid, nlat, ncol):
    """The whole scenario with nothing in between: every transition is met with trusted flags."""
    with Pair(pkg, grid, nlat, ncol) as p:
        p.run(SCENARIO)
        p.check("scenario")
        p.assert_flags_were_seen()


@pytest.mark.parametrize("one_run", [False, True], ids=["step_by_step", "one_run"])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("nlat,ncol", SHAPES)
def test_melt_through(pkg, grid, nlat, ncol, one_run):
    """The melt-through scenario: flags and fields after the warm first steps, the freeze-up, and inside and after the melt —
    or after the whole of it with nothing in between, every transition met with trusted flags."""
    with Pair(pkg, grid, nlat, ncol, forcing=melt_forcing(nlat)) as p:
        for c in ((MELT,) if one_run else (2, 3, 5, 7, MELT)):
            p.run(c - p.pos)
            p.check(f"step {c}")
        p.assert_flags_were_seen()
        assert all(np.isfinite(v).all() for v in p.off.get_state(PROG).values())


def one_icy_cell(p):
    """Exactly one icy cell, through set_field, into a line whose Ei flag is set (cell 7 of the last column where no real
    line is flagged)."""
    words, _ = p.on.zero_line_flags()
    col, cell = p.on.ncol - 1, 7
    for c, w in zip(*np.nonzero(words & bit(0, "Ei"))):
        if 256 * w + 4 < p.nlat:
            col, cell = int(c), 256 * int(w) + 4
            break

    def put(e):
        s = e.get_state(PROG)
        s["Ei"][col, cell], s["h"][col, cell], s["D"][col, cell], s["phi"][col, cell] = -0.95, 0.2, 10.0, 0.5
        for k in ("Ei", "h", "D", "phi"):
            e.set_field(k, s[k])
    p.both(put)


def parents_of(ncol):
    return np.array([(c + 1) % ncol for c in range(ncol)], dtype=np.int32)


def import_columns(p):
    """Column 0 takes the state of the last column, on the device, through export and import."""
    import torch

    def move(e):
        buf = torch.zeros((1, e.column_record()[0]), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        mask = e.export_columns([e.ncol - 1], buf.data_ptr())
        e.import_columns([0], buf.data_ptr(), mask)
        e.sync()
    p.both(move)


OUTSIDE = {
    "set_field": one_icy_cell,
    "get_field": lambda p: p.both(lambda e: e.get_field("Ew")),
    "fused": lambda p: p.run(4, steps_per_launch=2),
    "equilibrate": lambda p: p.both(lambda e: e.equilibrate(256, 1, None, {"Ei": 0.0})),
    "import": import_columns,
    "resample": lambda p: p.both(lambda e: e.resample_columns(parents_of(e.ncol))),
}


@pytest.mark.parametrize("writer", sorted(OUTSIDE))
@pytest.mark.parametrize("grid,nlat,ncol", [("sin", 258, 3), ("identity", 1025, 2), ("sin", 4096, 2)])
def test_an_outside_write_takes_the_trust_away(pkg, grid, nlat, ncol, writer):
    """The scenario, after which flags are set and trusted; then somebody
    else writes — non-zero values into flagged lines, or the same lines into another layout: the flags are clear or untrusted,
    and the steps that follow are those of the handle without flags."""
    with Pair(pkg, grid, nlat, ncol) as p:
        p.run(SCENARIO)
        words, trusted = p.on.zero_line_flags()
        assert trusted and words.any()
        OUTSIDE[writer](p)
        words, trusted = p.on.zero_line_flags()
        assert not trusted or not words.any(), writer
        for n in (1, 2, 3):
            p.run(n)
            # (a writer of Ei, h or phi makes the first step load the phi that is stored: another kernel, no trust yet)
            trusted = p.on.zero_line_flags()[1]
            assert trusted or n == 1, writer
            p.check(f"{writer} + {n}", flags=trusted)
        p.assert_flags_were_seen()
        assert all(np.isfinite(v).all() for v in p.off.get_state(PROG).values())


@pytest.mark.parametrize("variant", ["two_chains", "resampled_between"])
@pytest.mark.parametrize("grid,nlat", [("sin", 258), ("identity", 4096)])
def test_two_launch_chains(pkg, grid, nlat, variant):
    """Two launch chains over three columns (1 / 2): each chain's launches keep the flags of its own columns.
    resampled_between: after the scenario a resampling copies column 1 over column 2 — every flag is cleared — and the
    stepping goes on: the flags of each chain's columns are rebuilt by its own launches.
    (No call steps a SUBSET of the columns with the one-step kernel: ebm_equilibrate and ebm_run_until step their active
    lists with the fused kernels, after which no flag is trusted — the `equilibrate` writer above.  That an eliding launch
    over some columns keeps the other columns' flags true is the rule of the book, walked in tests/host_zero_flags_main.cpp,
    event step_chain0.)"""
    with Pair(pkg, grid, nlat, 3, launch_chains=2) as p:
        p.run(SCENARIO)
        p.check("two chains")
        if variant == "resampled_between":
            p.run(3)
            p.both(lambda e: e.resample_columns(np.array([0, 1, 1], dtype=np.int32)))
            p.run(1)                          # (loads the phi that is stored: another kernel)
            p.run(3)
            p.check("after the resampling")
        p.assert_flags_were_seen()
