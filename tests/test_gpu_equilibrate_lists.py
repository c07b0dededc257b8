"""GPU tests (-m gpu) of ebm_equilibrate's ACTIVE LIST past one wave and one round, and of NaN sentinels in some cells only.

ebm_equilibrate steps the entries of a device-side list that compact_active_kernel (csrc/ebm_launch.hip) rebuilds every year
— per wave a ballot and a popcount below the lane, across the 16 waves a scan of wave_base[] in LDS, rounds of 1024 entries
that carry `total` — and that the check and step kernels read through cols[blockIdx.x]; with two launch chains the host cuts
the LIST in two (csrc/ebm_drive.hip).  tests/test_gpu_equilibrate.py runs 4 to 12 columns: one partial wave, one round.
Here the ensembles have 65, 1024, 1025 and 2100 columns, 3 and 2 for the tail of two chains.

The oracle is the one of tests/test_gpu_equilibrate.py and involves no new code: a second handle steps plain ebm_run_fused
over ALL columns a year at a time, every field comes down every year, and NumPy restates the header's criterion.
ebm_equilibrate must reproduce years, converged and resid (bit patterns where finite), every field of every column at the
column's own year, ebm_field_step and counters[0].  Two more numbers come from the reference alone:
  counters[3]  the launches: sum over the years run of ceil(nt / K) x (chains that had columns), with nactive_y = #{c : Y_c
               >= y} — the host's view of the list length, every year;
  counters[1]  the solves.  Neither model's counter is "one solve per column-step": classic_step_kernel does exactly one
               tridiagonal solve per column-step but never touches the counters (they stay 0), and the MIZ kernels count
               the Newton iterations of the T0 solve, which vary.  So nt * sum(Y_c) is NOT asserted.  What is asserted for
               the MIZ models: a one-column handle per member type, stepped a year at a time, gives the iterations of that
               type in each year (the header: a column gives the same bits and counters alone), and counters[1] must be
               their sum over the column-years the reference says were stepped.  A list that holds a column twice has two
               workgroups load, step and store the same values — the fields come out right; only this count doubles.

Shapes: nlat = 16, nt = 200 (the compaction does not care about nlat).  The members are of a handful of TYPES (TYPES below)
chosen with the CPU oracle: warm open water relaxing towards a strongly forced state, whose year-on-year distance in T
falls smoothly by a quarter a year (4.8, 3.1, 2.1, 1.5, 1.1 K), started after 3, 2, 1 and 0 years of spin-up, so that under
the tolerance "the unspun type's own distance of year 5" they freeze in years 2, 3, 4 and 5; colder water under another
D and forcing, still at 2.5 K in year 6 (never converges); the golden fixtures' icy mid-year state resampled cell by
cell, whose ice edge keeps jumping (never converges; in the classic model it settles in year 5); and one all-NaN column
(the classic step writes T = 0 for it, so there the criterion is T and E: see `criterion`).
The test asserts FROM THE REFERENCE that every type has the year written in TYPES, that the non-NaN members are finite in
every year and that a frozen column of each early type would have moved on — else it fails with the distances printed.
PATTERNS maps column index to type; tests/test_host_equilibrate_lists.py (CPU) checks, by replaying the compaction in
NumPy, that each pattern has an empty wave, a wave where only lane 0 / only lane 63 / every lane but 63 survives, an empty
round between live ones, and so on.

Which wrong build fails where (argued from the code; no mutant is run: a broken compaction indexes out of bounds):
  `below` off by one.  Counting the lane itself moves every survivor one slot up: slot 0 keeps a stale entry and the last
      survivor falls behind `count` — in every pattern the last column (NEVER / E5 / E4: it survives) stops stepping, and
      test_*[...] fail on years, fields and solves.  The variants that only the edges of a FULL wave show — a mask that is
      wrong for lane 63 ((2 << lane) - 1 shifted the other way, 1ull << (lane + 1)), a 32-bit popcount that drops lanes
      32 .. 63 — need a survivor in lane 63 behind others: rows "lane63" (it must land in slot base + 0), "all" (base + 63)
      and "all_but63" (the next wave's base is 63 further, not 64), against "lane0" and "empty"; 4 to 12 columns never
      reach lane 12.
  wave_base read before the scan's barrier: a wave reads its base as the raw count of the wave before it, not the prefix
      sum — wrong wherever more than one earlier wave has survivors (rows "lane0" + "lane63" + "all_but63" precede "all");
      the 4 and 12 column tests have one wave, whose base is always wave_base[0].
  `total` not carried between rounds: round 1 of 1025 writes column 1024 to slot 0 over round 0's first survivor; in 2100
      the empty round 1024 .. 2047 must carry `total` UNCHANGED for round 2 to land behind round 0's survivors, and the
      count read by the host (counters[3] through the chains, years through the check launch) is the last round's only.

Time (one run of this module, then tests/test_gpu_equilibrate.py, with --durations=0 on an MI355X): the slowest test of
tests/test_gpu_equilibrate.py took 0.88 s (test_imex_long_meridians[4096]); the new tests took 0.03 to 0.25 s each,
but for the first test of the process, test_miz_sin_default_options[65], at 1.91 s: it ran first and so loaded the
library and initialised the device, once for the process (the same test with one step per launch took 0.12 s).
"""
import functools

import numpy as np
import pytest

from support import MIZ_PROG as PROG, all_fields, is_miz, midyear_state
from test_gpu_equilibrate import Setup, check_against_reference, distances, expected, reference

pytestmark = pytest.mark.gpu

NLAT, NT, MAX_YEARS, TOL_YEAR = 16, 200, 6, 5

# ---- member types ------------------------------------------------------------------------------------------------------
E2, E3, E4, E5, NEVER, ICE, NAN = range(7)
TYPE_NAMES = ("E2", "E3", "E4", "E5", "NEVER", "ICE", "NAN")
# start ("open": open water of `temp` degrees; "ice": the golden mid-year state; "nan"), temp, forcing offset, D factor,
# years of spin-up, and what the reference must give: (equilibrium year, converged)
_LADDER = [("open", 30.0, 50.0, 1.0, 3, (2, True)),        # E2
           ("open", 30.0, 50.0, 1.0, 2, (3, True)),        # E3
           ("open", 30.0, 50.0, 1.0, 1, (4, True)),        # E4
           ("open", 30.0, 50.0, 1.0, 0, (5, True)),        # E5: the tolerance is its distance of year TOL_YEAR
           ("open", 10.0, 55.0, 1.2, 0, (MAX_YEARS, False))]   # NEVER
_NANCOL = ("nan", 0.0, 0.0, 1.0, 0, (MAX_YEARS, False))
TYPES = {
    "MIZ": _LADDER + [("ice", 0.0, 6.0, 1.0, 0, (MAX_YEARS, False)), _NANCOL],
    "Classic": _LADDER + [("ice", 0.0, 6.0, 1.2, 0, (5, True)), _NANCOL],
}


def nominal_years(model):
    return np.array([t[5][0] for t in TYPES["MIZ" if is_miz(model) else "Classic"]])


# ---- patterns: column index -> type --------------------------------------------------------------------------------------
# Rows, applied in order over a seeded random fill of the six non-NaN types:
#   ("fill", seed)                       the remainder
#   ("wave", w, kind, type)              the 64 columns of wave w of the first compaction (the list is the identity then):
#                                        "empty" all E2 (ballot 0); "lane0" / "lane63" only that lane survives, as `type`, the
#                                        others E2; "all_but63" lane 63 is E2, the others survive as drawn; "all" every E2
#                                        drawn in the wave becomes `type`
#   ("range", first, stop, type)         columns first .. stop-1
WAVES_OF_ROUND_0 = [("wave", 0, "empty", None), ("wave", 1, "lane0", E3), ("wave", 2, "lane63", E4),
                    ("wave", 3, "all_but63", None), ("wave", 4, "all", E5), ("wave", 5, "empty", None),
                    ("wave", 9, "lane0", NEVER), ("wave", 12, "all_but63", None)]
PATTERNS = {
    # two waves, the second a single lane that survives; lane 63 of the first does not
    "65": (65, [("fill", 65), ("wave", 0, "all_but63", None), ("range", 64, 65, E5), ("range", 17, 18, NAN)]),
    # the single lane of the second wave freezes at once (a wave in which nothing survives); lane 63 of the first stays
    "65_tail_dies": (65, [("fill", 66), ("range", 63, 64, NEVER), ("range", 64, 65, E2), ("range", 40, 41, NAN)]),
    # exactly one full round, 16 full waves
    "1024": (1024, [("fill", 1024)] + WAVES_OF_ROUND_0 + [("range", 1023, 1024, NEVER), ("range", 700, 701, NAN)]),
    # one entry in the second round, of another type than column 1023
    "1025": (1025, [("fill", 1025)] + WAVES_OF_ROUND_0 + [("range", 1023, 1024, NEVER), ("range", 1024, 1025, E5),
                                                           ("range", 700, 701, NAN)]),
    # three rounds, the last one short; the whole second round freezes in year 2 between live columns on both sides
    "2100": (2100, [("fill", 2100)] + WAVES_OF_ROUND_0 + [("range", 1023, 1024, NEVER), ("range", 1024, 2048, E2),
                                                           ("range", 2048, 2049, E3), ("range", 2099, 2100, E4),
                                                           ("range", 700, 701, NAN)]),
    # the tail of two launch chains: the list shrinks through 2 to 1 entry, half = 0
    "tail3": (3, [("range", 0, 1, E3), ("range", 1, 2, E4), ("range", 2, 3, NEVER)]),
    "tail2": (2, [("range", 0, 1, E5), ("range", 1, 2, E3)]),
}


def build_pattern(name):
    ncol, rows = PATTERNS[name]
    types = np.full(ncol, -1, dtype=np.int64)
    for row in rows:
        if row[0] == "fill":
            types[:] = np.random.default_rng(row[1]).integers(E2, ICE + 1, ncol)
        elif row[0] == "range":
            types[row[1]:row[2]] = row[3]
        else:
            _, w, kind, typ = row
            lanes = types[64 * w:64 * (w + 1)]                 # (a view)
            if kind == "empty":
                lanes[:] = E2
            elif kind in ("lane0", "lane63"):
                lanes[:] = E2
                lanes[0 if kind == "lane0" else 63] = typ
            elif kind == "all_but63":
                lanes[lanes == E2] = E3
                lanes[63] = E2
            else:
                lanes[lanes == E2] = typ
    assert (types >= 0).all(), name
    return types


def replay(types, years_of_type, max_years=MAX_YEARS, first_test=2):
    """The compactions ebm_equilibrate makes, in NumPy: [(year, list before, keep flags)], one per compact launch."""
    Y = np.asarray(years_of_type)[types]
    cur = np.arange(len(types))
    out = []
    for y in range(1, max_years + 1):
        if y == max_years or y < first_test:
            continue
        keep = Y[cur] > y
        out.append((y, cur, keep))
        cur = cur[keep]
        if len(cur) == 0:
            break
    return out


def launches_expected(years, nt, K, chains, max_years=MAX_YEARS):
    """counters[3] from the reference's years alone (the issue's formula)."""
    total = 0
    for y in range(1, int(years.max()) + 1):
        n = int((years >= y).sum())
        nchains = ((n // 2 > 0) + (n - n // 2 > 0)) if chains == 2 else 1
        total += -(-nt // K) * nchains
    return total


# ---- setups --------------------------------------------------------------------------------------------------------------

def criterion(model):
    """T decides.  The classic step writes T = 0 where E is NaN (its branches are products with comparisons, which a NaN
    fails), so there the criterion also names E, under a tolerance no finite distance exceeds: only its NaN counts."""
    return ("T",) if is_miz(model) else ("T", "E")


def type_table(model):
    return TYPES["MIZ" if is_miz(model) else "Classic"]


def unspun_state(pkg, model, st, table):
    """One column per type: whole cells of the nearest golden cell (support.midyear_state explains why not np.interp field
    by field), open water, or NaN."""
    gold = midyear_state(model, st, 1)
    cw = pkg.default_parameters("MIZ" if is_miz(model) else "Classic")["cw"]
    state = {k: np.zeros((len(table), st.nx)) for k in gold}
    for t, (start, temp, *_rest) in enumerate(table):
        for k in state:
            if start == "ice":
                state[k][t] = gold[k][0]
            elif start == "nan":
                state[k][t] = np.nan
            elif k == ("Ew" if is_miz(model) else "E"):
                state[k][t] = cw * temp
            elif k == "Tg":
                state[k][t] = temp
    return state


class ListSetup(Setup):
    """Setup (tests/test_gpu_equilibrate.py) whose columns are members of the types of `types` [ncol]."""

    def __init__(self, pkg, model, grid, types, **opt):
        table = type_table(model)
        self.pkg, self.model, self.opt = pkg, model, opt
        self.types = np.asarray(types)
        self.ncol = len(self.types)
        self.st = pkg.SpaceTime(grid, NLAT, NT, 1)
        self.f_year, self.clock0 = None, 0
        rows, fcol, state = type_members(pkg, model, grid)
        self.rows, self.fcol = rows[self.types], fcol[self.types]
        self.state = {k: v[self.types] for k, v in state.items()}
        assert len(table) == len(rows)


@functools.lru_cache(maxsize=None)
def type_members(pkg, model, grid):
    """(parameter rows, forcing offsets, start state) of one column per type, each spun up its own number of years by plain
    ebm_run_fused on a handle of the default options."""
    table = type_table(model)
    one = Setup.__new__(ListSetup)
    one.pkg, one.model, one.opt, one.ncol = pkg, model, {}, len(table)
    one.st = pkg.SpaceTime(grid, NLAT, NT, 1)
    one.f_year, one.clock0 = None, 0
    base = pkg.engine.param_vector(pkg.default_parameters("MIZ" if is_miz(model) else "Classic"), pkg.default_parval)
    one.rows = np.tile(base, (len(table), 1))
    one.rows[:, pkg.engine.PARAM_ORDER.index("D")] *= np.array([t[3] for t in table])
    one.fcol = np.array([t[2] for t in table])
    one.state = unspun_state(pkg, model, one.st, table)
    spin = np.array([t[4] for t in table])
    state = {k: v.copy() for k, v in one.state.items()}
    with one.engine() as eng:
        for s in range(1, int(spin.max()) + 1):
            eng.run((s - 1) * NT, NT, None, True, 64)
            after = eng.get_state(one.prognostic())
            for k in state:
                state[k][spin == s] = after[k][spin == s]
    return one.rows, one.fcol, state


def solves_of_types(setup):
    """nit[type, y]: Newton iterations the MIZ step kernels count for one member of the type in its y-th year, from a
    one-column handle of the setup's options stepped by plain ebm_run_fused."""
    ntypes = len(type_table(setup.model))
    nit = np.zeros((ntypes, MAX_YEARS + 1), dtype=np.int64)
    for t in sorted(set(setup.types.tolist())):
        c = int(np.flatnonzero(setup.types == t)[0])
        with setup.engine(slice(c, c + 1)) as eng:
            eng.reset_counters()
            done = 0
            for y in range(1, MAX_YEARS + 1):
                eng.run((y - 1) * NT, NT, None, True, 64)
                now = eng.counters()["solves"]
                nit[t, y], done = now - done, now
    return nit


def run_case(pkg, model, grid, pattern, **opt):
    """Reference, honesty of the data (from the reference alone), ebm_equilibrate against it, the two counters."""
    types = build_pattern(pattern)
    setup = ListSetup(pkg, model, grid, types, **opt)
    snaps = reference(setup, MAX_YEARS)
    names = criterion(model)
    d = distances(snaps, names)
    present = sorted(set(types.tolist()))
    rep = {t: int(np.flatnonzero(types == t)[0]) for t in present}
    assert E5 in rep or pattern.startswith("tail"), pattern
    # the tolerance: the unspun ladder type's own distance of year TOL_YEAR, so that `<=` against `<` decides its columns
    tol = np.array([d[0, TOL_YEAR, rep[E5]] if E5 in rep else tolerance_of_ladder(pkg, model, grid)] + [1e300] * (len(names) - 1))
    assert np.isfinite(tol).all() and tol[0] > 0.0, tol
    years, conv, _ = expected(d, tol, MAX_YEARS, 2)
    # ---- honesty, on reference data only ----
    table = type_table(setup.model)
    report = "distances [year 2 ..][type]:\n" + "\n".join(
        f"{TYPE_NAMES[t]:6s} {np.array2string(d[0, 2:, rep[t]], precision=4)}" for t in present) + f"\ntol {tol}"
    for t in present:
        cols = types == t
        assert (years[cols] == table[t][5][0]).all() and (conv[cols] == table[t][5][1]).all(), \
            f"type {TYPE_NAMES[t]}: the reference gives year {set(years[cols].tolist())}, converged " \
            f"{set(conv[cols].tolist())}, not {table[t][5]}\n{report}"
    live = types != NAN
    prognostic = PROG if is_miz(model) else ("E", "Tg")
    for y in range(1, MAX_YEARS + 1):
        for k in prognostic + ("T",):
            assert np.isfinite(snaps[k][y][live]).all(), f"{k} of a non-NaN member is not finite after year {y}: the " \
                                                         f"comparison would be of NaNs"
        for k in prognostic:
            assert np.isnan(snaps[k][y][~live]).all(), f"{k} of the NaN column after year {y}"
        assert any(np.isnan(snaps[k][y][~live]).all() for k in names), f"no criterion field of the NaN column is NaN after year {y}"
    if not pattern.startswith("tail"):
        assert (~live).sum() == 1, "one all-NaN column"
        early = sorted(set(years[conv & (years < MAX_YEARS)].tolist()))
        assert len(early) >= 3, f"fewer than three distinct equilibrium years below max_years: {early}\n{report}"
        assert (live & ~conv).any(), f"no finite member runs to max_years unconverged\n{report}"
    for t in present:
        if table[t][5][1] and table[t][5][0] < MAX_YEARS:
            c, y = rep[t], table[t][5][0]
            assert any(not np.array_equal(snaps[k][MAX_YEARS][c], snaps[k][y][c]) for k in all_fields(model)), \
                f"type {TYPE_NAMES[t]} would not have moved on after year {y}: a build that keeps stepping it would pass"
    strict = expected(d, tol, MAX_YEARS, 2, strict=True)[0]
    assert E5 not in rep or (strict[types == E5] != years[types == E5]).all(), "`<=` against `<` decides no column"
    # ---- the code under test ----
    got, _, _ = check_against_reference(setup, names, MAX_YEARS, snaps=snaps, tol=tol)
    K = opt.get("integrate_steps_per_launch", 64)
    want_launches = launches_expected(years, NT, K, opt.get("launch_chains", 1))
    print(f"{pattern} {model} {opt}: launches {got['counters']['launches']} (reference {want_launches}), solves "
          f"{got['counters']['solves']}, tol {tol[0]!r}")
    assert got["counters"]["launches"] == want_launches, (got["counters"], want_launches)
    if is_miz(model):
        nit = solves_of_types(setup)
        want_solves = int(sum(nit[t, 1:years[c] + 1].sum() for c, t in enumerate(types)))
        print(f"    solves per type and year:\n{nit[:, 1:]}\n    reference {want_solves}")
        assert nit[[t for t in present if t != NAN], 1:].min() > 0, "a type whose steps count no iteration"
        assert got["counters"]["solves"] == want_solves, (got["counters"], want_solves)
    else:
        assert got["counters"]["solves"] == 0        # classic_step_kernel does not count its solve
    return got, years, setup


@functools.lru_cache(maxsize=None)
def tolerance_of_ladder(pkg, model, grid):
    """For a pattern without the unspun ladder type: the same tolerance, from a reference run of that type alone."""
    setup = ListSetup(pkg, model, grid, [E5])
    return distances(reference(setup, TOL_YEAR), ("T",))[0, TOL_YEAR, 0]


# ---- 1, 2: lists past one wave and one round -------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", ["65", "1024", "1025", "2100"])
def test_miz_sin_default_options(pkg, pattern):
    """fused_state_in_lds = -1 picks the step kernel from ncol: both fused kernels run over an active list."""
    run_case(pkg, "MIZ", "sin", pattern)


@pytest.mark.parametrize("pattern", ["1025", "2100"])
def test_miz_identity_two_chains(pkg, pattern):
    run_case(pkg, "MIZ", "identity", pattern, launch_chains=2, use_graph=False, cells_per_thread=2)


def test_classic_1025(pkg):
    run_case(pkg, "Classic", "identity", "1025")


def test_imex_65(pkg):
    run_case(pkg, "MIZ_IMEX", "sin", "65_tail_dies")


def test_one_step_per_launch_65(pkg):
    run_case(pkg, "MIZ", "sin", "65", integrate_steps_per_launch=1)


@pytest.mark.parametrize("pattern", ["tail3", "tail2"])
def test_two_chains_down_to_one_column(pkg, pattern):
    """half = nactive / 2 = 0: the first chain is skipped, the second steps the list's only entry."""
    types = build_pattern(pattern)
    Y = nominal_years("MIZ")[types]
    nactive = [int((Y >= y).sum()) for y in range(1, int(Y.max()) + 1)]
    assert 2 in nactive and 1 in nactive and nactive[0] == len(types), nactive
    got, years, _ = run_case(pkg, "MIZ", "identity", pattern, launch_chains=2, use_graph=False)
    # and from the reference: it does pass through exactly one active column for at least one year, and through two
    ref_active = [int((years >= y).sum()) for y in range(1, int(years.max()) + 1)]
    assert ref_active == nactive and ref_active.count(1) >= 1, ref_active


# ---- 3: NaN sentinels in some cells only ------------------------------------------------------------------------------------

SENTINEL_YEARS = 4


@functools.lru_cache(maxsize=None)
def sentinel_reference(pkg):
    setup = Setup(pkg, "MIZ", "sin", 180, 2000, 12)
    return setup, reference(setup, SENTINEL_YEARS)


@pytest.mark.parametrize("names", [("Ti",), ("Tw",), ("T", "Ti")], ids=["Ti", "Tw", "T-Ti"])
def test_partial_nan_criteria(pkg, names):
    """Ti and Tw hold NaN where there is no ice / no open water: in some cells of a column only, and (180 latitudes, 256
    threads) in waves 1 and 2 of the check kernel.  The tolerances are huge, so nothing but a NaN keeps a column from
    converging in year 2: a max_nan that drops the NaN of one lane or one wave converges the column."""
    setup, snaps = sentinel_reference(pkg)
    tol = np.full(len(names), 1e9)
    d = distances(snaps, names)
    want_y, want_c, want_r = expected(d, tol, SENTINEL_YEARS, 2)
    sentinel = [k for k in names if k in ("Ti", "Tw")]
    for k in sentinel:
        # compared year ends: 1 .. SENTINEL_YEARS
        masks = np.array([np.isnan(snaps[k][y]) for y in range(1, SENTINEL_YEARS + 1)])      # [year, col, lat]
        partial = masks.any(axis=2) & ~masks.all(axis=2)
        cols = np.flatnonzero(partial.all(axis=0))
        assert len(cols), f"no column holds NaN in some but not all cells of {k} at every compared year end"
        assert masks[:, cols, 64:].any(), f"{k}: no NaN cell with index >= 64 (waves 1 to 3 of the check kernel)"
        if k == "Tw":            # (CPU oracle: from the second year end on, Tw is NaN in cells 61 ... 179 only)
            assert (masks[:, :, 64:].any(axis=2) & ~masks[:, :, :64].any(axis=2)).any(), "no column with NaN in waves 1-3 only"
        bad = masks[1:].any(axis=(0, 2)) | masks[:-1].any(axis=(0, 2))
        assert (want_y[bad] == SENTINEL_YEARS).all() and not want_c[bad].any()
        assert np.isnan(want_r[names.index(k)][bad]).all()
    for k in names:
        if k not in sentinel:
            assert np.isfinite(want_r[names.index(k)]).all(), k
    clean = np.isfinite(d[:, 2:]).all(axis=(0, 1))
    assert (want_y[clean] == 2).all() and want_c[clean].all()      # (a NaN-free column converges at once under 1e9)
    got, _, _ = check_against_reference(setup, names, SENTINEL_YEARS, snaps=snaps, tol=tol)
    has_nan = ~clean
    assert (got["years"][has_nan] == SENTINEL_YEARS).all() and not got["converged"][has_nan].any()
    for k in sentinel:
        assert np.isnan(got["resid"][k][has_nan]).all(), k
