"""GPU tests (-m gpu) of ebm_update_columns / ebm_update_columns_device (include/ebm_hip.h): every member moved by a gain
applied to its own innovation, on the fp64 matrix instruction.

Two oracles (tests/update_columns_ref.py).  EXACT: small-integer fields, gains, targets and perturbations make every product
and every partial sum an integer far below 2^53, so the result is the int64 restatement BIT FOR BIT whatever the order inside
the instruction — this is what catches an indexing, tiling, operand-layout, tail or aliasing error.  BOUND: real model state
with a real Kalman gain against the np.longdouble restatement and the header's bound n_obs 2^-53 sum|d g| (1 + 2^-4), plus the
one rounding of x + acc.

Shapes: one past each tile edge of the kernel as written (csrc/ebm_update.hip: 16 x 16 instruction tiles, 32 x 32 per wave,
64 members x 64 stored cells per workgroup, 16 observation cells per LDS chunk, 4 per instruction).  Latitudes 2 (below one
instruction tile, a j-tail of 2), 17 (one past it, odd, a j-tail of 1, one past a chunk), 65 (one past a 64-cell tile), 130
(more than two tiles, a j-tail of 2), 180 (the reference's).  Columns 1, 3, 5, 17 (one past an instruction tile), 65 (one past
the 64-member tile), 130 (more than two member tiles).  Crafted data is loaded with ebm_set_field, so those rows are natural;
the pair-split layout is what one-step launches leave behind, tested from real steps at 180 and at 513 latitudes."""
import ctypes

import numpy as np
import pytest
import torch

from support import MIZ_PROG, all_fields, assert_same_snapshot, forcing_of, make_engine, same_bits, snapshot
from test_gpu_ensemble_sums import blank_engine, load
from update_columns_ref import clamp, innovations, update_bound, update_exact, update_ref

pytestmark = pytest.mark.gpu

DP = ctypes.POINTER(ctypes.c_double)
NLATS = (2, 17, 65, 130, 180)
NCOLS = (1, 3, 5, 17, 65, 130)


def integer_case(nfields, ncol, nlat, seed, even_obs=False):
    """fields [nfields, ncol, nlat] of integers |x| <= 2^10, an observed field of integers (even ones on request) with NaN in
    some cells, gains [nfields, nlat, nlat] of integers |g| <= 8 with zeros, an integer target with NaN in some cells, and an
    integer perturbation [ncol, nlat]."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1024, 1025, (nfields, ncol, nlat)).astype(np.float64)
    xo = rng.integers(-512, 513, (ncol, nlat)).astype(np.float64) * (2.0 if even_obs else 1.0)
    xo[rng.random(xo.shape) < 0.1] = np.nan
    g = rng.integers(-8, 9, (nfields, nlat, nlat)).astype(np.float64)
    y = rng.integers(-1024, 1025, nlat).astype(np.float64)
    y[rng.random(nlat) < 0.2] = np.nan
    e = rng.integers(-16, 17, (ncol, nlat)).astype(np.float64)
    return x, xo, g, y, e


def expected(x, xo, g, y, scale, e=None, bounds=None):
    d = innovations(xo, y, scale, e)
    return np.stack([update_exact(x[v], d, g[v], *(bounds[v] if bounds else (None, None))) for v in range(x.shape[0])])


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlat", NLATS)
def test_integer_data_bit_for_bit(pkg, nlat, ncol):
    x, xo, g, y, e = integer_case(5, ncol, nlat, 1000 * nlat + ncol)
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, MIZ_PROG + ("T",), np.concatenate([x, xo[None]]))
        eng.update_columns(MIZ_PROG, "T", g, y, 1.0)
        got = np.stack([eng.get_field(n) for n in MIZ_PROG])
        assert same_bits(got, expected(x, xo, g, y, 1.0)), "five fields, a diagnostic obs_field, scale 1"
        # one field, scale 2, from the state the first call left (T is stale now: set it again)
        eng.set_field("T", xo)
        eng.update_columns(("h",), "T", g[2], y, 2.0)
        assert same_bits(eng.get_field("h"), expected(got[2:3], xo, g[2:3], y, 2.0)[0]), "one field, scale 2"
        assert same_bits(eng.get_field("Ei"), got[0]), "the fields that were not listed are untouched"
    x, xo, g, y, e = integer_case(2, ncol, nlat, 77 * nlat + ncol, even_obs=True)
    with blank_engine(pkg, "MIZ", nlat, ncol, 2) as eng:             # two cells per thread: the other launch geometry
        load(eng, ("D", "Ew", "T"), np.concatenate([x, xo[None]]))
        eng.update_columns(("D", "Ew"), "T", g, y, 0.5)
        assert same_bits(np.stack([eng.get_field(n) for n in ("D", "Ew")]), expected(x, xo, g, y, 0.5)), "scale 1/2, even obs"


def test_classic_model(pkg):
    ncol, nlat = 65, 65
    x, xo, g, y, e = integer_case(2, ncol, nlat, 5)
    with blank_engine(pkg, "Classic", nlat, ncol) as eng:
        load(eng, ("E", "Tg", "T"), np.concatenate([x, xo[None]]))
        eng.update_columns(("E", "Tg"), "T", g, y, 1.0)
        assert same_bits(np.stack([eng.get_field(n) for n in ("E", "Tg")]), expected(x, xo, g, y, 1.0))
        with pytest.raises(ValueError):
            eng.update_columns(("T",), "T", g[0], y)                  # diagnostic: not a field to update
        with pytest.raises(ValueError):
            eng.update_columns(("Ei",), "T", g[0], y)


def test_obs_field_among_the_updated_fields(pkg):
    """130 columns x 130 latitudes: nine workgroups per field write rows that other workgroups' innovations come from.  The
    result is the restatement's, which uses the entry state."""
    ncol = nlat = 130
    x, _, g, y, e = integer_case(5, ncol, nlat, 9)
    for obs in ("Ei", "phi"):
        with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
            load(eng, MIZ_PROG, x)
            eng.update_columns(MIZ_PROG, obs, g, y, 1.0)
            got = np.stack([eng.get_field(n) for n in MIZ_PROG])
        want = expected(x, x[MIZ_PROG.index(obs)], g, y, 1.0)
        assert same_bits(got, want), obs
        assert not same_bits(got[MIZ_PROG.index(obs)], x[MIZ_PROG.index(obs)]), "honesty: the observed field moved"


def test_masks_and_zero_gain(pkg):
    ncol, nlat = 17, 65
    x, xo, g, y, e = integer_case(2, ncol, nlat, 21)
    x[0, 3, 5] = -0.0
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, ("Ei", "h", "T"), np.concatenate([x, xo[None]]))
        eng.update_columns(("Ei", "h"), "T", np.zeros_like(g), y, 1.0)
        got = np.stack([eng.get_field(n) for n in ("Ei", "h")])
        assert same_bits(got, x + 0.0) and not same_bits(got, x), "a zero gain: x + 0.0, which turns -0.0 into +0.0"
        # an all-NaN target is no observation anywhere: the same
        eng.set_field("T", xo)
        eng.update_columns(("Ei", "h"), "T", g, np.full(nlat, np.nan), 1.0)
        assert same_bits(np.stack([eng.get_field(n) for n in ("Ei", "h")]), x + 0.0)
    assert np.isnan(y).any() and np.isnan(xo).any(), "honesty: test_integer_data_bit_for_bit has both masks"


def test_sentinels_of_real_steps_contribute_nothing(pkg):
    """Ti and Tw as real steps leave them, NaN where there is no ice / no water: those cells give d = +0.0."""
    ncol, nlat = 33, 180
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4)
    first = st.nt // 2
    rng = np.random.default_rng(3)
    g = rng.integers(-8, 9, (1, nlat, nlat)).astype(np.float64)
    y = rng.integers(-4, 5, nlat).astype(np.float64)
    with eng:
        eng.run(first, 2, forcing_of(first, 2), True, 1)
        x, sentinels = eng.get_field("Ew"), {obs: eng.get_field(obs) for obs in ("Ti", "Tw")}
        for obs, xo in sentinels.items():
            assert np.isnan(xo).any() and not np.isnan(xo).all(), obs
            if obs == "Tw":                                           # Ti is read as the steps left it; then Ew goes back and
                eng.set_field("Ew", x)                                #  Tw, stale by now, is stated again: the steps' values
                eng.set_field("Tw", xo)
            eng.update_columns(("Ew",), obs, g, y, 1.0)
            acc, T, n = update_ref(innovations(xo, y, 1.0), g[0])
            got = eng.get_field("Ew")
            assert np.isfinite(got).all() and (np.abs(got - (x + acc)) <= update_bound(T, n) + 2.0 ** -53 * np.abs(np.asarray(x + acc, dtype=np.float64))).all(), obs
            assert not same_bits(got, x)


def test_bounds(pkg):
    ncol, nlat = 17, 65
    x, xo, g, y, e = integer_case(2, ncol, nlat, 31)
    x[1, 2, 7] = np.nan                                               # a NaN cell set by ebm_set_field stays NaN
    free = expected(x, xo, g, y, 1.0)
    bounds = [(-500.0, 300.0), (0.0, 0.0)]
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, ("Ew", "D", "T"), np.concatenate([x, xo[None]]))
        eng.update_columns(("Ew", "D"), "T", g, y, 1.0, None, {"Ew": bounds[0], "D": bounds[1]})
        got = np.stack([eng.get_field(n) for n in ("Ew", "D")])
        assert same_bits(got, expected(x, xo, g, y, 1.0, None, bounds))
        assert (got[0] == -500.0).any() and (got[0] == 300.0).any() and ((got[0] > -500.0) & (got[0] < 300.0)).any(), "both sides clamp"
        assert np.isnan(got[1, 2, 7]) and np.isnan(free[1, 2, 7]) and (np.delete(got[1].ravel(), 2 * nlat + 7) == 0.0).all()
        load(eng, ("Ew", "D", "T"), np.concatenate([x, xo[None]]))
        eng.update_columns(("Ew", "D"), "T", g, y, 1.0, None, {"Ew": (-np.inf, np.inf), "D": (None, np.inf)})
        assert same_bits(np.stack([eng.get_field(n) for n in ("Ew", "D")]), free), "infinite bounds: the bits of the unbounded call"
    # strictness shows in the sign of a zero: x + acc = +0.0 is not < -0.0 and not > -0.0, so it stays +0.0 under lo = hi = -0.0
    zeros = np.zeros((1, ncol, nlat))
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, ("h", "T"), np.concatenate([zeros, xo[None]]))
        eng.update_columns(("h",), "T", np.zeros((1, nlat, nlat)), y, 1.0, None, {"h": (-0.0, -0.0)})
        assert same_bits(eng.get_field("h"), zeros[0]), "+0.0 stays +0.0: neither comparison holds"
    assert same_bits(clamp(np.array([-0.0, 0.0, np.nan, 1.0]), 0.0, 0.0), np.array([-0.0, 0.0, np.nan, 0.0])), "strict: -0.0 is not < 0.0"


def test_perturbation_and_device_gain(pkg):
    ncol, nlat = 65, 130
    x, xo, g, y, e = integer_case(5, ncol, nlat, 41)
    want = expected(x, xo, g, y, 1.0, e)
    assert not same_bits(want, expected(x, xo, g, y, 1.0)), "honesty: the perturbation matters"
    et = torch.from_numpy(e).cuda()
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, MIZ_PROG + ("T",), np.concatenate([x, xo[None]]))
        eng.update_columns(MIZ_PROG, "T", g, y, 1.0, et)
        host = np.stack([eng.get_field(n) for n in MIZ_PROG])
        assert same_bits(host, want), "integer perturbation: exact"
        load(eng, MIZ_PROG + ("T",), np.concatenate([x, xo[None]]))
        eng.update_columns(MIZ_PROG, "T", torch.from_numpy(g).cuda(), y, 1.0, et)
        assert same_bits(np.stack([eng.get_field(n) for n in MIZ_PROG]), host), "the _device variant gives the host variant's bits"
        load(eng, MIZ_PROG + ("T",), np.concatenate([x, xo[None]]))
        eng.update_columns(MIZ_PROG, "T", g, y, 1.0, et)
        assert same_bits(np.stack([eng.get_field(n) for n in MIZ_PROG]), host), "the same call on reloaded data, the same bits"


def real_gain(eng, names, obs, nlat, ncol, obs_var=0.25):
    """A Kalman gain from the handle's own covariances: G_f = P_fo (P_oo + R)^-1 (NaN sentinels contribute nothing)."""
    s = eng.ensemble_sums(names + (obs,))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(s[:, 0] > 0, s[:, 1] / s[:, 0], 0.0)
    P_oo = eng.ensemble_covariance(obs, obs, None, mean[-1], mean[-1]) / (ncol - 1)
    S = P_oo + obs_var * np.eye(nlat)
    return np.stack([np.linalg.solve(S, (eng.ensemble_covariance(n, obs, None, mean[i], mean[-1]) / (ncol - 1)).T).T
                     for i, n in enumerate(names)]), mean[-1]


@pytest.mark.parametrize("nlat, ncol", [(180, 70), (513, 37)])
def test_layout_and_bound_after_real_steps(pkg, nlat, ncol):
    """After real one-launch-per-step steps at four cells per thread the prognostic rows and T lie pair-split.  The update takes
    them where they lie (ebm_state_conversions unchanged) and gives the bits of the same update applied to a second handle
    loaded by get_field / set_field (natural rows), and to one at two cells per thread; every cell is within the header's
    bound of the longdouble restatement.  513 latitudes: pitch 768, several natural spans per half of a split row, padding
    tiles."""
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    twin, _ = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    first = st.nt // 2
    bounds = {"Ei": (None, 0.0), "Ew": (0.0, None), "h": (0.0, None), "phi": (0.0, 1.0)}
    with eng, twin:
        assert eng.launch_info()["cells_per_thread"] == 4
        for e_ in (eng, twin):
            e_.run(first, 3, forcing_of(first, 3), True, 1)
        entry = {n: twin.get_field(n) for n in MIZ_PROG + ("T",)}     # the twin's rows: converted to natural by this read
        G, mean_T = real_gain(twin, MIZ_PROG, "T", nlat, ncol)
        assert np.isfinite(G).all() and np.abs(G).max() > 0.0
        y = mean_T + np.random.default_rng(nlat).normal(0.0, 0.5, nlat)
        y[::7] = np.nan
        conv, counters, noise = eng.state_conversions(), eng.counters(), eng.noise_state()
        eng.update_columns(MIZ_PROG, "T", G, y - 0.5 * mean_T, 0.5, None, bounds)
        assert eng.state_conversions() == conv, "no field is converted"
        assert eng.counters() == counters and same_bits(eng.noise_state(), noise)
        got = {n: eng.get_field(n) for n in MIZ_PROG}
        assert eng.state_conversions() == conv + 1, "honesty: the state lay pair-split"
        assert len({row.tobytes() for row in entry["T"]}) == ncol, "honesty: the members differ"
    d = innovations(entry["T"], y - 0.5 * mean_T, 0.5)
    worst, moved = 0.0, 0
    for v, n in enumerate(MIZ_PROG):
        acc, T, nobs = update_ref(d, G[v])
        exact = entry[n].astype(np.longdouble) + acc
        # the accumulator's bound, and the add's one rounding, 2^-53 |x + acc|; its factor 1 + 2^-10 is the reference's own
        # rounding: `exact` is a 64-bit-mantissa sum, off by up to 2^-64 |exact| = 2^-11 of the add's term
        bound = update_bound(T, nobs) + 2.0 ** -53 * np.abs(exact).astype(np.float64) * (1.0 + 2.0 ** -10)
        lo, hi = bounds.get(n, (None, None))
        lo, hi = (-np.inf if lo is None else lo), (np.inf if hi is None else hi)
        want = clamp(exact, lo, hi)
        inside = want == exact                                        # a clamped cell holds the bound itself
        err = np.abs(got[n] - want).astype(np.float64)
        assert (err[inside] <= bound[inside]).all(), (n, float(np.max(err - bound)))
        assert ((got[n][~inside] == lo) | (got[n][~inside] == hi) | (err[~inside] <= bound[~inside])).all(), n
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.max(np.where(inside & (bound > 0.0), err / bound, 0.0))))
        if np.abs(G[v]).max() > 0.0:                                  # (D is the same in every member here: no covariance, no gain)
            assert not same_bits(got[n], entry[n]), (n, "honesty: the field moved")
            moved += 1
    assert moved >= 3, "honesty: most fields co-vary with T"
    print("largest error / bound:", worst)
    for cells in (4, 2):
        with blank_engine(pkg, "MIZ", nlat, ncol, cells) as other:
            assert other.launch_info()["cells_per_thread"] == cells
            load(other, tuple(entry), np.stack(list(entry.values())))
            other.update_columns(MIZ_PROG, "T", G, y - 0.5 * mean_T, 0.5, None, bounds)
            for n in MIZ_PROG:
                assert same_bits(other.get_field(n), got[n]), (cells, n, "natural rows give the bits of the pair-split ones")


def test_bookkeeping_and_refusals(pkg):
    ncol, nlat = 33, 180
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    first = st.nt // 2
    lib, h = eng.lib, eng._h
    F = pkg.engine.FIELD
    rng = np.random.default_rng(8)
    g = rng.normal(0.0, 1e-3, (2, nlat, nlat))
    y = rng.normal(0.0, 1.0, nlat)
    ptr = lambda a: a.ctypes.data_as(DP)
    ids = (ctypes.c_int * 2)(F["Ei"], F["h"])
    twin, _ = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    with twin:                                                        # the same steps: what every field must still hold
        twin.run(first, 4, None, True, 1)
        entry = snapshot(twin, "MIZ")
    with eng:
        eng.run(first, 4, None, True, 1)                              # pair-split rows, current diagnostics
        before = (eng.counters(), {k: eng.field_step(k) for k in all_fields("MIZ")}, eng.state_conversions(), eng.noise_state())
        buf = torch.zeros(2, nlat, nlat, dtype=torch.float64, device="cuda")

        def bad(a, idx, v):
            b = a.copy()
            b[idx] = v
            return b
        twice = (ctypes.c_int * 2)(F["Ei"], F["Ei"])
        diag = (ctypes.c_int * 2)(F["Ei"], F["T"])
        keep = []                                                     # the arrays behind the pointers stay alive

        def P(a):
            keep.append(a)
            return ptr(a)
        cases = {
            "null fields": lambda: lib.ebm_update_columns(h, 2, None, F["T"], P(g), P(y), 1.0, None, None, None),
            "null gain": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], None, P(y), 1.0, None, None, None),
            "null target": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), None, 1.0, None, None, None),
            "nvars 0": lambda: lib.ebm_update_columns(h, 0, ids, F["T"], P(g), P(y), 1.0, None, None, None),
            "nvars 6": lambda: lib.ebm_update_columns(h, 6, ids, F["T"], P(g), P(y), 1.0, None, None, None),
            "diagnostic field": lambda: lib.ebm_update_columns(h, 2, diag, F["T"], P(g), P(y), 1.0, None, None, None),
            "listed twice": lambda: lib.ebm_update_columns(h, 2, twice, F["T"], P(g), P(y), 1.0, None, None, None),
            "obs T0": lambda: lib.ebm_update_columns(h, 2, ids, F["T0"], P(g), P(y), 1.0, None, None, None),
            "obs 99": lambda: lib.ebm_update_columns(h, 2, ids, 99, P(g), P(y), 1.0, None, None, None),
            "scale nan": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(y), float("nan"), None, None, None),
            "scale inf": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(y), float("inf"), None, None, None),
            "gain nan": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(bad(g, (1, 7, 5), np.nan)), P(y), 1.0, None, None, None),
            "target inf": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(bad(y, 11, np.inf)), 1.0, None, None, None),
            "lo > hi": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(y), 1.0, None, P(np.array([0.0, 1.0])), P(np.array([1.0, 0.0]))),
            "nan bound": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(y), 1.0, None, P(np.array([np.nan, 0.0])), None),
            "misaligned gain": lambda: lib.ebm_update_columns_device(h, 2, ids, F["T"], ctypes.c_void_p(buf.data_ptr() + 8), P(y), 1.0, None, None, None),
            "misaligned perturb": lambda: lib.ebm_update_columns(h, 2, ids, F["T"], P(g), P(y), 1.0, ctypes.c_void_p(buf.data_ptr() + 4), None, None),
        }
        says = {"gain nan": b"field h, k = 7, j = 5", "target inf": b"target[11]", "listed twice": b"Ei is listed twice"}
        for name, call in cases.items():
            assert call() == -1, name                                 # EBM_ERR_ARG
            msg = lib.ebm_last_error()
            assert b"ebm_update_columns" in msg and says.get(name, b"") in msg, (name, msg)
            now = (eng.counters(), {k: eng.field_step(k) for k in all_fields("MIZ")}, eng.state_conversions(), eng.noise_state())
            assert now[:3] == before[:3] and same_bits(now[3], before[3]), name
        assert lib.ebm_update_columns(None, 2, ids, F["T"], ptr(g), ptr(y), 1.0, None, None, None) == -1 and b"null handle" in lib.ebm_last_error()
        after_refusals = snapshot(eng, "MIZ")
        assert_same_snapshot(after_refusals, entry, "every field bit for bit what a handle holds that was never asked")
        assert set(after_refusals["fields"]) == set(all_fields("MIZ")), "honesty: every field was readable and compared"
        # (snapshot converted the rows; a step puts them back pair-split with current diagnostics)
        eng.run(first + 4, 1, None, True, 1)
        fields_before = {k: eng.field_step(k) for k in all_fields("MIZ")}
        eng.update_columns(("Ei", "h"), "T", g, y, 1.0)
        for k in ("T", "Ti", "n", "T0"):
            with pytest.raises(pkg.StaleFieldError) as err:
                eng.get_field(k)
            assert f"step {first + 4}" in str(err.value) and "overwritten since" in str(err.value), str(err.value)
        assert {k: eng.field_step(k)["written_step"] for k in fields_before} == {k: v["written_step"] for k, v in fields_before.items()}
        # a stale obs_field: the refusal of ebm_hemispheric_mean, with the same steps in the message, and nothing changes
        state = (eng.counters(), {k: eng.field_step(k) for k in all_fields("MIZ")}, eng.state_conversions())
        prog = {n: eng.get_field(n) for n in MIZ_PROG}
        state = (eng.counters(), {k: eng.field_step(k) for k in all_fields("MIZ")}, eng.state_conversions())
        with pytest.raises(pkg.StaleFieldError) as mine:
            eng.update_columns(("Ei", "h"), "T", g, y, 1.0)
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        assert tail(mine) == tail(theirs) and mine.value.status == -5
        assert (eng.counters(), {k: eng.field_step(k) for k in all_fields("MIZ")}, eng.state_conversions()) == state
        assert all(same_bits(eng.get_field(n), prog[n]) for n in MIZ_PROG)
    assert after_refusals["field_step"] == before[1]


def stepped_state_only(pkg, ncol, nlat, nsteps, **opt):
    """A handle after `nsteps` state-only one-launch steps at four cells per thread: the rows lie pair-split, phi is left
    underived, the zero-line flags are trusted and, with use_graph, a graph has been captured.  (eng, the next step)"""
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",), **opt)
    first = st.nt // 2
    eng.run(first, nsteps, forcing_of(first, nsteps), False, 1)
    return eng, first + nsteps


@pytest.mark.parametrize("path", ["run_1", "fused_7", "graph"])
def test_stepping_continues_as_from_a_handle_loaded_by_set_field(pkg, path):
    """After state-only steps — phi underived, flags trusted, the graph captured — the update must do to the book what
    ebm_set_field does.  Three handles take the same steps.  `a` and `donor` take the same update (the donor from natural rows
    that have been read, which gives the same bits: test_layout_and_bound_after_real_steps); `b` is loaded by
    ebm_set_field with the donor's downloaded post-update fields; then `a`, whose rows nobody has read, and `b` continue by
    ebm_run, ebm_run_fused or a graph-replaying ebm_run and must agree bit for bit in every field, the bookkeeping, the
    counters and the noise state."""
    ncol, nlat, n0, n = 9, 180, 20, 7
    opt = {"use_graph": True} if path == "graph" else {}
    rng = np.random.default_rng(2)
    g = rng.normal(0.0, 2e-3, (5, nlat, nlat))
    bounds = {"Ei": (None, 0.0), "Ew": (0.0, None), "h": (0.0, None), "D": (0.0, None), "phi": (0.0, 1.0)}
    (a, nxt), (donor, _), (b, _) = (stepped_state_only(pkg, ncol, nlat, n0, **opt) for _ in range(3))
    f = forcing_of(nxt, n)
    with a, donor, b:
        conv = a.state_conversions()
        y = np.clip(b.get_field("phi")[0] + 0.3, 0.0, 1.0)            # (this read converts b, which set_field loads anyway)
        # the donor's rows are read first: natural, phi formed and stored, so its update and its download rest on nothing that
        # `a` needs from the book — `a` takes the update as the steps left it, pair-split with phi underived
        for k in MIZ_PROG:
            donor.get_field(k)
        for e_ in (a, donor):
            e_.update_columns(MIZ_PROG, "phi", g, y, 1.0, None, bounds)
        assert a.state_conversions() == conv, "the update converts nothing"
        post = {k: donor.get_field(k) for k in MIZ_PROG}
        assert not same_bits(post["Ew"], b.get_field("Ew")) and not same_bits(post["phi"], b.get_field("phi")), "honesty: the state moved"
        for k in MIZ_PROG:
            b.set_field(k, post[k])
        for e_ in (a, b):
            e_.run(nxt, n, f, True, 7 if path == "fused_7" else 1)
        assert_same_snapshot(snapshot(a, "MIZ"), snapshot(b, "MIZ"), path)


def test_obs_phi_after_state_only_steps(pkg):
    """obs_field = phi where state-only steps have left the phi row underived: it is made current first, so the innovations
    are those of the phi a reader gets (the twin's get_field), and every field is within the bound of the restatement."""
    ncol, nlat, n0 = 33, 180, 20
    (eng, _), (twin, _) = (stepped_state_only(pkg, ncol, nlat, n0) for _ in range(2))
    rng = np.random.default_rng(4)
    g = rng.normal(0.0, 0.05, (5, nlat, nlat))
    y = rng.uniform(0.0, 1.0, nlat)
    with eng, twin:
        entry = {k: twin.get_field(k) for k in MIZ_PROG}
        assert entry["phi"].max() > 0.0 and len({r.tobytes() for r in entry["Ei"]}) > 1, "honesty: ice, and members that differ"
        conv = eng.state_conversions()
        eng.update_columns(MIZ_PROG, "phi", g, y, 1.0)
        assert eng.state_conversions() == conv
        got = {k: eng.get_field(k) for k in MIZ_PROG}
    d = innovations(entry["phi"], y, 1.0)
    for v, k in enumerate(MIZ_PROG):
        acc, T, nobs = update_ref(d, g[v])
        exact = entry[k].astype(np.longdouble) + acc
        bound = update_bound(T, nobs) + 2.0 ** -53 * np.abs(exact).astype(np.float64) * (1.0 + 2.0 ** -10)
        assert (np.abs(got[k] - exact).astype(np.float64) <= bound).all(), k
        assert not same_bits(got[k], entry[k]), k
