"""GPU tests (-m gpu) of ebm_ensemble_sums / ebm_ensemble_sums_device (include/ebm_hip.h): the weighted sums S0, S1, S2 across
the columns of a handle, per variable and latitude.

The oracle is tests/ensemble_sums_ref.py, the NumPy restatement of the definition's loop (checked on the CPU against exact
sums, tests/test_host_ensemble_sums.py); every comparison is BIT FOR BIT (same_bits: uint64 equality, NaN positions equal).

Shapes, the smallest at which the kernels can go wrong.  Columns 1, 31, 32, 33, 97: less than a block, a block less one, one
whole block, a block and one, three blocks and one (a batch of 16 hoisted loads, two, and every tail length class).
Latitudes 2, 5, 181, 1440 at four cells per thread and 181 at two: one pair, an odd tail whose last pair is half padding,
more than one 128-cell tile with an odd tail, twelve tiles (pitch 1536: padding tiles that must not be read); 4096 x 33: the
longest row, 32 tiles.  Crafted data is loaded with ebm_set_field (setting a diagnostic field makes it current), so those
rows are in the natural layout; the pair-split layout is what one-step launches leave behind, tested from real steps at 180
latitudes (pitch 256, 128 threads: both halves of the permutation, tiles that mix them).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from ensemble_sums_ref import ensemble_sums_ref, same_bits
from support import MIZ_PROG, assert_same_snapshot, forcing_of, make_engine, snapshot

pytestmark = pytest.mark.gpu

MIZ_ALL = ("Ei", "Ew", "h", "D", "phi", "Tw", "Ti", "n", "E", "T")
CRAFTED = ("Ei", "phi", "Ti", "T")                   # two prognostic and two diagnostic fields
DP = ctypes.POINTER(ctypes.c_double)


@functools.lru_cache(maxsize=None)
def grid(pkg, nlat):
    return pkg.SpaceTime("sin", nlat, 2000, 1)


def blank_engine(pkg, model, nlat, ncol, cells=4):
    st = grid(pkg, nlat)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ" if model != "Classic" else "Classic"), pkg.default_parval)
    return pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, ncol, device=0, cells_per_thread=cells)


def crafted(nvars, ncol, nlat, seed):
    """[nvars, ncol, nlat]: magnitudes over 30 binades, both signs, -0.0 and +-Inf in a few cells, NaN in some cells of some
    members; per variable one (variable, latitude) pair without any contributor, and pairs with some and with all."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 2.0, (nvars, ncol, nlat)) * 2.0 ** rng.integers(-15, 16, (nvars, ncol, nlat)) * rng.choice([-1.0, 1.0], (nvars, ncol, nlat))
    some = rng.random((nvars, ncol, nlat)) < 0.15
    some[:, ::2, :] = False                          # NaN only in the odd members ...
    some[:, :, 1::3] = False                         # ... and never at these latitudes (every member contributes there)
    x[some] = np.nan
    for v in range(nvars):
        for val in (-0.0, np.inf, -np.inf, -0.0):
            x[v, rng.integers(ncol), rng.integers(nlat)] = val
    nobody = [(v + 2 * (nlat // 3)) % nlat for v in range(nvars)]
    for v in range(nvars):
        x[v, :, nobody[v]] = np.nan                  # nobody contributes here
    if nvars >= 3:                                   # one Inf and one -0.0 that stay, whatever the draws above hit
        x[1, 0, (nobody[1] + 1) % nlat] = np.inf
        x[2, 0, (nobody[2] + 1) % nlat] = -0.0
    if ncol >= 2:
        x[0, 1, 0] = np.nan                          # some, not all: member 1 of at least two
        x[0, 0, 0] = 1.5
    if nvars * nlat >= 4:
        x[-1, :, -1] = rng.uniform(1.0, 2.0, ncol)   # all, finite
    return x


def coverage(x):
    """(none, some, all): is there a (variable, latitude) pair with no / some but not all / all members contributing?"""
    n = (~np.isnan(x)).sum(axis=1)
    return bool((n == 0).any()), bool(((n > 0) & (n < x.shape[1])).any()), bool((n == x.shape[1]).any())


def load(eng, names, x):
    prog = [n for n in names if n in eng.prognostic]
    for n in prog + [n for n in names if n not in prog]:          # a prognostic write makes the diagnostic fields stale
        eng.set_field(n, x[names.index(n)])


def weights_for(ncol, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, ncol) * rng.choice([-1.0, 1.0, 1.0], ncol)      # negative weights are legal
    w[rng.random(ncol) < 0.25] = 0.0
    if ncol > 2:
        w[2] = 0.0
    return w


SHAPES = [(ncol, nlat, 4) for ncol in (1, 31, 32, 33, 97) for nlat in (2, 5, 181, 1440)] + \
         [(ncol, 181, 2) for ncol in (1, 31, 32, 33, 97)] + [(33, 4096, 4)]


@pytest.mark.parametrize("ncol, nlat, cells", SHAPES, ids=lambda v: str(v))
def test_crafted_data_against_the_restatement(pkg, ncol, nlat, cells):
    """No weights against explicit ones (identical bits); weights with zeros and negative entries; no center against a
    center; all against the restatement."""
    x = crafted(len(CRAFTED), ncol, nlat, 1000 * ncol + nlat + cells)
    none, some, every = coverage(x)
    assert none and every and (some or ncol < 2), "honesty: the data holds the contributor patterns it claims"
    assert np.isinf(x).any() and (np.signbit(x) & (x == 0.0)).any()
    w = weights_for(ncol, nlat)
    center = np.random.default_rng(nlat).normal(0.0, 3.0, (len(CRAFTED), nlat))
    with blank_engine(pkg, "MIZ", nlat, ncol, cells) as eng:
        assert eng.launch_info()["cells_per_thread"] == cells
        load(eng, CRAFTED, x)
        plain = eng.ensemble_sums(CRAFTED)
        assert same_bits(plain, ensemble_sums_ref(x)), "unit weights"
        assert same_bits(eng.ensemble_sums(CRAFTED, np.ones(ncol)), plain), "NULL weights are ones"
        assert same_bits(eng.ensemble_sums(CRAFTED, w), ensemble_sums_ref(x, w)), "weights"
        assert same_bits(eng.ensemble_sums(CRAFTED, w, center), ensemble_sums_ref(x, w, center)), "weights and center"
        assert same_bits(eng.ensemble_sums(CRAFTED, None, center), ensemble_sums_ref(x, None, center)), "center"
        assert same_bits(eng.ensemble_sums(CRAFTED, None, np.zeros_like(center)), plain), "a zero center subtracts nothing"
        assert same_bits(eng.ensemble_sums(CRAFTED), plain), "the same call, the same bits"
        one = eng.ensemble_sums("Ti", w, center[2:3])
        assert same_bits(one, ensemble_sums_ref(x[2:3], w, center[2:3])), "one variable"
        gone = np.isnan(x).all(axis=1)
        assert (plain[:, 0][gone] == 0.0).all() and (plain[:, 1][gone] == 0.0).all() and (plain[:, 2][gone] == 0.0).all()


def test_zero_weight_hides_an_inf_cell(pkg):
    ncol, nlat = 33, 5
    rng = np.random.default_rng(5)
    x = rng.normal(0.0, 1.0, (1, ncol, nlat))
    x[0, 32, 3] = np.inf                             # the one column of the second block
    x[0, 7, 1] = -np.inf
    w = np.ones(ncol)
    w[[32, 7]] = 0.0
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        eng.set_field("T", x[0])
        plain = eng.ensemble_sums("T")
        assert plain[0, 1, 3] == np.inf and plain[0, 1, 1] == -np.inf and plain[0, 2, 1] == np.inf, "Inf is data and propagates"
        got = eng.ensemble_sums("T", w)
        assert np.isfinite(got).all(), "the member is skipped: no 0 * Inf"
        assert same_bits(got, ensemble_sums_ref(x, w)) and (got[0, 0] == ncol - 2.0).all()
        center = np.full((1, nlat), 0.25)
        assert same_bits(eng.ensemble_sums("T", None, center), ensemble_sums_ref(x, None, center))     # Inf - c, NaN from Inf sums


def test_zero_weights_select_a_sub_ensemble(pkg):
    """Weights that are 0 from column 64 on: the sums of a handle that holds the first two blocks only.  Zeros scattered
    inside the blocks: the restatement."""
    ncol, nlat = 97, 181
    x = crafted(2, ncol, nlat, 77)
    names = ("h", "T")
    w = np.ones(ncol)
    w[64:] = 0.0
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng, blank_engine(pkg, "MIZ", nlat, 64) as sub:
        load(eng, names, x)
        load(sub, names, x[:, :64])
        assert same_bits(eng.ensemble_sums(names, w), sub.ensemble_sums(names))
        w2 = weights_for(64, 3)
        assert same_bits(eng.ensemble_sums(names, np.concatenate([w2, np.zeros(33)])), sub.ensemble_sums(names, w2))
        scattered = weights_for(ncol, 9)
        assert (scattered == 0.0).sum() >= 10
        assert same_bits(eng.ensemble_sums(names, scattered), ensemble_sums_ref(x, scattered))


def test_more_blocks_than_a_batch_of_the_finish_kernel(pkg):
    """1057 columns are 34 blocks of 32: the finish kernel, which the histogram and the range share, adds 32 block partials per
    batch of loads, so this is one batch and a tail of two.  With weights: the order shows."""
    ncol, nlat = 1057, 5
    x = crafted(1, ncol, nlat, 99)
    w = weights_for(ncol, 1)
    center = np.random.default_rng(nlat).normal(0.0, 3.0, (1, nlat))
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        eng.set_field("T", x[0])
        assert same_bits(eng.ensemble_sums("T", w), ensemble_sums_ref(x, w))
        assert same_bits(eng.ensemble_sums("T", w, center), ensemble_sums_ref(x, w, center))


def test_all_variables_of_each_model(pkg):
    ncol, nlat = 33, 181
    x = crafted(10, ncol, nlat, 21)
    w = weights_for(ncol, 4)
    center = np.random.default_rng(2).normal(0.0, 1.0, (10, nlat))
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, MIZ_ALL, x)
        assert same_bits(eng.ensemble_sums(MIZ_ALL, w, center), ensemble_sums_ref(x, w, center))
        order = ("T", "Ei", "Tw")                    # the caller's order, not the enum's
        idx = [MIZ_ALL.index(n) for n in order]
        assert same_bits(eng.ensemble_sums(order, w, center[idx]), ensemble_sums_ref(x[idx], w, center[idx]))
    names = ("E", "Tg", "T", "h")
    with blank_engine(pkg, "Classic", nlat, ncol) as eng:
        load(eng, names, x[:4])
        assert same_bits(eng.ensemble_sums(names, w, center[:4]), ensemble_sums_ref(x[:4], w, center[:4]))
    with blank_engine(pkg, "MIZ_IMEX", 5, ncol) as eng:
        load(eng, MIZ_ALL, x[:, :, :5])
        assert same_bits(eng.ensemble_sums(MIZ_ALL, w), ensemble_sums_ref(x[:, :, :5], w))


def test_device_variant_equals_the_host_variant(pkg):
    ncol, nlat = 97, 181
    x = crafted(3, ncol, nlat, 31)
    names = ("Ei", "Tw", "T")
    w = weights_for(ncol, 6)
    center = np.random.default_rng(8).normal(0.0, 1.0, (3, nlat))
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, names, x)
        for ww, cc in ((None, None), (w, center)):
            buf = torch.full((3, 3, nlat), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng.ensemble_sums_device(names, buf.data_ptr(), ww, cc)
            assert same_bits(buf.cpu().numpy(), eng.ensemble_sums(names, ww, cc))
            assert same_bits(buf.cpu().numpy(), ensemble_sums_ref(x, ww, cc))


def test_moments_against_numpy_two_pass_variance(pkg):
    """EnsembleRun.moments on benign data, unit weights, against np.mean / np.var (NumPy's two-pass variance).  The bound is
    derived: both variances are sums of ncol squared deviations d^2 <= max|d|^2 divided by ncol; a sequential sum of ncol
    terms is off by at most ncol 2^-53 of the sum of their magnitudes (<= ncol max|d|^2), each d^2 carries three roundings
    (the subtraction twice through the square, the product) and NumPy's own pairwise sum less than the sequential one; the
    shift between the two means enters both S2 / S0 and (S1 / S0)^2 and cancels to second order.  Per unit of max|d|^2 that is
    (ncol + 3 + 1) 2^-53 for this library and at most as much again for NumPy: 4 ncol 2^-53 max|d|^2 for every ncol >= 2."""
    ncol, nlat = 97, 181
    st = grid(pkg, nlat)
    rng = np.random.default_rng(12)
    T = 10.0 + rng.normal(0.0, 1.0, (ncol, nlat))
    phi = rng.uniform(0.0, 1.0, (ncol, nlat))
    run = pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), {k: np.zeros((ncol, nlat)) for k in MIZ_PROG if k != "phi"} | {"phi": phi})
    try:
        run.engine.set_field("T", T)
        m = run.moments(("T", "phi"))
        for name, x in (("T", T), ("phi", phi)):
            d2 = np.max(np.abs(x - x.mean(axis=0)), axis=0) ** 2
            assert (m[name]["weight"] == ncol).all()
            # (each mean: a sum of ncol terms, off by at most ncol 2^-53 max|x| after the division)
            assert (np.abs(m[name]["mean"] - x.mean(axis=0)) <= 2 * ncol * 2.0 ** -53 * np.abs(x).max(axis=0)).all(), name
            err = np.abs(m[name]["var"] - x.var(axis=0))
            print(name, "max var error / bound:", float(np.max(err / (4 * ncol * 2.0 ** -53 * d2))))
            assert (err <= 4 * ncol * 2.0 ** -53 * d2).all(), name
        # the members above the mean at the equator only: a conditional mean by zero weights
        sel = (T[:, 0] > T[:, 0].mean()).astype(np.float64)
        m = run.moments("T", sel)
        assert (m["T"]["weight"] == sel.sum()).all()
        assert np.allclose(m["T"]["mean"], T[sel > 0].mean(axis=0), rtol=1e-14)
    finally:
        run.close()


# ---- both stored layouts, from real steps ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cells, spl, diag, names",
                         [(4, 1, True, ("Ei", "phi", "T")), (4, 1, True, MIZ_ALL), (4, 7, True, ("Ei", "phi", "T")),
                          (4, 1, False, ("phi", "Ei")), (4, 1, False, MIZ_PROG), (2, 1, True, MIZ_ALL)],
                         ids=["pair_split", "pair_split_all_ten", "natural_after_fused", "phi_underived", "underived_all_five",
                              "two_cells"])
def test_rows_are_read_where_they_lie(pkg, cells, spl, diag, names):
    """Three steps (one launch per step at four cells per thread: state and diagnostics pair-split; state-only: phi not
    stored; fused: natural), then the sums: no conversion, the bits of the restatement on the fields read back afterwards,
    the bookkeeping untouched, and the run continues as the twin's that never made the call.  Honesty: that the prognostic rows
    really lie pair-split is read off the twin, whose first ebm_get_field of a prognostic field must convert the state
    (ebm_state_conversions grows by one) exactly in the cases that claim it; the diagnostic rows are stored by the same
    launches in the same layout, for which the library has no counter."""
    ncol = 65
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, cells, ("noise",))
    twin, _ = make_engine(pkg, "MIZ", "sin", 180, ncol, cells, ("noise",))
    first = st.nt // 2
    w = weights_for(ncol, 13)
    center = np.random.default_rng(3).normal(0.0, 2.0, (len(names), 180))
    with eng, twin:
        for e in (eng, twin):
            e.run(first, 3, forcing_of(first, 3), diag, spl)
        conv, counters = eng.state_conversions(), eng.counters()
        steps = {k: eng.field_step(k) for k in MIZ_ALL}
        plain, weighted = eng.ensemble_sums(names), eng.ensemble_sums(names, w, center)
        assert eng.state_conversions() == conv, "no field is converted"
        assert eng.counters() == counters and {k: eng.field_step(k) for k in MIZ_ALL} == steps
        if not diag:
            with pytest.raises(pkg.StaleFieldError):
                eng.ensemble_sums(("phi", "T"))
        # what the twin reads back through the host (this converts the twin, not eng)
        before = twin.state_conversions()
        twin.get_field("Ei")
        assert twin.state_conversions() - before == (1 if cells == 4 and spl == 1 else 0), "honesty: the layout the case names"
        x = np.stack([twin.get_field(n) for n in names])
        assert len({row.tobytes() for row in x[0]}) == ncol, "honesty: the members differ"
        assert same_bits(plain, ensemble_sums_ref(x)) and same_bits(weighted, ensemble_sums_ref(x, w, center))
        for e in (eng, twin):
            e.run(first + 3, 4, forcing_of(first + 3, 4), True, spl)
        assert_same_snapshot(snapshot(eng, "MIZ"), snapshot(twin, "MIZ"), "the run continues as without the call")
        again = eng.ensemble_sums(names, w, center)
        assert same_bits(again, ensemble_sums_ref(np.stack([twin.get_field(n) for n in names]), w, center))


def test_a_steady_run_loop_still_converts_once(pkg):
    eng, st = make_engine(pkg, "MIZ", "sin", 180, 33, 4)
    first = st.nt // 2
    with eng:
        base = eng.state_conversions()
        for i in range(4):
            eng.run(first + 2 * i, 2, None, True, 1)
            eng.ensemble_sums(("Ei", "phi", "T"))
        assert eng.state_conversions() == base + 1


# ---- bookkeeping and refusals ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    ncol = 33
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, 4)
    first = st.nt // 2
    lib, h = eng.lib, eng._h
    with eng:
        eng.run(first, 2, None, True, 1)
        before = eng.ensemble_sums(("Ei", "T"))
        state = (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions())
        out = np.zeros((2, 3, 180))
        w, center = np.ones(ncol), np.zeros((2, 180))
        ids = lambda *names: (ctypes.c_int * len(names))(*[pkg.engine.FIELD[n] if isinstance(n, str) else n for n in names])
        op = out.ctypes.data_as(DP)

        def bad(k, v):
            a = (w if k == "w" else center).copy()
            a.flat[v[0]] = v[1]
            return a
        cases = {
            "null fields": lambda: lib.ebm_ensemble_sums(h, 2, None, None, None, op),
            "null out": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T"), None, None, None),
            "null dev_out": lambda: lib.ebm_ensemble_sums_device(h, 2, ids("Ei", "T"), None, None, None),
            "nvars 0": lambda: lib.ebm_ensemble_sums(h, 0, ids("Ei", "T"), None, None, op),
            "nvars 13": lambda: lib.ebm_ensemble_sums(h, 13, ids(*(MIZ_ALL + MIZ_ALL[:3])), None, None, op),
            "T0": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T0"), None, None, op),
            "Tg on MIZ": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "Tg"), None, None, op),
            "field 99": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", 99), None, None, op),
            "field -1": lambda: lib.ebm_ensemble_sums(h, 2, ids(-1, "Ei"), None, None, op),
            "repeated": lambda: lib.ebm_ensemble_sums(h, 2, ids("T", "T"), None, None, op),
            "w nan": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T"), bad("w", (7, np.nan)).ctypes.data_as(DP), None, op),
            "w inf": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T"), bad("w", (32, -np.inf)).ctypes.data_as(DP), None, op),
            "center nan": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T"), None, bad("c", (359, np.nan)).ctypes.data_as(DP), op),
            "center inf": lambda: lib.ebm_ensemble_sums(h, 2, ids("Ei", "T"), None, bad("c", (0, np.inf)).ctypes.data_as(DP), op),
        }
        says = {"w nan": b"w[7]", "w inf": b"w[32]", "repeated": b"twice", "nvars 13": b"nvars = 13", "center nan": b"center[1][179]"}
        for name, call in cases.items():
            assert call() == -1, name                                     # EBM_ERR_ARG
            msg = lib.ebm_last_error()
            assert b"ebm_ensemble_sums" in msg and says.get(name, b"") in msg, (name, msg)
            assert (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions()) == state, name
            assert same_bits(eng.ensemble_sums(("Ei", "T")), before), name
        # a stale T: the refusal of ebm_hemispheric_mean, with the same steps in the message
        eng.run(first + 2, 3, None, False, 1)
        with pytest.raises(pkg.StaleFieldError) as mine:
            eng.ensemble_sums(("Ei", "T"))
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        assert tail(mine) == tail(theirs) and f"step {first + 1}" in tail(mine) and f"step {first + 4}" in tail(mine)
        assert mine.value.status == -5
        assert same_bits(eng.ensemble_sums("Ei"), ensemble_sums_ref(eng.get_field("Ei")[None]))
