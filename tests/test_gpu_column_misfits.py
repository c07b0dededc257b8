"""GPU tests (-m gpu) of ebm_column_misfits / ebm_column_misfits_device (include/ebm_hip.h): per column and target, the weighted
squared distance J of the column's profiles to the target and the number N of cells behind it.

The oracle is tests/column_misfits_ref.py, the NumPy restatement of the definition's chains, parity add and tree (checked on
the CPU against exact sums, tests/test_host_column_misfits.py); every comparison is BIT FOR BIT (same_bits).

Shapes, the smallest at which the kernel can go wrong.  Latitudes at four cells per thread: 2 (one unit, 63 idle lanes), 5 (the
last pair is half padding), 127, 128, 129, 130 (lane 63's unit half and whole, the first wrap at its half unit and at its whole
unit), 181, 1440 (pitch 1536: padding units that must not be read); 181 at two cells per thread; 4096 x 3, 32 units per lane.
Columns 1, 2, 33; targets 1, 3, 8 (the kernel is instantiated per count; 3 and 8 also have the smaller load batches); 1, 4 and
all ten variables.  Crafted data is loaded with ebm_set_field, so those rows are in the natural layout; the pair-split layout
is what one-step launches leave behind, tested from real steps at 180 and 1025 latitudes."""
import ctypes

import numpy as np
import pytest
import torch

from column_misfits_ref import column_misfits_ref, same_bits
from support import MIZ_PROG, assert_same_snapshot, forcing_of, make_engine, snapshot
from test_gpu_ensemble_sums import CRAFTED, DP, MIZ_ALL, blank_engine, crafted, load

pytestmark = pytest.mark.gpu


def targets_for(ntargets, nvars, nlat, seed):
    """[ntargets, nvars, nlat] over the data's binades, NaN ("no observation") at some latitudes; of three and more targets
    the last observes nothing at all."""
    rng = np.random.default_rng(seed)
    y = rng.uniform(1.0, 2.0, (ntargets, nvars, nlat)) * 2.0 ** rng.integers(-15, 16, (ntargets, nvars, nlat)) * rng.choice([-1.0, 1.0], (ntargets, nvars, nlat))
    y[rng.random(y.shape) < 0.2] = np.nan
    y[:, :, 0] = 0.5                                     # observed by every target but the blind one
    if ntargets >= 3:
        y[-1] = np.nan
    return y


def rweights_for(x, seed):
    """dict of rw [nvars, nlat]: `weights` — positive over a few binades with zeros, and zero wherever a member holds an Inf, so
    that every J is finite; `band` — a 0 / 1 mask of the middle latitudes and the last one; `nobody` — 1 at the one cell of
    the first variable that has one where every member is NaN; `everybody` — 1 at the last cell of the last variable, where
    every member is finite."""
    nvars, ncol, nlat = x.shape
    rng = np.random.default_rng(seed)
    w = rng.uniform(1.0, 2.0, (nvars, nlat)) * 2.0 ** rng.integers(-4, 5, (nvars, nlat))
    w[rng.random(w.shape) < 0.2] = 0.0
    w[np.isinf(x).any(axis=1)] = 0.0
    w[:, 0] = np.where(np.isinf(x[:, :, 0]).any(axis=1), 0.0, 1.25)
    band = np.zeros((nvars, nlat))
    band[:, nlat // 4:max(3 * nlat // 4, 1)] = 1.0
    band[:, -1] = 1.0
    nobody = np.zeros((nvars, nlat))
    v, k = np.argwhere(np.isnan(x).all(axis=1))[0]
    nobody[v, k] = 1.0
    everybody = np.zeros((nvars, nlat))
    everybody[-1, -1] = 1.0
    return dict(weights=w, band=band, nobody=nobody, everybody=everybody)


def check_crafted(pkg, names, ncol, nlat, cells, model="MIZ"):
    """Every rw of rweights_for and none, for 1, 3 and 8 targets, against the restatement; the honesty conditions."""
    nvars = len(names)
    x = crafted(nvars, ncol, nlat, 1000 * ncol + nlat + cells + nvars)
    assert np.isinf(x).any() and (np.signbit(x) & (x == 0.0)).any() and np.isnan(x).any()
    rws = rweights_for(x, nlat + ncol)
    seen = dict(none=False, some=False, all=False, inf=False, finite=False)
    with blank_engine(pkg, model, nlat, ncol, cells) as eng:
        assert eng.launch_info()["cells_per_thread"] == cells
        load(eng, names, x)
        for ntargets in (1, 3, 8):
            y = targets_for(ntargets, nvars, nlat, 7 * nlat + ntargets)
            if nvars * nlat >= 4:
                y[0, -1, -1] = 0.75                      # the cell of `everybody` is observed by target 0
            for key, rw in [("unit", None)] + list(rws.items()):
                got = eng.column_misfits(names, y, rw)
                assert same_bits(got, column_misfits_ref(x, y, rw)), (ntargets, key)
                assert same_bits(eng.column_misfits(names, y, rw), got), "the same call, the same bits"
                J, N = got[:, 0], got[:, 1]
                cells_open = ((np.ones((nvars, nlat)) if rw is None else rw) != 0.0)[None] & ~np.isnan(y)      # [ntargets, nvars, nlat]
                candidates = cells_open.sum(axis=(1, 2))[:, None]
                assert ((N == 0.0) <= (J == 0.0)).all() and not np.signbit(J[N == 0.0]).any(), "no contributor: J = +0.0"
                seen["none"] |= bool((N == 0.0).any())
                seen["some"] |= bool(((N > 0.0) & (N < candidates)).any())
                seen["all"] |= bool(((N > 0.0) & (N == candidates)).any())
                seen["inf"] |= bool(np.isinf(J).any())
                seen["finite"] |= bool((np.isfinite(J) & (J > 0.0)).any())
                if key == "weights":
                    assert np.isfinite(J).all() and ((J > 0.0) | (N == 0.0)).all(), "rw = 0 hides every Inf cell"
                if key == "nobody":
                    assert (got == 0.0).all()
                if key == "unit" and ntargets >= 3:
                    assert (got[-1] == 0.0).all(), "the target that observes nothing"
                    one = eng.column_misfits(names, y[1], None)
                    assert one.shape == (1, 2, ncol) and same_bits(one[0], got[1]), "a single target as [nvars, nlat]"
            if ntargets == 1:
                assert same_bits(eng.column_misfits(names, y, np.ones((nvars, nlat))), eng.column_misfits(names, y)), "NULL rw is ones"
    want = dict(none=True, some=True, all=nvars * nlat >= 4, inf=True, finite=True)
    assert {k: seen[k] or not want[k] for k in seen} == dict.fromkeys(seen, True), f"honesty: the data holds the patterns it claims: {seen}"


@pytest.mark.parametrize("ncol", [1, 2, 33])
@pytest.mark.parametrize("nlat, cells", [(2, 4), (5, 4), (127, 4), (128, 4), (129, 4), (130, 4), (181, 4), (1440, 4), (181, 2)],
                         ids=lambda v: str(v))
def test_crafted_data_against_the_restatement(pkg, nlat, cells, ncol):
    check_crafted(pkg, CRAFTED, ncol, nlat, cells)


def test_the_longest_meridian(pkg):
    check_crafted(pkg, CRAFTED, 3, 4096, 4)


@pytest.mark.parametrize("nlat", [5, 181])
def test_one_variable_and_all_ten(pkg, nlat):
    check_crafted(pkg, ("T",), 33, nlat, 4)
    check_crafted(pkg, MIZ_ALL, 33, nlat, 4)


def test_the_order_of_the_variables_is_the_callers(pkg):
    """One accumulator runs across the variables in the order of the call: the same fields in another order give the
    restatement of that order, and on this data other bits."""
    ncol, nlat = 33, 181
    x = crafted(4, ncol, nlat, 5)
    x[np.isinf(x)] = 3.0
    y = targets_for(3, 4, nlat, 6)
    order = [3, 1, 0, 2]
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, CRAFTED, x)
        a = eng.column_misfits(CRAFTED, y)
        b = eng.column_misfits([CRAFTED[i] for i in order], y[:, order])
        assert same_bits(a, column_misfits_ref(x, y)) and same_bits(b, column_misfits_ref(x[order], y[:, order]))
        assert np.array_equal(a[:, 1], b[:, 1]) and not same_bits(a[:, 0], b[:, 0]), "honesty: the order shows in the bits"


def test_a_classic_handle(pkg):
    ncol, nlat = 33, 181
    names = ("E", "Tg", "T", "h")
    check_crafted(pkg, names, ncol, nlat, 4, "Classic")


# ---- both stored layouts, from real steps ---------------------------------------------------------------------------------------

def stepped(pkg, nlat, ncol, diag=True, spl=1, nsteps=3):
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    first = st.nt // 2
    eng.run(first, nsteps, forcing_of(first, nsteps), diag, spl)
    return eng, first


def targets_near(x, ntargets, seed):
    """Targets near the members' own profiles (finite where any member is), NaN at every seventh latitude."""
    rng = np.random.default_rng(seed)
    ok = np.isfinite(x)
    base = np.where(ok, x, 0.0).sum(axis=1) / np.maximum(ok.sum(axis=1), 1)      # [nvars, nlat]; 0.0 where no member is finite
    y = base[None] + rng.normal(0.0, 0.1, (ntargets,) + base.shape) * (1.0 + np.abs(base[None]))
    y[:, :, ::7] = np.nan
    return y


@pytest.mark.parametrize("nlat, ncol", [(180, 65), (1025, 5)])
@pytest.mark.parametrize("names", [("Ei", "phi", "T"), MIZ_ALL], ids=["three", "all_ten"])
def test_rows_are_read_where_they_lie(pkg, nlat, ncol, names):
    """Three one-step launches leave state and diagnostics pair-split.  The misfits: no conversion, the bits of the
    restatement on the fields that a twin downloads, the bookkeeping untouched; the same bits again after a read has forced
    the natural layout; and the run continues as the twin's that never made the call."""
    eng, first = stepped(pkg, nlat, ncol)
    twin, _ = stepped(pkg, nlat, ncol)
    with eng, twin:
        before = twin.state_conversions()
        twin.get_field("Ei")
        assert twin.state_conversions() - before == 1, "honesty: the state lies pair-split after one-step launches"
        x = np.stack([twin.get_field(n) for n in names])
        assert len({row.tobytes() for row in x[0]}) == ncol, "honesty: the members differ"
        assert np.isnan(x).any() or len(names) < 10, "honesty: the sentinels of Ti and Tw are there"
        y = targets_near(x, 3, nlat)
        rw = np.random.default_rng(nlat).uniform(0.5, 2.0, (len(names), nlat))
        rw[:, 1::5] = 0.0
        conv, counters = eng.state_conversions(), eng.counters()
        steps = {k: eng.field_step(k) for k in MIZ_ALL}
        plain, weighted = eng.column_misfits(names, y), eng.column_misfits(names, y, rw)
        assert eng.state_conversions() == conv, "no field is converted"
        assert eng.counters() == counters and {k: eng.field_step(k) for k in MIZ_ALL} == steps
        assert same_bits(plain, column_misfits_ref(x, y)) and same_bits(weighted, column_misfits_ref(x, y, rw))
        assert np.isfinite(plain).all() and (plain[:, 0] > 0.0).all() and len(set(plain[0, 0].tolist())) == ncol
        for n in names:
            eng.get_field(n)                             # forces the natural layout of state and diagnostics
        assert eng.state_conversions() == conv + 1
        assert same_bits(eng.column_misfits(names, y), plain) and same_bits(eng.column_misfits(names, y, rw), weighted), "either layout, the same bits"
        twin.get_field("T")
        for e in (eng, twin):
            e.run(first + 3, 4, forcing_of(first + 3, 4), True, 1)
        assert_same_snapshot(snapshot(eng, "MIZ"), snapshot(twin, "MIZ"), "the run continues as without the call")


@pytest.mark.parametrize("nlat, ncol", [(180, 33), (1025, 3)])
def test_stale_diagnostics_and_underived_phi(pkg, nlat, ncol):
    """State-only one-step launches: T is stale (the refusal of ebm_hemispheric_mean, the same message), phi is underived and
    is made current first, in the layout the state has."""
    eng, first = stepped(pkg, nlat, ncol, diag=False)
    twin, _ = stepped(pkg, nlat, ncol, diag=False)
    with eng, twin:
        x = np.stack([twin.get_field(n) for n in ("phi", "Ei")])
        y = targets_near(x, 2, 3)
        conv = eng.state_conversions()
        with pytest.raises(pkg.StaleFieldError) as mine:
            eng.column_misfits(("phi", "T"), np.zeros((1, 2, nlat)))
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        assert tail(mine) == tail(theirs) and mine.value.status == -5 and "ebm_column_misfits" in str(mine.value)
        got = eng.column_misfits(("phi", "Ei"), y)
        assert same_bits(got, column_misfits_ref(x, y)) and eng.state_conversions() == conv
        assert (x[0] != 0.0).any(), "honesty: there is ice, phi is not trivially zero"
        x5 = np.stack([twin.get_field(n) for n in MIZ_PROG])
        y5 = targets_near(x5, 1, 4)
        assert same_bits(eng.column_misfits(MIZ_PROG, y5), column_misfits_ref(x5, y5)) and eng.state_conversions() == conv


def test_a_steady_run_loop_still_converts_once(pkg):
    eng, st = make_engine(pkg, "MIZ", "sin", 180, 33, 4)
    first = st.nt // 2
    with eng:
        base = eng.state_conversions()
        for i in range(4):
            eng.run(first + 2 * i, 2, None, True, 1)
            eng.column_misfits(("Ei", "phi", "T"), np.zeros((2, 3, 180)))
        assert eng.state_conversions() == base + 1


# ---- identities without the restatement -----------------------------------------------------------------------------------------

def test_identities(pkg):
    """A member's own profile as the target: J = 0 exactly and N = its cells that are not NaN.  Several targets in one call:
    the separate calls.  A shift by resample_columns: the same permutation of the result.  The _device form: the host form."""
    nlat, ncol = 180, 33
    names = ("Ei", "Ti", "phi", "T")
    eng, first = stepped(pkg, nlat, ncol)
    twin, _ = stepped(pkg, nlat, ncol)
    with eng, twin:
        x = np.stack([twin.get_field(n) for n in names])           # the twin's bits are eng's; eng's rows stay pair-split
        picks = [0, 7, 32]
        y = x[:, picks].transpose(1, 0, 2).copy()        # [3, nvars, nlat]: the members' own fields, NaN sentinels included
        got = eng.column_misfits(names, y)
        for t, j in enumerate(picks):
            assert got[t, 0, j] == 0.0 and got[t, 1, j] == float((~np.isnan(x[:, j])).sum())
            others = np.delete(np.arange(ncol), j)
            assert (got[t, 0, others] > 0.0).all()
        assert np.isnan(x).any() and (got[:, 1] < len(names) * nlat).all(), "honesty: the sentinels are there"
        for t in range(3):
            assert same_bits(eng.column_misfits(names, y[t:t + 1])[0], got[t]), "ntargets in one call equal separate calls"
        y8 = np.concatenate([y, targets_near(x, 5, 8)])
        got8 = eng.column_misfits(names, y8)
        assert same_bits(got8[:3], got)
        for t in range(8):
            assert same_bits(eng.column_misfits(names, y8[t])[0], got8[t])
        # the device form
        rw = np.random.default_rng(2).uniform(0.0, 2.0, (len(names), nlat))
        for yy, rr in ((y, None), (y8, rw), (y8[4], rw)):
            nt = 1 if yy.ndim == 2 else yy.shape[0]
            buf = torch.full((nt, 2, ncol), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng.column_misfits_device(names, yy, buf.data_ptr(), rr)
            assert same_bits(buf.cpu().numpy(), eng.column_misfits(names, yy, rr))
        # a shift of the members permutes the result the same way
        before = eng.column_misfits(names, y8, rw)
        parents = (np.arange(ncol) + 5) % ncol
        eng.resample_columns(parents)
        after = eng.column_misfits(names, y8, rw)
        assert same_bits(after, before[:, :, parents]) and not same_bits(after, before)


def test_ensemble_run_misfits_and_assimilate(pkg):
    """EnsembleRun.misfits / misfits_tensor are the engine's calls; assimilate towards member 3's own T resamples onto it."""
    nlat, ncol = 180, 16
    eng, first = stepped(pkg, nlat, ncol)
    with eng:
        run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
        run.engine, run.ncol, run.device = eng, ncol, 0
        run.st = type("St", (), {"nx": nlat})()
        T = eng.get_field("T")
        obs = T[3].copy()
        obs[1::2] = np.nan
        got = run.misfits("T", obs[None])
        assert same_bits(got, column_misfits_ref(T[None], obs[None, None]))
        assert same_bits(run.misfits_tensor("T", obs[None]).cpu().numpy(), got)
        # (three steps apart the members' T differ in the fourth digit: an observation error far below that singles one out)
        res = run.assimilate("T", obs[None], 1e-12, np.random.default_rng(0))
        assert res["J"][3] == 0.0 and res["weights"][3] == pytest.approx(1.0) and res["ess"] < 1.5
        assert (res["parents"] == 3).all() and (res["N"] == nlat // 2).all()
        assert same_bits(eng.get_field("T"), np.tile(T[3], (ncol, 1))), "every member continues from member 3"


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    ncol, nlat = 33, 180
    eng, first = stepped(pkg, nlat, ncol, nsteps=2)
    lib, h = eng.lib, eng._h
    with eng:
        y = np.random.default_rng(1).normal(0.0, 1.0, (2, 2, nlat))
        y[:, :, ::9] = np.nan
        rw = np.random.default_rng(2).uniform(0.0, 1.0, (2, nlat))
        before = eng.column_misfits(("Ei", "T"), y, rw)
        state = (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions())
        out = np.zeros((2, 2, ncol))
        ids = lambda *names: (ctypes.c_int * len(names))(*[pkg.engine.FIELD[n] if isinstance(n, str) else n for n in names])
        op, yp, rp = out.ctypes.data_as(DP), y.ctypes.data_as(DP), rw.ctypes.data_as(DP)
        big = np.zeros((9, 2, nlat))

        def bad(a, index, value):
            a = a.copy()
            a[index] = value
            keep.append(a)
            return a.ctypes.data_as(DP)
        keep = []
        cases = {
            "null fields": lambda: lib.ebm_column_misfits(h, 2, None, 2, yp, rp, op),
            "null target": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, None, rp, op),
            "null out": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, yp, rp, None),
            "null dev_out": lambda: lib.ebm_column_misfits_device(h, 2, ids("Ei", "T"), 2, yp, rp, None),
            "nvars 0": lambda: lib.ebm_column_misfits(h, 0, ids("Ei", "T"), 2, yp, rp, op),
            "nvars 13": lambda: lib.ebm_column_misfits(h, 13, ids(*(MIZ_ALL + MIZ_ALL[:3])), 2, yp, rp, op),
            "ntargets 0": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 0, yp, rp, op),
            "ntargets 9": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 9, big.ctypes.data_as(DP), rp, op),
            "T0": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T0"), 2, yp, rp, op),
            "Tg on MIZ": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "Tg"), 2, yp, rp, op),
            "field 99": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", 99), 2, yp, rp, op),
            "field -1": lambda: lib.ebm_column_misfits(h, 2, ids(-1, "Ei"), 2, yp, rp, op),
            "repeated": lambda: lib.ebm_column_misfits(h, 2, ids("T", "T"), 2, yp, rp, op),
            "target inf": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, bad(y, (1, 0, 179), np.inf), rp, op),
            "target -inf": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, bad(y, (0, 1, 4), -np.inf), None, op),
            "rw negative": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, yp, bad(rw, (1, 7), -0.5), op),
            "rw nan": lambda: lib.ebm_column_misfits(h, 2, ids("Ei", "T"), 2, yp, bad(rw, (0, 0), np.nan), op),
            "rw inf": lambda: lib.ebm_column_misfits_device(h, 2, ids("Ei", "T"), 2, yp, bad(rw, (1, 179), np.inf), ctypes.c_void_p(16)),
        }
        says = {"repeated": b"twice", "nvars 13": b"nvars = 13", "ntargets 0": b"ntargets = 0", "ntargets 9": b"ntargets = 9",
                "target inf": b"target[1][0][179]", "target -inf": b"target[0][1][4]", "rw negative": b"rw[1][7]", "rw nan": b"rw[0][0]",
                "rw inf": b"rw[1][179]"}
        for name, call in cases.items():
            assert call() == -1, name                                     # EBM_ERR_ARG
            msg = lib.ebm_last_error()
            assert b"ebm_column_misfits" in msg and says.get(name, b"") in msg, (name, msg)
            assert (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions()) == state, name
            assert same_bits(eng.column_misfits(("Ei", "T"), y, rw), before), name
        # a stale T: the refusal of ebm_hemispheric_mean, with the same steps in the message
        eng.run(first + 2, 3, None, False, 1)
        with pytest.raises(pkg.StaleFieldError) as mine:
            eng.column_misfits(("Ei", "T"), y, rw)
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        assert tail(mine) == tail(theirs) and f"step {first + 1}" in tail(mine) and f"step {first + 4}" in tail(mine)
        assert mine.value.status == -5
        x = eng.get_field("Ei")[None]
        assert same_bits(eng.column_misfits("Ei", y[:, :1], rw[:1]), column_misfits_ref(x, y[:, :1], rw[:1]))
