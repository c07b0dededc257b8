"""GPU tests (-m gpu) of ebm_ensemble_range and ebm_ensemble_histogram with their _device forms (include/ebm_hip.h): the
number, minimum and maximum and the weighted histogram across the columns of a handle, per entry and latitude.

The oracle is tests/ensemble_hist_ref.py, the NumPy restatement of the two definitions (checked on the CPU against
np.histogram, np.min and np.max, tests/test_host_ensemble_hist.py); every comparison is BIT FOR BIT (same_bits).

Shapes, the smallest at which the kernels can go wrong.  Columns 1, 255, 256, 257, 513: less than a block of the histogram, a
block less one, one whole block, a block and one, two blocks and one — of the range's blocks of 32 that is up to seventeen —
with the load batch of 16 columns whole (256), with a tail of one (1, 257, 513) and of fifteen (255).  Latitudes 2, 5, 181,
1440 at four cells per thread and 181 at two: one pair, an odd tail whose last pair is half padding, more than one tile with
an odd tail, padding tiles that must not be read; 4096 x 257: the longest row; 8449 columns x 5: more blocks than one batch
of loads of the two finish kernels.  Bins 1, 7 and 64 on every shape.  Crafted
data is loaded with ebm_set_field, so those rows are in the natural layout; the pair-split layout is what one-step launches
leave behind, tested from real steps at 180 latitudes.
"""
import ctypes

import numpy as np
import pytest
import torch

from ensemble_hist_ref import ensemble_histogram_ref, ensemble_range_ref, same_bits, slots_ref
from support import assert_same_snapshot, forcing_of, make_engine, snapshot
from test_gpu_ensemble_sums import MIZ_ALL, blank_engine, coverage, crafted, grid, load, weights_for

pytestmark = pytest.mark.gpu

CRAFTED = ("Ei", "phi", "Ti", "T")                   # two prognostic and two diagnostic fields
BINS = (1, 7, 64)
DP = ctypes.POINTER(ctypes.c_double)


def edges_for(nvars, nlat, seed):
    """lo < 0 < hi over a few binades, so that the crafted magnitudes 2^-15 ... 2^16 of both signs fall below, inside and
    above; no value of crafted() lies within rounding of an edge except by the planted cases of the edge test."""
    rng = np.random.default_rng(seed)
    lo = -rng.uniform(1.0, 2.0, (nvars, nlat)) * 2.0 ** rng.integers(-3, 9, (nvars, nlat))
    hi = rng.uniform(1.0, 2.0, (nvars, nlat)) * 2.0 ** rng.integers(-3, 9, (nvars, nlat))
    return lo, hi


SHAPES = [(ncol, nlat, 4) for ncol in (1, 255, 256, 257, 513) for nlat in (2, 5, 181, 1440)] + \
         [(ncol, 181, 2) for ncol in (1, 255, 256, 257, 513)] + [(257, 4096, 4)]


@pytest.mark.parametrize("ncol, nlat, cells", SHAPES, ids=lambda v: str(v))
def test_crafted_data_against_the_restatement(pkg, ncol, nlat, cells):
    """The range and the histograms of 1, 7 and 64 bins: no weights against explicit ones (identical bits), weights with
    zeros and negative entries, all against the restatement."""
    x = crafted(len(CRAFTED), ncol, nlat, 1000 * ncol + nlat + cells)
    none, some, every = coverage(x)
    assert none and every and (some or ncol < 2), "honesty: the data holds the contributor patterns it claims"
    assert np.isinf(x).any() and (np.signbit(x) & (x == 0.0)).any()
    w = weights_for(ncol, nlat)
    lo, hi = edges_for(len(CRAFTED), nlat, ncol + nlat)
    with blank_engine(pkg, "MIZ", nlat, ncol, cells) as eng:
        assert eng.launch_info()["cells_per_thread"] == cells
        load(eng, CRAFTED, x)
        plain = eng.ensemble_range(CRAFTED)
        assert same_bits(plain, ensemble_range_ref(x)), "range"
        assert same_bits(eng.ensemble_range(CRAFTED, np.ones(ncol)), plain), "NULL weights are ones"
        assert same_bits(eng.ensemble_range(CRAFTED, w), ensemble_range_ref(x, w)), "range, weights"
        assert same_bits(eng.ensemble_range(CRAFTED, 3.0 * w), eng.ensemble_range(CRAFTED, w)), "a weight acts through being zero or not"
        gone = np.isnan(x).all(axis=1)
        assert (plain[:, 0][gone] == 0.0).all() and (plain[:, 1][gone] == np.inf).all() and (plain[:, 2][gone] == -np.inf).all()
        assert same_bits(eng.ensemble_range("Ti", w), ensemble_range_ref(x[2:3], w)), "one variable"
        for nbins in BINS:
            h = eng.ensemble_histogram(CRAFTED, lo, hi, nbins)
            assert same_bits(h, ensemble_histogram_ref(x, lo, hi, nbins)), ("unit weights", nbins)
            assert same_bits(eng.ensemble_histogram(CRAFTED, lo, hi, nbins, np.ones(ncol)), h), ("NULL weights are ones", nbins)
            assert same_bits(h.sum(axis=1), plain[:, 0]), "every contributor is in exactly one slot"
            assert (h.transpose(0, 2, 1)[gone] == 0.0).all(), "nobody contributes there"
            if ncol >= 255:
                assert (h[:, 0] > 0).any() and (h[:, -1] > 0).any() and (h[:, 1:-1] > 0).any(), "honesty: every slot class is filled"
                assert nbins == 1 or ((h[:, 1:-1] > 0).sum(axis=1) >= 2).any(), "honesty: more than one bin is filled"
            hw = eng.ensemble_histogram(CRAFTED, lo, hi, nbins, w)
            assert same_bits(hw, ensemble_histogram_ref(x, lo, hi, nbins, w)), ("weights", nbins)
            assert same_bits(eng.ensemble_histogram(CRAFTED, lo, hi, nbins, w), hw), "the same call, the same bits"
        assert same_bits(eng.ensemble_histogram("Ti", lo[2:3], hi[2:3], 7, w), ensemble_histogram_ref(x[2:3], lo[2:3], hi[2:3], 7, w))


@pytest.mark.parametrize("nbins", (1, 2, 3, 5, 7, 32, 63, 64))
def test_values_on_the_edges(pkg, nbins):
    """lo = -1, hi = 2: a value equal to lo is in bin 0, one equal to hi is above, nextafter(hi, -Inf) has t == nbins exactly
    and is clamped into the last bin; -Inf below, +Inf above; -0.0 with lo = 0.0 in bin 0.  Each planted member alone (all
    other weights zero) lands in the slot the definition names, and the whole ensemble gives the restatement's bits."""
    ncol, nlat = 257, 5
    x = np.random.default_rng(nbins).uniform(-2.0, 3.0, (1, ncol, nlat))
    lo, hi = np.full((1, nlat), -1.0), np.full((1, nlat), 2.0)
    lo[0, 3], hi[0, 3] = 0.0, 1.0
    last = np.nextafter(2.0, -np.inf)
    planted = {(5, 0): (-1.0, 1), (6, 0): (2.0, nbins + 1), (7, 0): (last, nbins), (256, 1): (last, nbins), (9, 2): (-np.inf, 0),
               (10, 2): (np.inf, nbins + 1), (11, 3): (-0.0, 1), (12, 3): (0.0, 1), (13, 3): (1.0, nbins + 1)}
    for (c, k), (val, _) in planted.items():
        x[0, c, k] = val
    _, t = slots_ref(x[0, 7], lo[0], hi[0], nbins)
    assert t[0] == float(nbins), "honesty: the data holds a value with t == nbins, which only the clamp keeps in the last bin"
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        eng.set_field("T", x[0])
        h = eng.ensemble_histogram("T", lo, hi, nbins)
        assert same_bits(h, ensemble_histogram_ref(x, lo, hi, nbins))
        assert h.sum() == ncol * nlat
        for (c, k), (_, slot) in planted.items():
            alone = np.zeros(ncol)
            alone[c] = 2.5
            got = eng.ensemble_histogram("T", lo, hi, nbins, alone)
            assert got[0, slot, k] == 2.5 and got[0, :, k].sum() == 2.5, (c, k, slot, got[0, :, k])
            want = ensemble_histogram_ref(x, lo, hi, nbins, alone)         # 2.5 in that member's slot at every latitude, 0.0 elsewhere
            assert same_bits(got, want), (c, k, slot, got[0, :, k])


def test_equal_extremes_keep_the_bits_of_the_first(pkg):
    """+0.0 and -0.0 compare equal: the first contributor in ascending column order gives the bits of the minimum and of the
    maximum — inside a block of 32, across blocks, and with the first of them hidden by a zero weight."""
    ncol, nlat = 97, 5
    x = np.random.default_rng(3).uniform(1.0, 2.0, (1, ncol, nlat))
    x[0, :, 0] = 0.0
    x[0, 3, 0] = -0.0                                    # lat 0: +0.0 first (column 0), -0.0 later in the block
    x[0, :, 1] = -0.0
    x[0, 40, 1] = 0.0                                    # lat 1: -0.0 first
    x[0, :, 2] = -x[0, :, 2]
    x[0, 33, 2], x[0, 70, 2] = 0.0, -0.0                 # lat 2: the maximum is +0.0 of block 1, then -0.0 of block 2
    x[0, 33, 3], x[0, 70, 3] = -0.0, 0.0                 # lat 3: the minimum is -0.0 of block 1, then +0.0 of block 2
    x[0, 3, 4], x[0, 5, 4] = -0.0, 0.0                   # lat 4: the minimum is -0.0, then +0.0 inside the same block, the last of them
    w = np.ones(ncol)
    w[[0, 33]] = 0.0
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        eng.set_field("T", x[0])
        got, gotw = eng.ensemble_range("T"), eng.ensemble_range("T", w)
    sign = lambda a: bool(np.signbit(a))
    assert [sign(got[0, 1, 0]), sign(got[0, 2, 0]), sign(got[0, 1, 1]), sign(got[0, 2, 1])] == [False, False, True, True]
    assert got[0, 2, 2] == 0.0 and not sign(got[0, 2, 2]) and got[0, 1, 3] == 0.0 and sign(got[0, 1, 3])
    assert got[0, 1, 4] == 0.0 and sign(got[0, 1, 4]), "a later equal value inside the block does not replace the first"
    assert sign(gotw[0, 1, 0]) is False and sign(gotw[0, 2, 2]) is True and sign(gotw[0, 1, 3]) is False
    for ww in (None, w):
        want = ensemble_range_ref(x, ww)
        assert same_bits(got if ww is None else gotw, want)
        for block in (1, 7, ncol):
            assert same_bits(ensemble_range_ref(x, ww, block), want), "the result does not depend on the blocking"


def test_more_blocks_than_a_batch_of_the_finish_kernels(pkg):
    """8449 columns are 34 blocks of the histogram and 265 of the range: the finish kernels add 32 block partials per batch of
    loads, so this is one batch and a tail of two, and eight batches and a tail of nine.  With weights: the order shows."""
    ncol, nlat = 8449, 5
    x = crafted(1, ncol, nlat, 99)
    w = weights_for(ncol, 1)
    lo, hi = edges_for(1, nlat, 3)
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        eng.set_field("T", x[0])
        assert same_bits(eng.ensemble_range("T", w), ensemble_range_ref(x, w))
        assert same_bits(eng.ensemble_histogram("T", lo, hi, 7, w), ensemble_histogram_ref(x, lo, hi, 7, w))
        assert same_bits(eng.ensemble_histogram("T", lo, hi, 64), ensemble_histogram_ref(x, lo, hi, 64))


def test_a_repeated_field_with_its_own_edges(pkg):
    ncol, nlat = 257, 181
    x = crafted(2, ncol, nlat, 5)
    names, rows = ("T", "phi", "T", "T"), [1, 0, 1, 1]
    w = weights_for(ncol, 2)
    lo, hi = edges_for(4, nlat, 17)
    lo[3], hi[3] = lo[0], hi[0]                          # the same entry twice: the same result twice
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, ("phi", "T"), x)
        h = eng.ensemble_histogram(names, lo, hi, 7, w)
        assert same_bits(h, ensemble_histogram_ref(x[rows], lo, hi, 7, w))
        assert same_bits(h[0], h[3]) and not same_bits(h[0], h[2]), "honesty: the rows of edges differ"


def test_all_variables_of_each_model(pkg):
    ncol, nlat = 257, 181
    x = crafted(10, ncol, nlat, 21)
    w = weights_for(ncol, 4)
    lo, hi = edges_for(10, nlat, 9)
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, MIZ_ALL, x)
        assert same_bits(eng.ensemble_range(MIZ_ALL, w), ensemble_range_ref(x, w))
        assert same_bits(eng.ensemble_histogram(MIZ_ALL, lo, hi, 7, w), ensemble_histogram_ref(x, lo, hi, 7, w))
        twelve = MIZ_ALL + ("T", "Ei")
        idx = [MIZ_ALL.index(n) for n in twelve]
        assert same_bits(eng.ensemble_histogram(twelve, lo[idx], hi[idx], 64), ensemble_histogram_ref(x[idx], lo[idx], hi[idx], 64))
    names = ("E", "Tg", "T", "h")
    with blank_engine(pkg, "Classic", nlat, ncol) as eng:
        load(eng, names, x[:4])
        assert same_bits(eng.ensemble_range(names, w), ensemble_range_ref(x[:4], w))
        assert same_bits(eng.ensemble_histogram(names, lo[:4], hi[:4], 64, w), ensemble_histogram_ref(x[:4], lo[:4], hi[:4], 64, w))


def test_device_variants_equal_the_host_variants(pkg):
    ncol, nlat = 257, 181
    x = crafted(3, ncol, nlat, 31)
    names = ("Ei", "Tw", "T")
    w = weights_for(ncol, 6)
    lo, hi = edges_for(3, nlat, 4)
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, names, x)
        for ww in (None, w):
            buf = torch.full((3, 3, nlat), float("nan"), dtype=torch.float64, device="cuda")
            hist = torch.full((3, 66, nlat), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            eng.ensemble_range_device(names, buf.data_ptr(), ww)
            eng.ensemble_histogram_device(names, lo, hi, 64, hist.data_ptr(), ww)
            assert same_bits(buf.cpu().numpy(), eng.ensemble_range(names, ww))
            assert same_bits(buf.cpu().numpy(), ensemble_range_ref(x, ww))
            assert same_bits(hist.cpu().numpy(), eng.ensemble_histogram(names, lo, hi, 64, ww))
            assert same_bits(hist.cpu().numpy(), ensemble_histogram_ref(x, lo, hi, 64, ww))


def test_shards_combine_to_the_unsharded_call(pkg):
    """Three handles hold the shards of one ensemble: unit-weight histograms add, and the ranges combine with SUM, MIN and
    MAX, to the unsharded call bit for bit."""
    ncol, nlat = 513, 181
    x = crafted(2, ncol, nlat, 8)
    assert not ((x == 0.0) & ~np.signbit(x)).any(), "no +0.0 beside the -0.0: extremes have one bit pattern"
    names = ("h", "T")
    lo, hi = edges_for(2, nlat, 6)
    cuts = [0, 200, 456, 513]
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, names, x)
        whole_h, whole_r = eng.ensemble_histogram(names, lo, hi, 64), eng.ensemble_range(names)
    hs, rs = [], []
    for a, b in zip(cuts, cuts[1:]):
        with blank_engine(pkg, "MIZ", nlat, b - a) as eng:
            load(eng, names, x[:, a:b])
            hs.append(eng.ensemble_histogram(names, lo, hi, 64))
            rs.append(eng.ensemble_range(names))
    assert same_bits(sum(hs[1:], hs[0]), whole_h)
    rs = np.stack(rs)
    assert same_bits(rs[:, :, 0].sum(axis=0), whole_r[:, 0])
    assert same_bits(np.minimum.reduce(rs[:, :, 1]), whole_r[:, 1]) and same_bits(np.maximum.reduce(rs[:, :, 2]), whole_r[:, 2])


# ---- both stored layouts, from real steps ---------------------------------------------------------------------------------------

def real_edges(x):
    """Per entry and latitude edges a little inside the members' spread, so that below, above and the bins all fill."""
    nobody = np.isnan(x).all(axis=1)                     # (Ti and Tw where no member has ice or water)
    mn, mx = np.nanmin(np.where(nobody[:, None], 0.0, x), axis=1), np.nanmax(np.where(nobody[:, None], 0.0, x), axis=1)
    width = np.where(mx > mn, mx - mn, 1.0)
    return mn + 0.1 * width, mn + 0.8 * width


@pytest.mark.parametrize("cells, spl, diag, names",
                         [(4, 1, True, MIZ_ALL), (4, 7, True, ("Ei", "phi", "T")), (4, 1, False, ("phi", "Ei")), (2, 1, True, MIZ_ALL)],
                         ids=["pair_split_all_ten", "natural_after_fused", "phi_underived", "two_cells"])
def test_rows_are_read_where_they_lie(pkg, cells, spl, diag, names):
    """Three steps, then the range and the histogram: no conversion, the bits of the restatement on the fields read back from
    a twin afterwards, the bookkeeping untouched, and the run continues as the twin's that never made the calls.  Honesty:
    that the prognostic rows really lie pair-split is read off the twin, whose first ebm_get_field of a prognostic field
    must convert the state exactly in the cases that claim it."""
    ncol = 65
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, cells, ("noise",))
    twin, _ = make_engine(pkg, "MIZ", "sin", 180, ncol, cells, ("noise",))
    first = st.nt // 2
    w = weights_for(ncol, 13)
    with eng, twin:
        for e in (eng, twin):
            e.run(first, 3, forcing_of(first, 3), diag, spl)
        before = twin.state_conversions()
        twin.get_field("Ei")
        assert twin.state_conversions() - before == (1 if cells == 4 and spl == 1 else 0), "honesty: the layout the case names"
        x = np.stack([twin.get_field(n) for n in names])
        lo, hi = real_edges(x)
        conv, counters = eng.state_conversions(), eng.counters()
        steps = {k: eng.field_step(k) for k in MIZ_ALL}
        r, rw = eng.ensemble_range(names), eng.ensemble_range(names, w)
        h, hw = eng.ensemble_histogram(names, lo, hi, 7), eng.ensemble_histogram(names, lo, hi, 64, w)
        assert eng.state_conversions() == conv, "no field is converted"
        assert eng.counters() == counters and {k: eng.field_step(k) for k in MIZ_ALL} == steps
        if not diag:
            with pytest.raises(pkg.StaleFieldError):
                eng.ensemble_range(("phi", "T"))
        assert len({row.tobytes() for row in x[0]}) == ncol, "honesty: the members differ"
        assert same_bits(r, ensemble_range_ref(x)) and same_bits(rw, ensemble_range_ref(x, w))
        assert same_bits(h, ensemble_histogram_ref(x, lo, hi, 7)) and same_bits(hw, ensemble_histogram_ref(x, lo, hi, 64, w))
        assert (h[:, 0] > 0).any() and (h[:, -1] > 0).any() and (h[:, 1:-1] > 0).any()
        for e in (eng, twin):
            e.run(first + 3, 4, forcing_of(first + 3, 4), True, spl)
        assert_same_snapshot(snapshot(eng, "MIZ"), snapshot(twin, "MIZ"), "the run continues as without the calls")


# ---- bookkeeping and refusals ---------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    ncol = 33
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, 4)
    first = st.nt // 2
    lib, h = eng.lib, eng._h
    with eng:
        eng.run(first, 2, None, True, 1)
        lo, hi = np.full((2, 180), -5.0), np.full((2, 180), 40.0)
        before = (eng.ensemble_range(("Ei", "T")), eng.ensemble_histogram(("Ei", "T"), lo, hi, 7))
        state = (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions())
        out = np.zeros((13, 66, 180))
        w = np.ones(ncol)
        ids = lambda *names: (ctypes.c_int * len(names))(*[pkg.engine.FIELD[n] if isinstance(n, str) else n for n in names])
        op, lop, hip_ = out.ctypes.data_as(DP), lo.ctypes.data_as(DP), hi.ctypes.data_as(DP)

        def bad(a, i, v):
            a = a.copy()
            a.flat[i] = v
            return a
        bad_w = {k: bad(w, *v) for k, v in {"nan": (7, np.nan), "inf": (32, -np.inf)}.items()}
        bad_lo = {k: bad(lo, *v) for k, v in {"nan": (359, np.nan), "inf": (3, -np.inf), "eq": (181, 40.0), "gt": (5, 41.0),
                                              "wide": (2, -1.7e308)}.items()}
        bad_hi = {k: bad(hi, *v) for k, v in {"nan": (0, np.nan), "inf": (190, np.inf), "wide": (2, 1.7e308)}.items()}
        p = lambda a: a.ctypes.data_as(DP)
        rng = lambda n, f, ww, o: lib.ebm_ensemble_range(h, n, f, ww, o)
        hst = lambda n, f, ww, nb, l, u, o: lib.ebm_ensemble_histogram(h, n, f, ww, nb, l, u, o)
        cases = {
            "range null fields": lambda: rng(2, None, None, op),
            "range null out": lambda: rng(2, ids("Ei", "T"), None, None),
            "range null dev_out": lambda: lib.ebm_ensemble_range_device(h, 2, ids("Ei", "T"), None, None),
            "range nvars 0": lambda: rng(0, ids("Ei", "T"), None, op),
            "range nvars 13": lambda: rng(13, ids(*(MIZ_ALL + MIZ_ALL[:3])), None, op),
            "range T0": lambda: rng(2, ids("Ei", "T0"), None, op),
            "range Tg on MIZ": lambda: rng(2, ids("Ei", "Tg"), None, op),
            "range repeated": lambda: rng(2, ids("T", "T"), None, op),
            "range w nan": lambda: rng(2, ids("Ei", "T"), p(bad_w["nan"]), op),
            "hist null fields": lambda: hst(2, None, None, 7, lop, hip_, op),
            "hist null out": lambda: hst(2, ids("Ei", "T"), None, 7, lop, hip_, None),
            "hist null dev_out": lambda: lib.ebm_ensemble_histogram_device(h, 2, ids("Ei", "T"), None, 7, lop, hip_, None),
            "hist null lo": lambda: hst(2, ids("Ei", "T"), None, 7, None, hip_, op),
            "hist null hi": lambda: hst(2, ids("Ei", "T"), None, 7, lop, None, op),
            "hist nvars 0": lambda: hst(0, ids("Ei", "T"), None, 7, lop, hip_, op),
            "hist nvars 13": lambda: hst(13, ids(*(MIZ_ALL + MIZ_ALL[:3])), None, 7, lop, hip_, op),
            "hist T0": lambda: hst(2, ids("Ei", "T0"), None, 7, lop, hip_, op),
            "hist field 99": lambda: hst(2, ids("Ei", 99), None, 7, lop, hip_, op),
            "hist nbins 0": lambda: hst(2, ids("Ei", "T"), None, 0, lop, hip_, op),
            "hist nbins 65": lambda: hst(2, ids("Ei", "T"), None, 65, lop, hip_, op),
            "hist nbins -1": lambda: hst(2, ids("Ei", "T"), None, -1, lop, hip_, op),
            "hist w nan": lambda: hst(2, ids("Ei", "T"), p(bad_w["nan"]), 7, lop, hip_, op),
            "hist w inf": lambda: hst(2, ids("Ei", "T"), p(bad_w["inf"]), 7, lop, hip_, op),
            "hist lo nan": lambda: hst(2, ids("Ei", "T"), None, 7, p(bad_lo["nan"]), hip_, op),
            "hist lo inf": lambda: hst(2, ids("Ei", "T"), None, 7, p(bad_lo["inf"]), hip_, op),
            "hist lo == hi": lambda: hst(2, ids("Ei", "T"), None, 7, p(bad_lo["eq"]), hip_, op),
            "hist lo > hi": lambda: hst(2, ids("Ei", "T"), None, 7, p(bad_lo["gt"]), hip_, op),
            "hist hi nan": lambda: hst(2, ids("Ei", "T"), None, 7, lop, p(bad_hi["nan"]), op),
            "hist hi inf": lambda: hst(2, ids("Ei", "T"), None, 7, lop, p(bad_hi["inf"]), op),
            "hist hi - lo overflows": lambda: hst(2, ids("Ei", "T"), None, 7, p(bad_lo["wide"]), p(bad_hi["wide"]), op),
        }
        says = {"range w nan": b"w[7]", "hist w inf": b"w[32]", "range repeated": b"twice", "range nvars 13": b"nvars = 13",
                "hist nvars 13": b"nvars = 13", "hist nbins 0": b"nbins = 0", "hist nbins 65": b"nbins = 65",
                "hist lo nan": b"lo[1][179]", "hist lo inf": b"lo[0][3]", "hist lo == hi": b"lo[1][1]", "hist lo > hi": b"lo[0][5]",
                "hist hi nan": b"hi[0][0]", "hist hi inf": b"hi[1][10]", "hist hi - lo overflows": b"lo[0][2]"}
        for name, call in cases.items():
            assert call() == -1, name                                     # EBM_ERR_ARG
            msg = lib.ebm_last_error()
            who = b"ebm_ensemble_range" if name.startswith("range") else b"ebm_ensemble_histogram"
            assert who in msg and says.get(name, b"") in msg, (name, msg)
            assert (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions()) == state, name
            assert same_bits(eng.ensemble_range(("Ei", "T")), before[0]), name
            assert same_bits(eng.ensemble_histogram(("Ei", "T"), lo, hi, 7), before[1]), name
        assert same_bits(eng.ensemble_histogram(("T", "T"), lo, hi, 7)[1], before[1][1]), "a histogram may repeat a field"
        # a stale T: the refusal of ebm_hemispheric_mean, with the same steps in the message
        eng.run(first + 2, 3, None, False, 1)
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        for call in (lambda: eng.ensemble_range(("Ei", "T")), lambda: eng.ensemble_histogram(("Ei", "T"), lo, hi, 7)):
            with pytest.raises(pkg.StaleFieldError) as mine:
                call()
            assert tail(mine) == tail(theirs) and f"step {first + 1}" in tail(mine) and f"step {first + 4}" in tail(mine)
            assert mine.value.status == -5
        x = eng.get_field("Ei")[None]
        assert same_bits(eng.ensemble_range("Ei"), ensemble_range_ref(x))
        assert same_bits(eng.ensemble_histogram("Ei", lo[:1], hi[:1], 7), ensemble_histogram_ref(x, lo[:1], hi[:1], 7))


# ---- quantiles ------------------------------------------------------------------------------------------------------------------

def test_quantiles_of_a_noisy_ensemble_against_numpy(pkg):
    """EnsembleRun.quantiles after a short noisy run: every value within its halfwidth of NumPy's inverted-CDF quantile of
    the downloaded fields (np.quantile(method="inverted_cdf"): the smallest value whose cumulative frequency reaches q), the
    halfwidth within (max - min) * nbins ** -passes up to the stated widening, ice-free latitudes constant with halfwidth 0."""
    ncol, nlat = 300, 90
    st = grid(pkg, nlat)
    rng = np.random.default_rng(12)
    init = {k: np.zeros((ncol, nlat)) for k in ("Ei", "Ew", "h", "D", "phi")}
    init["Ew"] = rng.normal(0.0, 2.0, (ncol, 1)) * np.ones((1, nlat))
    run = pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), init, noise={"sigma": 20.0, "rho": 0.9, "seed": 5})
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    try:
        run.run(40)
        got = run.quantiles(("T", "phi", "Ew"), qs)
        fields = {n: run.engine.get_field(n) for n in ("T", "phi", "Ew")}
        ensemble = __import__("sys").modules[pkg.__name__ + ".ensemble"]
        nbins, passes = ensemble.QUANTILE_NBINS, ensemble.QUANTILE_PASSES
        for n, x in fields.items():
            assert not np.isnan(x).any()
            want = np.quantile(x, qs, axis=0, method="inverted_cdf")
            spread = x.max(axis=0) - x.min(axis=0)
            v, hw = got[n]["value"], got[n]["halfwidth"]
            print(n, "max halfwidth", float(hw.max()), "max |value - numpy| / halfwidth",
                  float(np.max(np.abs(v - want)[hw > 0] / hw[hw > 0])) if (hw > 0).any() else 0.0)
            assert (np.abs(v - want) <= hw).all(), n
            # the widening: 16 ulps a side of the first bracket and of every pass's bin, of an end at most a binade above the data's
            pad = 2 * 16 * (passes + 1) * np.spacing(np.maximum(np.abs(x.max(axis=0)), np.abs(x.min(axis=0))))
            assert (hw <= spread * float(nbins) ** -passes + pad).all(), n
            assert ((hw == 0.0) == (spread == 0.0)[None]).all(), n
        assert (fields["T"].max(axis=0) > fields["T"].min(axis=0)).all(), "honesty: the members differ"
    finally:
        run.close()
