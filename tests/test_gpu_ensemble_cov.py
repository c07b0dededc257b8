"""GPU tests (-m gpu) of ebm_ensemble_covariance / ebm_ensemble_covariance_device (include/ebm_hip.h): the covariance across
the columns of a handle for every pair of latitudes, on the fp64 matrix instruction.

Two oracles.  EXACT: small-integer fields, weights and centers make every product and every partial sum an integer below
2^53, so the result is the integer matrix BIT FOR BIT whatever the order inside the instruction — this is what catches an
indexing, tiling, operand-layout or tail error.  BOUND: on real model data the NumPy restatement of the terms with
np.longdouble sums (tests/ensemble_cov_ref.py) and the derived bound (n + nblocks) 2^-53 T_ij (1 + 2^-4).

Shapes, the smallest at which the kernels can go wrong.  Latitudes 2 (below one 16 x 16 instruction tile), 17 (one past it,
odd), 65 (one past a 64-cell workgroup tile: off-diagonal tiles and the mirror), 130 (more than two tiles), 180 (the
reference's).  Columns 1, 3, 5, 37 (no multiple of four; more than two staged chunks of 16), 513 and 1027 (kCovBlock + 1 and
2 kCovBlock + 3: more than one and more than two member blocks, each with a tail).  Crafted data is loaded with ebm_set_field, so
those rows are natural; the pair-split layout is what one-step launches leave behind, tested from real steps at 180 latitudes
(pitch 256: one 128-cell natural span per half of a split row) and at 513 (pitch 768: three spans per half, padding tiles)."""
import ctypes

import numpy as np
import pytest
import torch

from ensemble_cov_ref import K_COV_BLOCK, covariance_bound, ensemble_cov_ref, terms
from support import MIZ_PROG, forcing_of, make_engine, same_bits
from test_gpu_ensemble_sums import blank_engine, grid, load

pytestmark = pytest.mark.gpu

MIZ_ALL = ("Ei", "Ew", "h", "D", "phi", "Tw", "Ti", "n", "E", "T")
DP = ctypes.POINTER(ctypes.c_double)
NLATS = (2, 17, 65, 130, 180)
NCOLS = (1, 3, 5, 37, K_COV_BLOCK + 1, 2 * K_COV_BLOCK + 3)


def integer_fields(nfields, ncol, nlat, seed):
    """[nfields, ncol, nlat] of integers |x| <= 2^10 with NaN in some cells, integer weights in -3 ... 4 with zeros, whose
    members hold Inf in a few cells, and two integer centers |c| <= 8."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1024, 1025, (nfields, ncol, nlat)).astype(np.float64)
    x[rng.random(x.shape) < 0.1] = np.nan
    w = rng.integers(-3, 5, ncol).astype(np.float64)
    if ncol > 2:
        w[2] = 0.0
    for c in np.flatnonzero(w == 0.0):
        x[:, c, rng.integers(nlat)] = np.inf
    centers = rng.integers(-8, 9, (2, nlat)).astype(np.float64)
    return x, w, centers


def exact_cov(xa, xb, w, ca, cb, symmetric):
    """The integer matrix in int64: the terms of the restatement are integers here, and so is every sum."""
    with np.errstate(invalid="ignore"):
        a, b = terms(np.where(np.isinf(xa), np.nan, xa), np.where(np.isinf(xb), np.nan, xb), w, ca, cb)    # (Inf only where w == 0)
    assert (a == np.rint(a)).all() and (b == np.rint(b)).all()
    out = (a.astype(np.int64).T @ b.astype(np.int64)).astype(np.float64)
    assert np.abs(out).max(initial=0.0) < 2.0 ** 52 and np.abs(a).max() * np.abs(b).max() * a.shape[0] < 2.0 ** 52
    return (np.triu(out) + np.triu(out, 1).T) if symmetric else out


@pytest.mark.parametrize("ncol", NCOLS)
@pytest.mark.parametrize("nlat", NLATS)
def test_integer_data_bit_for_bit(pkg, nlat, ncol):
    x, w, (ca, cb) = integer_fields(2, ncol, nlat, 100 * nlat + ncol)
    names = ("Ei", "T")                              # a prognostic and a diagnostic field
    unit = np.where(np.isinf(x), np.nan, x)          # with w = NULL every member counts: no Inf then
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, names, x)
        both = eng.ensemble_covariance("Ei", "T", w, ca, cb)
        assert same_bits(both, exact_cov(x[0], x[1], w, ca, cb, False)), "two fields, weights, two centers"
        assert same_bits(eng.ensemble_covariance("T", "Ei", w, None, cb), exact_cov(x[1], x[0], w, None, cb, False)), "one center"
        sym = eng.ensemble_covariance("T", None, w)
        assert same_bits(sym, exact_cov(x[1], x[1], w, None, None, True)) and same_bits(sym, sym.T), "one field, no center"
        sym = eng.ensemble_covariance("Ei", "Ei", w, ca, ca.copy())
        assert same_bits(sym, exact_cov(x[0], x[0], w, ca, ca, True)) and same_bits(sym, sym.T), "one field, one center twice"
        assert same_bits(eng.ensemble_covariance("Ei", "Ei", w, ca, cb), exact_cov(x[0], x[0], w, ca, cb, False)), "two centers: no mirror"
        load(eng, names, unit)
        plain = eng.ensemble_covariance("Ei", "T")
        assert same_bits(plain, exact_cov(unit[0], unit[1], None, None, None, False)), "w = NULL"
        assert same_bits(eng.ensemble_covariance("Ei", "T", np.ones(ncol)), plain), "NULL weights are ones"
        assert same_bits(eng.ensemble_covariance("Ei", "T"), plain), "the same call, the same bits"
        assert same_bits(eng.ensemble_covariance("T", "T", None, cb, cb), exact_cov(unit[1], unit[1], None, cb, cb, True))


def test_classic_model(pkg):
    ncol, nlat = 37, 65
    x, w, (ca, cb) = integer_fields(2, ncol, nlat, 5)
    with blank_engine(pkg, "Classic", nlat, ncol) as eng:
        load(eng, ("E", "T"), x)
        assert same_bits(eng.ensemble_covariance("E", "T", w, ca, cb), exact_cov(x[0], x[1], w, ca, cb, False))
        assert same_bits(eng.ensemble_covariance("T", "T", w, cb, cb), exact_cov(x[1], x[1], w, cb, cb, True))
        with pytest.raises(ValueError):
            eng.ensemble_covariance("E", "Ti")


def test_inf_is_data(pkg):
    """An infinite contributing cell: out[i][j] is +-Inf where every other term is finite, NaN where Inf meets a cleaned b = 0."""
    ncol, nlat = 5, 17
    x = np.random.default_rng(1).integers(1, 9, (2, ncol, nlat)).astype(np.float64)
    x[0, 1, 3] = np.inf
    x[1, 1, 7] = np.nan                              # the same member: b = +0.0 there
    with blank_engine(pkg, "MIZ", nlat, ncol) as eng:
        load(eng, ("Ei", "T"), x)
        got = eng.ensemble_covariance("Ei", "T")
        assert np.isnan(got[3, 7]) and (got[3, np.arange(nlat) != 7] == np.inf).all() and np.isfinite(np.delete(got, 3, axis=0)).all()


# ---- real model data: both stored layouts, the bound, the independence of layout and geometry ------------------------------------

PAIRS = (("T", "T"), ("Ti", "phi"), ("Ei", "Tw"), ("phi", "phi"))


def weights_for(ncol, seed):
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 4.0, ncol) * rng.choice([-1.0, 1.0, 1.0], ncol)
    w[rng.random(ncol) < 0.25] = 0.0
    w[2] = 0.0
    return w


@pytest.fixture(scope="module")
def stepped(pkg):
    """A stepped MIZ ensemble of kCovBlock + 1 members with noise at four cells per thread, three one-step launches with the
    diagnostics written by the last: state and diagnostics lie pair-split.  Yields (eng, ncol)."""
    ncol = K_COV_BLOCK + 1
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, 4, ("noise",))
    first = st.nt // 2
    with eng:
        eng.run(first, 3, forcing_of(first, 3), True, 1)
        yield eng, ncol


def test_real_data_within_the_derived_bound_in_either_layout_and_geometry(pkg, stepped):
    eng, ncol = stepped
    nlat = 180
    w = weights_for(ncol, 13)
    centers = {n: np.random.default_rng(i).normal(0.0, 2.0, nlat) for i, n in enumerate(MIZ_ALL)}
    conv, counters = eng.state_conversions(), eng.counters()
    steps = {k: eng.field_step(k) for k in MIZ_ALL}
    calls = [(a, b, ww, ca, cb) for a, b in PAIRS for ww, ca, cb in ((None, None, None), (w, centers[a], centers[b]))]
    split = [eng.ensemble_covariance(*c) for c in calls]
    assert all(same_bits(eng.ensemble_covariance(*c), s) for c, s in zip(calls, split)), "the same call, the same bits"
    assert eng.state_conversions() == conv, "no field is converted"
    assert eng.counters() == counters and {k: eng.field_step(k) for k in MIZ_ALL} == steps
    # the fields AFTER the calls: this converts state and diagnostics to the natural layout
    x = {n: eng.get_field(n) for n in ("T", "Ti", "phi", "Ei", "Tw")}
    assert eng.state_conversions() == conv + 1, "honesty: the state lay pair-split"
    assert np.isnan(x["Ti"]).any() and np.isnan(x["Tw"]).any(), "honesty: the sentinels are there"
    assert len({row.tobytes() for row in x["T"]}) == ncol, "honesty: the members differ"
    worst = 0.0
    for (a, b, ww, ca, cb), got in zip(calls, split):
        ref, T, n = ensemble_cov_ref(x[a], x[b], ww, ca, cb, same_field=a == b)
        bound = covariance_bound(T, n, ncol)
        err = np.abs(got - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0.0, err / bound, 0.0))))
        assert (err <= bound).all(), (a, b, ww is not None, float(np.max(err - bound)))
        if a == b:
            assert same_bits(got, got.T), (a, "rule 6: symmetric to the bit")
    print("largest error / bound:", worst)
    natural = [eng.ensemble_covariance(*c) for c in calls]
    assert all(same_bits(s, m) for s, m in zip(split, natural)), "the natural layout gives the bits of the pair-split one"
    # the same fields in a handle at two cells per thread; then Inf for NaN in the members of weight zero
    hidden = {n: np.where(np.isnan(v) & (w == 0.0)[:, None], np.inf, v) for n, v in x.items()}
    assert any(np.isinf(v).any() for v in hidden.values())
    with blank_engine(pkg, "MIZ", nlat, ncol, 2) as two:
        assert two.launch_info()["cells_per_thread"] == 2
        load(two, tuple(x), np.stack(list(x.values())))
        assert all(same_bits(two.ensemble_covariance(*c), s) for c, s in zip(calls, split)), "two cells per thread"
        load(two, tuple(x), np.stack(list(hidden.values())))
        for c, s in zip(calls, split):
            if c[2] is not None:
                assert same_bits(two.ensemble_covariance(*c), s), "a zero weight hides the cell, whatever it holds"


def test_device_variant_equals_the_host_variant(pkg, stepped):
    eng, ncol = stepped
    w = weights_for(ncol, 3)
    c = np.linspace(-1.0, 1.0, 180)
    for a, b, ww, ca, cb in (("T", "T", None, None, None), ("Ei", "T", w, c, None)):
        buf = torch.full((180, 180), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        eng.ensemble_covariance_device(a, b, ww, ca, cb, buf.data_ptr())
        assert same_bits(buf.cpu().numpy(), eng.ensemble_covariance(a, b, ww, ca, cb))


def test_rule_six_in_split_rows_of_more_than_one_span(pkg):
    """513 latitudes at four cells per thread: 192 threads, pitch 768, twelve stored tiles of which each half of a pair-split
    row holds six — several 128-cell natural spans per half, so that the tiles and waves which rule 6 skips are decided from
    natural spans that differ from the tile indices, and padding tiles exist.  The bits of the pair-split rows against the
    natural ones and against two cells per thread; the bound; the symmetry."""
    ncol, nlat = 37, 513
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, 4, ("noise",))
    first = st.nt // 2
    w = weights_for(ncol, 5)
    c = np.random.default_rng(4).normal(0.0, 2.0, nlat)
    calls = [("T", "T", None, None, None), ("phi", "phi", w, c, c), ("Ei", "T", w, c, None), ("T", "Ei", None, None, c)]
    with eng:
        assert eng.launch_info()["cells_per_thread"] == 4
        eng.run(first, 3, forcing_of(first, 3), True, 1)
        conv = eng.state_conversions()
        split = [eng.ensemble_covariance(*k) for k in calls]
        assert eng.state_conversions() == conv
        x = {n: eng.get_field(n) for n in ("T", "phi", "Ei")}
        assert eng.state_conversions() == conv + 1, "honesty: the state lay pair-split"
        for (a, b, ww, ca, cb), got in zip(calls, split):
            ref, T, n = ensemble_cov_ref(x[a], x[b], ww, ca, cb, same_field=a == b)
            assert (np.abs(got - ref) <= covariance_bound(T, n, ncol)).all(), (a, b)
            assert a != b or same_bits(got, got.T)
        assert all(same_bits(eng.ensemble_covariance(*k), s) for k, s in zip(calls, split)), "natural rows, the same bits"
    with blank_engine(pkg, "MIZ", nlat, ncol, 2) as two:
        load(two, tuple(x), np.stack(list(x.values())))
        assert all(same_bits(two.ensemble_covariance(*k), s) for k, s in zip(calls, split)), "two cells per thread"


def test_tensor_variant_of_an_ensemble_run(pkg):
    """EnsembleRun.ensemble_covariance_tensor, the payload of the all-reduce between shards: the bits of the host variant."""
    ncol, nlat = 37, 65
    st = grid(pkg, nlat)
    rng = np.random.default_rng(2)
    phi, T = rng.uniform(0.0, 1.0, (ncol, nlat)), rng.normal(5.0, 2.0, (ncol, nlat))
    run = pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), {n: np.zeros((ncol, nlat)) for n in MIZ_PROG if n != "phi"} | {"phi": phi})
    try:
        run.engine.set_field("T", T)
        w, c = weights_for(ncol, 1), rng.normal(0.0, 1.0, nlat)
        for args in (("T",), ("T", "phi", w, c, None), ("phi", "phi", w, c, c)):
            t = run.ensemble_covariance_tensor(*args)
            assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (nlat, nlat)
            assert same_bits(t.cpu().numpy(), run.ensemble_covariance(*args))
        assert not same_bits(run.ensemble_covariance("T", "phi"), run.ensemble_covariance("phi", "T")), "honesty: rows are field_a"
    finally:
        run.close()


def test_refusals_leave_the_handle_alone(pkg):
    ncol = 33
    eng, st = make_engine(pkg, "MIZ", "sin", 180, ncol, 4)
    first = st.nt // 2
    lib, h = eng.lib, eng._h
    F = pkg.engine.FIELD
    with eng:
        eng.run(first, 2, None, True, 1)
        before = eng.ensemble_covariance("Ei", "T")
        state = (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions())
        out = np.zeros((180, 180))
        op = out.ctypes.data_as(DP)

        def bad(n, k, v):
            a = np.ones(n)
            a[k] = v
            return a.ctypes.data_as(DP), a
        cases = {
            "null out": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T"], None, None, None, None),
            "null dev_out": lambda: lib.ebm_ensemble_covariance_device(h, F["Ei"], F["T"], None, None, None, None),
            "T0": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T0"], None, None, None, op),
            "Tg on MIZ": lambda: lib.ebm_ensemble_covariance(h, F["Tg"], F["T"], None, None, None, op),
            "field 99": lambda: lib.ebm_ensemble_covariance(h, 99, F["T"], None, None, None, op),
            "field -1": lambda: lib.ebm_ensemble_covariance(h, F["T"], -1, None, None, None, op),
            "w nan": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T"], bad(ncol, 7, np.nan)[0], None, None, op),
            "w inf": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T"], bad(ncol, 32, -np.inf)[0], None, None, op),
            "center_a nan": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T"], None, bad(180, 179, np.nan)[0], None, op),
            "center_b inf": lambda: lib.ebm_ensemble_covariance(h, F["Ei"], F["T"], None, None, bad(180, 5, np.inf)[0], op),
        }
        says = {"w nan": b"w[7]", "w inf": b"w[32]", "center_a nan": b"center_a[179]", "center_b inf": b"center_b[5]"}
        for name, call in cases.items():
            assert call() == -1, name                                     # EBM_ERR_ARG
            msg = lib.ebm_last_error()
            assert b"ebm_ensemble_covariance" in msg and says.get(name, b"") in msg, (name, msg)
            assert (eng.counters(), {k: eng.field_step(k) for k in MIZ_ALL}, eng.state_conversions()) == state, name
            assert same_bits(eng.ensemble_covariance("Ei", "T"), before), name
        assert lib.ebm_ensemble_covariance(None, F["Ei"], F["T"], None, None, None, op) == -1 and b"null handle" in lib.ebm_last_error()
        # a stale T: the refusal of ebm_hemispheric_mean, with the same steps in the message
        eng.run(first + 2, 3, None, False, 1)
        with pytest.raises(pkg.StaleFieldError) as mine:
            eng.ensemble_covariance("Ei", "T")
        with pytest.raises(pkg.StaleFieldError) as theirs:
            eng.hemispheric_mean("T")
        tail = lambda e: str(e.value).split(": field ", 1)[1]
        assert tail(mine) == tail(theirs) and f"step {first + 1}" in tail(mine) and f"step {first + 4}" in tail(mine)
        assert mine.value.status == -5
        conv = eng.state_conversions()
        phi = eng.ensemble_covariance("phi", "Ei")                        # phi, left underived, is made current first
        assert eng.state_conversions() == conv
        ref, T, n = ensemble_cov_ref(eng.get_field("phi"), eng.get_field("Ei"))
        assert (np.abs(phi - ref) <= covariance_bound(T, n, ncol)).all()


def test_covariance_and_eofs_of_an_ensemble_run(pkg):
    """EnsembleRun.covariance against the NumPy path on the downloaded field, centred on the means the call returns: the
    matrix of sums within the derived bound, then one rounded division.  EnsembleRun.eofs on a rank-2 ensemble whose EOFs are
    known."""
    ncol, nlat = 97, 65
    st = grid(pkg, nlat)
    rng = np.random.default_rng(12)
    k = np.arange(nlat)
    e1, e2 = np.cos(np.pi * k / nlat), (k / nlat) ** 2
    e1, e2 = e1 / np.linalg.norm(e1), (e2 - e2 @ e1 / (e1 @ e1) * e1)
    e2 = e2 / np.linalg.norm(e2)
    s1, s2 = rng.normal(0.0, 3.0, ncol), rng.normal(0.0, 1.0, ncol)
    s2 = s2 - s2.mean()
    s1 = s1 - s1.mean()
    s2 = s2 - (s2 @ s1) / (s1 @ s1) * s1                                  # uncorrelated scores: the EOFs are e1, e2
    T = 10.0 + np.outer(s1, e1) + np.outer(s2, e2)
    phi = rng.uniform(0.0, 1.0, (ncol, nlat))
    run = pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), {n: np.zeros((ncol, nlat)) for n in MIZ_PROG if n != "phi"} | {"phi": phi})
    try:
        run.engine.set_field("T", T)
        for a, b in (("T", None), ("T", "phi")):
            got = run.covariance(a, b)
            xa, xb = T, (T if b is None else phi)
            assert (got["n"] == ncol).all()
            ref, Tij, n = ensemble_cov_ref(xa, xb, None, got["mean_a"], got["mean_b"], same_field=b is None)
            bound = covariance_bound(Tij, n, ncol) / ncol + 2.0 ** -53 * np.abs(ref / ncol)
            assert (np.abs(got["cov"] - ref / ncol) <= bound).all(), (a, b)
            assert np.allclose(got["cov"], np.cov(xa.T, xb.T, bias=True)[:nlat, nlat:], rtol=1e-9, atol=1e-12)
        eof = run.eofs("T", 2)
        for mode, e in zip(eof["modes"], (e1, e2)):
            e = e * np.sign(e[np.argmax(np.abs(e))])
            assert np.allclose(mode, e, atol=1e-9)
        assert np.allclose(eof["variance"], [s1 @ s1 / ncol, s2 @ s2 / ncol], rtol=1e-9) and abs(eof["explained"].sum() - 1.0) < 1e-9
    finally:
        run.close()
