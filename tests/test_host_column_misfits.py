"""CPU tests of the per-member misfits (ebm_column_misfits): the NumPy restatement of the definition against exact sums, the
contribution rules on hand-made arrays, the arithmetic from misfits to particle-filter weights (assimilation_weights), the
host-side argument checks of Engine.column_misfits, and the symbols in the header, the library and the bindings.

The bound is derived, not fitted.  A term is d = x - y, t1 = r d, t2 = t1 d: three roundings, so the float64 term is within
3 2^-53 |term| of the exact r (x - y)^2, to first order.  A chain adds at most nvars ceil(U / 64) terms, U = ceil(nlat / 2);
the parity add and the six steps of the tree are seven more rounded adds.  Hence, against the exact sum of the exact terms
(rational arithmetic: what math.fsum of them would round, without that last rounding),
    |restatement - exact| <= (nvars ceil(U / 64) + 10) 2^-53 sum|terms|."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from column_misfits_ref import column_misfits_fast, column_misfits_ref, rounds_of, same_bits
from conftest import ROOT

NAMES = ("ebm_column_misfits", "ebm_column_misfits_device")


def benign(nvars, ncol, nlat, ntargets, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (nvars, ncol, nlat)) * 2.0 ** rng.integers(-3, 4, (nvars, ncol, nlat))
    x[rng.random(x.shape) < 0.05] = np.nan
    y = rng.normal(0.0, 1.0, (ntargets, nvars, nlat))
    y[rng.random(y.shape) < 0.1] = np.nan
    r = rng.uniform(0.1, 3.0, (nvars, nlat))
    r[rng.random(r.shape) < 0.2] = 0.0
    return x, y, r


def exact_misfits(x, y, r):
    """J as a Fraction, the sum of |terms| as a Fraction, and N, per (target, column): exact terms, exact sums."""
    nvars, ncol, nlat = x.shape
    J = [[Fraction(0)] * ncol for _ in range(y.shape[0])]
    A = [[Fraction(0)] * ncol for _ in range(y.shape[0])]
    N = np.zeros((y.shape[0], ncol))
    for t in range(y.shape[0]):
        for c in range(ncol):
            for v in range(nvars):
                for k in range(nlat):
                    if r[v, k] == 0.0 or math.isnan(y[t, v, k]) or math.isnan(x[v, c, k]):
                        continue
                    d = Fraction(x[v, c, k]) - Fraction(y[t, v, k])
                    J[t][c] += Fraction(r[v, k]) * d * d
                    N[t, c] += 1
            A[t][c] = J[t][c]                            # every term is >= 0: the sum of the magnitudes is the sum
    return J, A, N


@pytest.mark.parametrize("nvars, ncol, nlat, ntargets", [(3, 3, 2, 2), (2, 3, 130, 2), (2, 2, 4096, 1), (1, 2, 5, 1), (4, 2, 181, 3)])
def test_restatement_against_exact_sums(nvars, ncol, nlat, ntargets):
    x, y, r = benign(nvars, ncol, nlat, ntargets, 17 * nlat + nvars)
    assert rounds_of(2) == 1 and rounds_of(128) == 1 and rounds_of(129) == 2 and rounds_of(130) == 2 and rounds_of(4096) == 32
    for rr in (None, r):
        got = column_misfits_ref(x, y, rr)
        J, A, N = exact_misfits(x, y, np.ones((nvars, nlat)) if rr is None else rr)
        assert np.array_equal(got[:, 1], N)
        factor = Fraction(nvars * rounds_of(nlat) + 10) / Fraction(2 ** 53)
        worst = 0.0
        for t in range(ntargets):
            for c in range(ncol):
                err, bound = abs(Fraction(got[t, 0, c]) - J[t][c]), factor * A[t][c]
                worst = max(worst, float(err / bound) if bound else 0.0)
                assert err <= bound, (t, c, float(err), float(bound))
        print(f"nvars {nvars} nlat {nlat} rw {'given' if rr is not None else 'none'}: worst error / bound = {worst:.3f}")
        fast = column_misfits_fast(x, y, rr)
        assert np.array_equal(fast[:, 1], N) and np.allclose(fast[:, 0], got[:, 0], rtol=1e-12)


def test_restatement_order_is_the_definitions():
    """Terms that the order of the adds sorts out.  A big term 1.0 and two small terms s = 0.75 2^-53 (x = 2^-27, rw = 1.5:
    exact): added to the 1.0 one by one they vanish, (1 + s) + s == 1; if they meet first, 1 + (s + s) == 1 + 2^-52.  One
    variable, 256 cells, target 0."""
    def J(big, small, nlat=256):
        x, r = np.zeros((1, 1, nlat)), np.ones((1, nlat))
        x[0, 0, big] = 1.0
        for k in small:
            x[0, 0, k], r[0, k] = 2.0 ** -27, 1.5
        return column_misfits_ref(x, np.zeros((1, 1, nlat)), r)[0, 0, 0]
    one_by_one, met_first = 1.0, 1.0 + 2.0 ** -52
    assert J(0, (128, 1)) == one_by_one, "cell 128 joins chain (0, 0) after cell 0; chain (0, 1) joins in the parity add"
    assert J(128, (0, 1)) == one_by_one, "ascending i within the chain: s, then 1, then the other parity's s"
    assert J(1, (0, 128)) == met_first, "the two cells of chain (0, 0) meet before the parity add"
    assert J(0, (2, 3)) == met_first, "the parity add of lane 1 comes before the tree"
    assert J(0, (64, 96)) == one_by_one, "s = 32 adds lane 32 to lane 0, lane 48 to lane 16; s = 16 adds lane 16 to lane 0"
    assert J(0, (32, 96)) == met_first, "lanes 16 and 48 meet at s = 32"
    assert J(0, (2, 4)) == one_by_one, "s = 2 adds lane 2 to lane 0, s = 1 lane 1"
    assert J(0, (4, 12)) == met_first, "lanes 2 and 6 meet at s = 4"
    # one accumulator runs across the variables: the small terms of two variables at one cell meet in their chain
    x, r = np.zeros((2, 1, 2)), np.full((2, 2), 1.5)
    x[0, 0, 0] = x[1, 0, 0] = 2.0 ** -27
    x[0, 0, 1], r[0, 1] = 1.0, 1.0
    assert column_misfits_ref(x, np.zeros((1, 2, 2)), r)[0, 0, 0] == met_first
    x[1, 0, 0], x[1, 0, 1] = 0.0, 2.0 ** -27             # ... and the one of variable 1 joins what variable 0 left in chain (0, 1)
    assert column_misfits_ref(x, np.zeros((1, 2, 2)), r)[0, 0, 0] == one_by_one


def test_contribution_rules():
    """NaN in x, NaN in the target, rw = 0 do not contribute; +Inf propagates; -0.0 is a value like any other; no contributor
    gives J = 0.0, N = 0.0."""
    x = np.array([[[1.0, np.nan, 3.0, -0.0, 5.0], [np.inf, 2.0, np.nan, 4.0, np.nan], [np.nan] * 5]])      # [1, 3, 5]
    y = np.array([[[0.0, 0.0, np.nan, 0.0, 1.0]], [[np.nan] * 5]])                                         # [2, 1, 5]
    out = column_misfits_ref(x, y)
    assert out[0, 1].tolist() == [3.0, 3.0, 0.0] and out[0, 0].tolist() == [1.0 + 0.0 + 16.0, np.inf, 0.0]
    assert out[1].tolist() == [[0.0] * 3, [0.0] * 3], "a target without an observation"
    assert not np.signbit(out[0, 0, 2]) and not np.signbit(out[1, 0, 0])
    r = np.array([[0.0, 2.0, 1.0, 0.5, 0.0]])
    out = column_misfits_ref(x, y, r)
    assert out[0, 1].tolist() == [1.0, 2.0, 0.0] and out[0, 0].tolist() == [0.0, 2.0 * 4.0 + 0.5 * 16.0, 0.0]
    assert np.isfinite(out).all(), "rw = 0 hides the Inf cell"
    # -0.0 against a target of -0.0 and of +0.0: d = 0, the term is +0.0 and it counts
    out = column_misfits_ref(np.array([[[-0.0, -0.0]]]), np.array([[[-0.0, 0.0]]]))
    assert out[0, 0, 0] == 0.0 and not np.signbit(out[0, 0, 0]) and out[0, 1, 0] == 2.0
    # -Inf as well, and Inf against a NaN target is no contributor
    out = column_misfits_ref(np.array([[[-np.inf, np.inf]]]), np.array([[[1.0, np.nan]], [[np.nan, np.nan]]]))
    assert out[0, 0, 0] == np.inf and out[0, 1, 0] == 1.0 and out[1, 0, 0] == 0.0 and out[1, 1, 0] == 0.0


def test_assimilation_weights(pkg):
    aw = pkg.assimilation_weights
    for n in (1, 3, 7, 64):
        r = aw(np.full(n, 12.5))
        assert r["weights"].tolist() == [1.0 / n] * n and r["ess"] == float(n)
        assert r["log_evidence"] == pytest.approx(-6.25, abs=1e-12)
    J = np.full(9, 2000.0)
    J[4] = 0.0
    r = aw(J)
    assert r["weights"][4] == 1.0 and (np.delete(r["weights"], 4) == 0.0).all() and not np.isnan(r["weights"]).any()
    assert r["ess"] == 1.0 and r["log_evidence"] == pytest.approx(-math.log(9.0), abs=1e-12)
    # far from the observation everywhere: still normalised, no NaN
    r = aw(np.array([4000.0, 4002.0, np.inf]))
    assert r["weights"][2] == 0.0 and r["weights"].sum() == pytest.approx(1.0) and r["weights"][0] == pytest.approx(1.0 / (1.0 + math.exp(-1.0)))
    assert r["log_evidence"] == pytest.approx(-2000.0 + math.log((1.0 + math.exp(-1.0)) / 3.0))
    # a prior is honoured: equal likelihoods return the normalised prior; -inf in the prior is a dead member
    prior = np.log(np.array([1.0, 2.0, 5.0]))
    r = aw(np.full(3, 3.0), prior)
    assert np.allclose(r["weights"], [0.125, 0.25, 0.625], rtol=1e-15) and r["log_evidence"] == pytest.approx(-1.5)
    r = aw(np.array([0.0, 2.0 * math.log(2.0)]), np.array([0.0, math.log(2.0)]))       # likelihoods 1 and 1/2, prior 1 : 2
    assert np.allclose(r["weights"], [0.5, 0.5]) and r["ess"] == pytest.approx(2.0)
    assert r["log_evidence"] == pytest.approx(math.log((1.0 * 1.0 + 2.0 * 0.5) / 3.0))
    r = aw(np.array([0.0, 0.0]), np.array([-np.inf, 0.0]))
    assert r["weights"].tolist() == [0.0, 1.0]
    for bad in (lambda: aw([]), lambda: aw([1.0, np.nan]), lambda: aw([1.0, -1.0]), lambda: aw([1.0], [0.0, 0.0]),
                lambda: aw([np.inf, np.inf]), lambda: aw([1.0, 2.0], [np.nan, 0.0]), lambda: aw([1.0, 2.0], [np.inf, 0.0])):
        with pytest.raises(ValueError):
            bad()


def test_assimilate_weighs_resamples_and_reports(pkg):
    """EnsembleRun.assimilate with a stand-in for the engine: rw = quad / obs_var reaches the reduction, the weights are those
    of assimilation_weights, and the ensemble is resampled exactly when the effective sample size is below the fraction."""
    nlat, ncol = 6, 5
    rng = np.random.default_rng(4)
    T = rng.normal(0.0, 1.0, (ncol, nlat))
    obs = T[2] + 0.01
    obs[::2] = np.nan

    class Standin:
        def __init__(self):
            self.calls = []

        def column_misfits(self, names, targets, rweights=None):
            self.calls.append((tuple(names) if not isinstance(names, str) else names, rweights.copy()))
            return column_misfits_ref(T[None], np.asarray(targets).reshape(1, 1, nlat), rweights)

    class St:
        nx = nlat
    run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
    run.engine, run.ncol, run.st, moved = Standin(), ncol, St(), []
    run.resample = lambda parents: moved.append(np.asarray(parents).copy())
    quad = np.linspace(0.5, 1.0, nlat)
    res = run.assimilate("T", obs[None], 0.04, np.random.default_rng(1), quad=quad, ess_fraction=0.9)
    assert np.array_equal(run.engine.calls[0][1], (quad / 0.04)[None])
    want = column_misfits_ref(T[None], obs[None, None], (quad / 0.04)[None])
    assert same_bits(res["J"], want[0, 0]) and (res["N"] == 3.0).all()
    w = pkg.assimilation_weights(want[0, 0])
    assert np.array_equal(res["weights"], w["weights"]) and res["ess"] == w["ess"] and res["log_evidence"] == w["log_evidence"]
    assert res["weights"].argmax() == 2 and res["ess"] < 0.9 * ncol
    assert len(moved) == 1 and np.array_equal(moved[0], res["parents"]) and (np.bincount(res["parents"], minlength=ncol)[2] >= 1)
    res = run.assimilate("T", obs[None], 1e6, np.random.default_rng(1), ess_fraction=0.5)      # a useless observation: equal weights
    assert res["parents"] is None and len(moved) == 1 and res["ess"] > 0.99 * ncol
    with pytest.raises(ValueError):
        run.assimilate("T", obs[None], 0.0, np.random.default_rng(1))
    with pytest.raises(ValueError):
        run.assimilate("T", obs[None], 1.0, np.random.default_rng(1), ess_fraction=1.5)


def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert "PER-MEMBER MISFITS TO TARGET PROFILES" in hdr and hdr.count("THIS TEXT IS THE DEFINITION") >= 11
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    julia = open(os.path.join(ROOT, "julia", "EBMHip.jl")).read()
    protos = {}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, bare)
        assert m, f"include/ebm_hip.h does not declare {name}"
        protos[name] = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert name in pkg.EXPORTS and hasattr(cdll, name)
        assert len(getattr(lib, name).argtypes) == 7, name
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name
    assert protos[NAMES[0]][:6] == protos[NAMES[1]][:6] == ["ebm_handle_t h", "int nvars", "const int *fields", "int ntargets",
                                                            "const double *target", "const double *rw"]
    assert protos[NAMES[0]][6] == "double *out" and protos[NAMES[1]][6] == "double *dev_out"
    C = ctypes
    dp = C.POINTER(C.c_double)
    assert lib.ebm_column_misfits.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, dp, dp, dp]
    assert lib.ebm_column_misfits_device.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, dp, dp, C.c_void_p]
    for name in ("misfits", "misfits_tensor", "assimilate"):
        assert callable(getattr(pkg.EnsembleRun, name)), name
    for name in ("column_misfits", "column_misfits_device"):
        assert callable(getattr(pkg.Engine, name)), name
    for doc in ("README.md", "DESIGN.md"):
        assert "ebm_column_misfits" in open(os.path.join(ROOT, doc)).read(), doc


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    f = (ctypes.c_int * 1)(10)
    y, out = np.zeros(4), np.zeros(2)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.ebm_column_misfits(None, 1, f, 1, y.ctypes.data_as(dp), None, out.ctypes.data_as(dp)) == -1
    assert lib.ebm_last_error() == b"ebm_column_misfits: null handle"
    assert lib.ebm_column_misfits_device(None, 1, f, 1, y.ctypes.data_as(dp), None, ctypes.c_void_p(16)) == -1
    assert lib.ebm_last_error() == b"ebm_column_misfits_device: null handle"


def test_engine_checks_raise_before_any_device_call(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)               # no handle: a device call would fail on the missing attributes
    eng.ncol, eng.nlat, eng.model = 5, 4, "MIZ"

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    eng.lib, eng._h = NoCalls(), None
    ok_y, ok_r = np.zeros((3, 2, 4)), np.ones((2, 4))

    def with_value(a, index, value):
        a = a.copy()
        a[index] = value
        return a
    for names, y, r in (((), ok_y, None), (("T", "T"), ok_y, None), (("T0", "T"), ok_y, None), (("Tg", "T"), ok_y, None),
                        (("T", "phi"), np.zeros((3, 2, 5)), None), (("T", "phi"), np.zeros((3, 1, 4)), None),
                        (("T", "phi"), np.zeros((9, 2, 4)), None), (("T", "phi"), np.zeros((0, 2, 4)), None),
                        (("T", "phi"), np.zeros(4), None), (("T", "phi"), with_value(ok_y, (2, 1, 3), np.inf), None),
                        (("T", "phi"), with_value(ok_y, (0, 0, 0), -np.inf), None), (("T", "phi"), ok_y, np.ones((1, 4))),
                        (("T", "phi"), ok_y, with_value(ok_r, (1, 2), -1.0)), (("T", "phi"), ok_y, with_value(ok_r, (0, 0), np.nan)),
                        (("T", "phi"), ok_y, with_value(ok_r, (0, 0), np.inf))):
        with pytest.raises(ValueError):
            eng.column_misfits(names, y, r)
    with pytest.raises(ValueError, match=r"targets\[2\]\[1\]\[3\]"):
        eng.column_misfits(("T", "phi"), with_value(ok_y, (2, 1, 3), np.inf))
    with pytest.raises(ValueError, match=r"rweights\[1\]\[2\]"):
        eng.column_misfits(("T", "phi"), ok_y, with_value(ok_r, (1, 2), -1.0))
    with pytest.raises(ValueError, match="dev_ptr"):
        eng.column_misfits_device(("T", "phi"), ok_y, 0, ok_r)
    names, ids, y, r = eng._check_misfit_args("T", with_value(np.zeros((1, 4)), (0, 1), np.nan), [[0, 1, 2, 0]])
    assert names == ("T",) and ids == [10] and y.shape == (1, 1, 4) and np.isnan(y[0, 0, 1]) and r.dtype == np.float64
    names, ids, y, r = eng._check_misfit_args(("T", "phi"), ok_y[0])
    assert y.shape == (1, 2, 4) and r is None, "a single target may be given as [nvars, nlat]"
