"""CPU tests of ebm_resample_columns (resampling ensemble members on the device): the symbol in the header, the library and
the bindings and its null refusals without a GPU; selection_parents (systematic resampling); Engine.check_resample_args,
which runs before any device call; and the host side of the genealogical cloning algorithm (gklt_run, gklt_lineage,
gklt_estimate — the functions examples/rare_transitions_gklt.py runs on the GPU ensemble) on a toy AR(1) process in NumPy."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT
from support import bare_engine


# ---- the symbol ----------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_exported_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert "RESAMPLE" in hdr and hdr.count("THIS TEXT IS THE DEFINITION") >= 5
    m = re.search(r"\bint\s+ebm_resample_columns\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert m, "include/ebm_hip.h does not declare ebm_resample_columns"
    assert [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")] == ["ebm_handle_t h", "const int *parent"]
    assert "ebm_resample_columns" in pkg.EXPORTS
    assert hasattr(ctypes.CDLL(pkg.LIB_PATH), "ebm_resample_columns")
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(_lib.load().ebm_resample_columns.argtypes) == 2
    assert re.search(r"\bebm_resample_columns\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert re.search(r"\(:ebm_resample_columns, libebm\)", open(os.path.join(ROOT, "julia", "EBMHip.jl")).read())


def test_null_arguments_are_refused_without_a_gpu(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    parent = np.zeros(2, dtype=np.int32)
    assert lib.ebm_resample_columns(None, parent.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == -1
    assert b"ebm_resample_columns" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()


# ---- selection_parents ---------------------------------------------------------------------------------------------------

def offspring(parents, n):
    return np.bincount(parents, minlength=n)


def test_selection_offspring_counts_are_floor_or_ceil(pkg):
    """Systematic resampling: member m has floor(n w_m) or ceil(n w_m) offspring, whatever the one uniform draw is.  200
    weight vectors with a fixed seed: lengths 1 .. 300, weights spread over up to six decades, some members at 0."""
    rng = np.random.default_rng(2024)
    for trial in range(200):
        n = int(rng.integers(1, 301))
        w = np.exp(rng.uniform(-7.0, 7.0) * rng.random(n))
        w[rng.random(n) < 0.1 * (trial % 3)] = 0.0
        if w.max() == 0.0:
            w[0] = 1.0
        p = pkg.selection_parents(w, rng)
        assert p.dtype == np.int32 and p.shape == (n,)
        assert (np.diff(p) >= 0).all(), "ascending"
        x = n * (w / w.sum())
        k = offspring(p, n)
        assert k.sum() == n
        assert ((k == np.floor(x)) | (k == np.ceil(x))).all(), (trial, np.flatnonzero((k != np.floor(x)) & (k != np.ceil(x))))
        assert (k[w == 0.0] == 0).all(), "a member of weight 0 has no offspring"


def test_selection_equal_weights_give_the_identity(pkg):
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 64, 1000):
        for value in (1.0, 0.1, 3e-300, 7e300 / n):
            assert np.array_equal(pkg.selection_parents(np.full(n, value), rng), np.arange(n)), (n, value)


def test_selection_zero_weight_members_die_and_the_rest_share(pkg):
    class Fixed:
        def __init__(self, u):
            self.u = u

        def random(self):
            return self.u
    w = np.array([0.0, 1.0, 0.0, 3.0, 0.0])
    for u in (0.0, 0.25, 0.5, np.nextafter(1.0, 0.0)):
        p = pkg.selection_parents(w, Fixed(u))
        k = offspring(p, 5)
        assert k[0] == k[2] == k[4] == 0 and k[1] in (1, 2) and k[3] in (3, 4) and k.sum() == 5, (u, p)
        assert (np.diff(p) >= 0).all()
    # by hand: n = 4, cumulative weights scaled to 4 are 0.4, 1.2, 4 (the last live member takes the rest); pointers u + j
    assert pkg.selection_parents(np.array([1.0, 2.0, 7.0, 0.0]), Fixed(0.3)).tolist() == [0, 2, 2, 2]
    assert pkg.selection_parents(np.array([1.0, 2.0, 7.0, 0.0]), Fixed(0.5)).tolist() == [1, 2, 2, 2]


@pytest.mark.parametrize("weights, msg", [([1.0, -0.5], ">= 0"), ([1.0, np.nan], "finite"), ([np.inf, 1.0], "finite"),
                                          ([0.0, 0.0, 0.0], "all zero"), ([], "at least one"), ([[1.0, 2.0]], "vector")])
def test_selection_refusals(pkg, weights, msg):
    with pytest.raises(ValueError, match=msg):
        pkg.selection_parents(np.array(weights, dtype=np.float64), np.random.default_rng(0))


# ---- Engine.check_resample_args ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("parents, msg", [
    ([0, 1], "expected 3 integers"),
    ([0, 1, 2, 0], "expected 3 integers"),
    ([[0, 1, 2]], "expected 3 integers"),
    ([0.0, 1.0, 2.0], "dtype float64"),
    (np.array([True, False, True]), "dtype bool"),
    ([0, -1, -2], r"parents\[1\] = -1 is outside \[0, 3\)"),
    ([0, 1, 3], r"parents\[2\] = 3 is outside \[0, 3\)"),
])
def test_engine_checks_before_the_device(pkg, parents, msg):
    eng = bare_engine(pkg)                               # its library refuses every call: a device call fails the test
    with pytest.raises(ValueError, match=msg):
        eng.resample_columns(parents)


def test_engine_check_returns_what_the_abi_takes(pkg):
    eng = bare_engine(pkg)
    for given in ([2, 0, 0], np.array([2, 0, 0], dtype=np.int64), np.array([2, 0, 0], dtype=np.uint8), np.array([9, 2, 9, 0, 9, 0])[1::2]):
        p = eng.check_resample_args(given)
        assert p.dtype == np.int32 and p.flags.c_contiguous and p.tolist() == [2, 0, 0]


def test_ensemble_resample_is_the_engine_call_and_keeps_the_step_index(pkg):
    ensemble = import_module(pkg.__name__ + ".ensemble")
    run = ensemble.EnsembleRun.__new__(ensemble.EnsembleRun)
    run.engine, run.step_index, run.ncol = bare_engine(pkg), 40, 3
    with pytest.raises(ValueError, match="outside"):
        run.resample([0, 1, 7])
    seen = []
    run.engine.resample_columns = lambda p: seen.append(list(p))
    run.resample([2, 2, 0])
    assert seen == [[2, 2, 0]] and run.step_index == 40
    assert "rank-local" in ensemble.EnsembleRun.resample.__doc__


# ---- the GKLT estimator on a toy process ---------------------------------------------------------------------------------

class Toy:
    """n members of the AR(1) process x <- a x + s xi, `every` steps per interval; the score of an interval is the time
    integral of x over it, the tracked value the lowest x seen in it.  The innovations come from the toy's own generator,
    one row per step for all slots: a clone draws its own noise after the selection."""

    def __init__(self, n, every=5, seed=3):
        self.x = np.zeros(n)
        self.rng = np.random.default_rng(seed)
        self.every, self.dt = every, 0.1
        self.low = []

    def advance(self, i):
        score, low = np.zeros_like(self.x), np.full_like(self.x, np.inf)
        for _ in range(self.every):
            self.x = 0.9 * self.x + 0.5 * self.rng.standard_normal(self.x.shape[0])
            score += self.x * self.dt
            low = np.minimum(low, self.x)
        self.low.append(low)
        return score

    def resample(self, parents):
        self.x = self.x[parents]


def run_toy(pkg, k, n=200, nint=8, seed=3):
    toy = Toy(n, seed=seed)
    out = pkg.gklt_run(toy.advance, toy.resample, n, nint, k, np.random.default_rng(9))
    acc = pkg.gklt_lineage(out["parents"], out["scores"])
    low = pkg.gklt_lineage(out["parents"], np.array(toy.low), np.minimum)
    return out, acc, low


def test_lineage_by_hand(pkg):
    parents = np.array([[0, 0, 2], [1, 1, 2]])            # interval 0 then 1: the final slots 0, 1 descend 1 <- 0, slot 2 <- 2 <- 2
    values = np.array([[1.0, 2.0, 4.0], [10.0, 20.0, 40.0]])
    assert pkg.gklt_lineage(parents, values).tolist() == [21.0, 21.0, 44.0]
    assert pkg.gklt_lineage(parents, values, np.minimum).tolist() == [1.0, 1.0, 4.0]


@pytest.mark.parametrize("k", [-3.0, -0.5, 0.0, 0.7, 40.0])
def test_the_estimate_of_one_is_one(pkg, k):
    """The normalisation identity of the self-normalised estimator: sum(1 * u) / sum(u).  Numerator and denominator are
    the same floating-point sum of the same array, so the bound is one rounding of the quotient — also where exp(-k A)
    would overflow without the shift by its largest exponent (k = 40)."""
    out, acc, low = run_toy(pkg, k)
    est = pkg.gklt_estimate(np.ones_like(acc), acc, k, out["log_norm"])
    print(f"k = {k}: estimate of 1 = {est['estimate']!r}, raw norm = {est['norm']:.4f}, ess = {est['ess']:.1f}")
    assert abs(est["estimate"] - 1.0) <= np.finfo(np.float64).eps
    assert np.isfinite(est["norm"]) and est["norm"] > 0.0 and 1.0 <= est["ess"] <= len(acc) * (1 + 1e-12)
    if k != 0.0:
        assert (out["parents"] != np.arange(len(acc))).any(), "honesty: the tilt selected"


def test_without_tilt_it_is_the_plain_sample_mean(pkg):
    """k = 0: every weight is 1, every parents row the identity, and the estimate is np.mean of the observable over the
    members of the direct run, bit for bit."""
    out, acc, low = run_toy(pkg, 0.0)
    assert (out["parents"] == np.arange(out["parents"].shape[1])).all() and out["log_norm"] == 0.0
    direct = Toy(200, seed=3)
    lows = np.array([(direct.advance(i), direct.low[-1])[1] for i in range(8)]).min(axis=0)
    assert np.array_equal(low, lows)
    obs = (low < -1.5).astype(np.float64)
    est = pkg.gklt_estimate(obs, acc, 0.0, out["log_norm"])
    assert 0.0 < obs.mean() < 1.0, "honesty: the event happens to some members"
    assert est["estimate"] == float(np.mean(obs)) and est["norm"] == 1.0 and est["ess"] == 200.0
    x = low * 1.2345                                       # and of an observable that is not 0 / 1
    assert pkg.gklt_estimate(x, acc, 0.0)["estimate"] == float(np.mean(x))


def test_the_example_uses_these_functions():
    src = open(os.path.join(ROOT, "examples", "rare_transitions_gklt.py")).read()
    for name in ("gklt_run", "gklt_lineage", "gklt_estimate", "run.series(", "run.resample"):
        assert name in src, name
