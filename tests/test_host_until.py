"""CPU tests of ebm_run_until (first passage: step each column until the hemispheric mean of one field crosses its level):
the symbol in the header, the library and the bindings; its null refusals without a GPU; the Python argument checks of
Engine.check_until_args and the level / direction broadcasting of EnsembleRun.first_passage, which run before any device
call; and first_crossing, the NumPy restatement of the header's crossing rule that tests/test_gpu_until.py takes as its
reference, on hand-made series."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT
from support import bare_engine


def first_crossing(series, level, direction):
    """The header's rule on a series m[j][c] of means (sample j = round j + 1): column c crosses at the first sample with
    direction[c] > 0 ? m >= level[c] : m <= level[c] — equality crosses, a NaN never does.  Returns (samples [ncol]: the
    rounds taken, the number of samples if it never crosses; crossed [ncol] bool; value [ncol]: the mean of its last round)."""
    m = np.asarray(series, dtype=np.float64)
    ns, ncol = m.shape
    level, direction = np.asarray(level, dtype=np.float64), np.asarray(direction)
    assert level.shape == direction.shape == (ncol,) and (direction != 0).all() and not np.isnan(level).any()
    with np.errstate(invalid="ignore"):
        hit = np.where(direction[None, :] > 0, m >= level[None, :], m <= level[None, :])      # NaN compares False
    crossed = hit.any(axis=0)
    samples = np.where(crossed, hit.argmax(axis=0) + 1, ns)
    return samples.astype(np.int64), crossed, m[samples - 1, np.arange(ncol)]


# ---- first_crossing on hand-made series ----------------------------------------------------------------------------------

def test_first_crossing_by_hand():
    inf, nan = np.inf, np.nan
    #             up@2   equal  never  first  nan    -inf   +inf   down   down=  nan-then  down+inf  down-inf
    m = np.array([[0.0,  1.0,   0.0,   5.0,   nan,   -3.0,  9e300, 4.0,   4.0,   nan,      7.0,      -9e300],
                  [2.0,  1.5,   0.5,   6.0,   nan,   -4.0,  inf,   3.0,   2.5,   1.0,      8.0,      -inf],
                  [1.0,  2.0,   0.9,   7.0,   nan,   -5.0,  9e300, 1.0,   2.0,   3.0,      9.0,      -9e300]])
    level = np.array([1.5, 2.0, 1.0,   5.0,   0.0,   -inf,  inf,   2.0,   2.0,   2.0,      inf,      -inf])
    direc = np.array([1,   1,   1,     1,     1,     1,     7,     -1,    -1,    1,        -1,       -2])
    samples, crossed, value = first_crossing(m, level, direc)
    assert samples.tolist() == [2, 3, 3, 1, 3, 1, 2, 3, 3, 3, 1, 2]
    assert crossed.tolist() == [True, True, False, True, False, True, True, True, True, True, True, True]
    want = [2.0, 2.0, 0.9, 5.0, nan, -3.0, inf, 1.0, 2.0, 3.0, 7.0, -inf]
    assert np.array_equal(value, np.array(want), equal_nan=True)


def test_first_crossing_equality_is_at_the_bit():
    x = 0.1 + 0.2                                      # 0.30000000000000004
    below = np.nextafter(x, -np.inf)
    m = np.array([[below, below], [x, x], [1.0, 1.0]])
    up = first_crossing(m, np.array([x, np.nextafter(x, np.inf)]), np.array([1, 1]))
    assert up[0].tolist() == [2, 3] and up[1].tolist() == [True, True]
    down = first_crossing(-m, np.array([-x, -np.nextafter(x, np.inf)]), np.array([-1, -1]))
    assert down[0].tolist() == [2, 3]
    # a `>` for `>=` build would pass the level by: the running maximum as level is met at its own sample, not later
    run_max = np.maximum.accumulate(m[:, 0])
    assert first_crossing(m[:, :1], run_max[1:2], np.array([1]))[0].tolist() == [2]


def test_first_crossing_never_and_nan_run_the_whole_series():
    m = np.full((4, 3), np.nan)
    m[:, 1] = [1.0, 2.0, 3.0, 4.0]
    samples, crossed, value = first_crossing(m, np.array([-np.inf, np.inf, np.inf]), np.array([1, 1, -1]))
    assert samples.tolist() == [4, 4, 4] and crossed.tolist() == [False, False, False]
    assert np.isnan(value[0]) and value[1] == 4.0 and np.isnan(value[2])


# ---- the symbol ----------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_exported_and_bound(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebm_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ebm_run_until\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/ebm_hip.h does not declare ebm_run_until"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["ebm_handle_t h", "long long first_step", "int max_samples", "int every", "const double *f_steps",
                      "int steps_per_launch", "int field", "const double *level", "const int *direction", "int *samples",
                      "int *crossed", "double *value"]
    assert "ebm_run_until" in pkg.EXPORTS
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "ebm_run_until")
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(_lib.load().ebm_run_until.argtypes) == 12
    assert re.search(r"\bebm_run_until\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    assert re.search(r"\bebm_run_until\b", open(os.path.join(ROOT, "julia", "EBMHip.jl")).read())


def test_null_arguments_are_refused_without_a_gpu(pkg):
    _lib = sys.modules[pkg.__name__ + "._lib"]
    lib = _lib.load()
    level, direc = np.zeros(2), np.ones(2, dtype=np.int32)
    samples, crossed = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    rc = lib.ebm_run_until(None, 0, 4, 2, None, 64, _lib.FIELD["T"], _lib.dptr(level), direc.ctypes.data_as(ip),
                           samples.ctypes.data_as(ip), crossed.ctypes.data_as(ip), None)
    assert rc == -1
    assert b"ebm_run_until" in lib.ebm_last_error() and b"null argument" in lib.ebm_last_error()


# ---- Engine.check_until_args ---------------------------------------------------------------------------------------------

GOOD = dict(first_step=0, max_samples=4, every=5, name="T", level=[1.0, 2.0, 3.0], direction=[1, -1, 1])
BAD = [
    (dict(every=0), "every = 0"),
    (dict(every=-3), "every = -3"),
    (dict(max_samples=0), "max_samples = 0"),
    (dict(first_step=-1), "first_step"),
    (dict(steps_per_launch=0), "steps_per_launch = 0"),
    (dict(name="Q"), "unknown field 'Q'"),
    (dict(name="Tg"), "unknown field 'Tg'"),
    (dict(name="T0"), "unknown field 'T0'"),
    (dict(name=("T", "phi")), "unknown field"),
    (dict(level=[1.0, np.nan, 3.0]), "level: NaN"),
    (dict(level=[1.0, 2.0]), "shape"),
    (dict(direction=[1, 0, -1]), "direction: 0"),
    (dict(direction=[1, -1]), "direction: expected 3 integers"),
    (dict(direction=[1.0, -1.0, 1.0]), "direction: expected 3 integers"),
    (dict(f_steps=np.zeros(19)), "shape"),
]


@pytest.mark.parametrize("kw, msg", BAD)
def test_engine_checks_before_the_device(pkg, kw, msg):
    eng = bare_engine(pkg)
    args = dict(GOOD)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        eng.run_until(**args)


def test_engine_check_returns_what_the_abi_takes(pkg):
    eng = bare_engine(pkg)
    fid, lev, d, f = eng.check_until_args(7, 4, 5, "phi", [np.inf, -np.inf, 0.25], [5, -2, 1], np.zeros(20), 1)
    assert fid == 4 and f.shape == (20,)
    assert lev.dtype == np.float64 and lev.tolist() == [np.inf, -np.inf, 0.25]
    assert d.dtype == np.int32 and d.flags.c_contiguous and d.tolist() == [1, -1, 1]
    for name, want in (("Ei", 0), ("Ti", 7), ("T", 10), ("E", 9)):
        assert eng.check_until_args(0, 1, 1, name, np.zeros(3), np.ones(3, dtype=np.int64))[0] == want
    classic = bare_engine(pkg, "Classic")
    assert classic.check_until_args(0, 1, 1, "Tg", np.zeros(3), np.ones(3, dtype=np.int64))[0] == 11
    with pytest.raises(ValueError, match="unknown field 'phi'"):
        classic.check_until_args(0, 1, 1, "phi", np.zeros(3), np.ones(3, dtype=np.int64))


# ---- EnsembleRun.first_passage -------------------------------------------------------------------------------------------

def test_levels_and_directions_broadcast(pkg):
    ensemble = import_module(pkg.__name__ + ".ensemble")
    lev, d = ensemble.passage_levels(3, 1.5, "up")
    assert lev.tolist() == [1.5] * 3 and d.tolist() == [1, 1, 1] and d.dtype == np.int32
    lev, d = ensemble.passage_levels(3, [1.0, np.inf, -np.inf], ["down", "up", -1])
    assert lev.tolist() == [1.0, np.inf, -np.inf] and d.tolist() == [-1, 1, -1]
    assert ensemble.passage_levels(2, 0.0, -7)[1].tolist() == [-1, -1]
    assert ensemble.passage_levels(2, 0.0, np.array([3, -3]))[1].tolist() == [1, -1]
    assert ensemble.passage_levels(1, [2.0], ["down"])[1].tolist() == [-1]
    for level, direction, msg in [(np.nan, "up", "level: NaN"), ([1.0, 2.0], "up", "level: expected"),
                                  (np.zeros((3, 1)), "up", "level: expected"), (0.0, "sideways", "neither 'up' nor 'down'"),
                                  (0.0, 0, "neither"), (0.0, 1.0, "neither"), (0.0, True, "neither"),
                                  (0.0, ["up", "down"], "direction: expected a scalar or 3")]:
        with pytest.raises(ValueError, match=msg):
            ensemble.passage_levels(3, level, direction)


def _bare_run(pkg, step_index=0):
    ensemble = import_module(pkg.__name__ + ".ensemble")
    run = ensemble.EnsembleRun.__new__(ensemble.EnsembleRun)
    run.st = pkg.SpaceTime("sin", 18, 100, 1)
    run.engine = bare_engine(pkg)
    run.has_schedules = False
    run.step_index = step_index
    run.ncol = 3
    return run


@pytest.mark.parametrize("kw, msg", [
    (dict(every=0), "every = 0"),
    (dict(max_steps=10, every=4), "not a positive multiple of every"),
    (dict(max_steps=0), "not a positive multiple of every"),
    (dict(name="T0"), "unknown field 'T0'"),
    (dict(level=np.nan), "level: NaN"),
    (dict(direction="left"), "neither 'up' nor 'down'"),
    (dict(direction=[1, 0, 1]), "neither"),
    (dict(steps_per_launch=0), "steps_per_launch = 0"),
])
def test_ensemble_checks_before_the_device(pkg, kw, msg):
    run = _bare_run(pkg, step_index=40)
    args = dict(max_steps=12, every=4, name="T", level=1.0, direction="up")
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        run.first_passage(**args)
    assert run.step_index == 40


def test_ensemble_first_passage_steps_and_times(pkg):
    """The arithmetic around the engine call, with the engine's answer given: first-passage step and model time."""
    run = _bare_run(pkg, step_index=40)
    seen = {}

    def run_until(first, rounds, every, name, lev, d, f, K):
        seen.update(first=first, rounds=rounds, every=every, name=name, lev=lev.tolist(), d=d.tolist(), f=f, K=K)
        samples = np.array([1, 3, 2])
        return dict(samples=samples, crossed=np.array([True, False, True]), value=np.array([0.5, 0.1, 0.7]), steps=3 * every)
    run.engine.run_until = run_until
    out = run.first_passage(12, 4, "phi", level=[0.5, 0.6, 0.7], direction="down", forcing=lambda t: 2.0 * t)
    assert seen["first"] == 40 and seen["rounds"] == 3 and seen["every"] == 4 and seen["name"] == "phi" and seen["K"] == 64
    assert seen["lev"] == [0.5, 0.6, 0.7] and seen["d"] == [-1, -1, -1]
    assert np.array_equal(seen["f"], 2.0 * (np.arange(40, 52) + 0.5) * run.st.dt)
    assert run.step_index == 52
    assert out["step"].tolist() == [43, -1, 47] and out["crossed"].tolist() == [True, False, True]
    assert out["time"][0] == 43.5 * run.st.dt and np.isnan(out["time"][1]) and out["time"][2] == 47.5 * run.st.dt
    assert out["samples"].tolist() == [1, 3, 2] and out["value"].tolist() == [0.5, 0.1, 0.7]
