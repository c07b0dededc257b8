"""CPU tests of ebm_run_series (time series of per-column hemispheric means sampled on the device): the symbol in the header,
the library and the bindings; its null-handle refusal without a GPU; the Python argument checks of Engine.run_series and
EnsembleRun.series, which run before any device call."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT
from support import bare_engine


def test_symbol_is_declared_exported_and_bound(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebm_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ebm_run_series\s*\(([^)]*)\)\s*;", hdr)
    assert m, "include/ebm_hip.h does not declare ebm_run_series"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["ebm_handle_t h", "long long first_step", "int nsteps", "const double *f_steps", "int every",
                      "int steps_per_launch", "int nvars", "const int *fields", "double *series"]
    assert len(params) == 9
    assert "ebm_run_series" in pkg.EXPORTS
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "ebm_run_series")
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(_lib.load().ebm_run_series.argtypes) == 9
    assert re.search(r"\bebm_run_series\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_null_handle_is_refused_without_a_gpu(pkg):
    _lib = sys.modules[pkg.__name__ + "._lib"]
    lib = _lib.load()
    fields = (ctypes.c_int * 1)(_lib.FIELD["T"])
    out = np.zeros(8)
    assert lib.ebm_run_series(None, 0, 8, None, 2, 64, 1, fields, _lib.dptr(out)) == -1
    assert b"null argument" in lib.ebm_last_error()


BAD = [
    (dict(every=0), "every = 0"),
    (dict(every=-3), "every = -3"),
    (dict(nsteps=10, every=4), "not a multiple of every"),
    (dict(names=("T", "Q")), "unknown field 'Q'"),
    (dict(names=("Tg",)), "unknown field 'Tg'"),
    (dict(names=("T", "phi", "T")), "listed twice"),
    (dict(names=("T0",)), "unknown field 'T0'"),
    (dict(names=()), "between 1 and"),
    (dict(steps_per_launch=0), "steps_per_launch = 0"),
]


@pytest.mark.parametrize("kw, msg", BAD)
def test_engine_checks_before_the_device(pkg, kw, msg):
    eng = bare_engine(pkg)
    args = dict(first_step=0, nsteps=12, every=4, names=("T", "phi"))
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        eng.run_series(**args)


def test_engine_check_accepts_every_solution_variable(pkg):
    eng = bare_engine(pkg)
    miz = ("Ei", "Ew", "h", "D", "phi", "Tw", "Ti", "n", "E", "T")
    names, ids, f = eng.check_series_args(5, 12, 4, miz, np.zeros(12))
    assert names == miz and ids == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10] and f.shape == (12,)
    assert eng.check_series_args(0, 12, 4, "T")[0] == ("T",)
    classic = bare_engine(pkg, "Classic")
    assert classic.check_series_args(0, 12, 12, ("E", "Tg", "T", "h"))[1] == [9, 11, 10, 2]
    with pytest.raises(ValueError, match="unknown field 'phi'"):
        classic.check_series_args(0, 12, 4, ("phi",))
    with pytest.raises(ValueError, match="shape"):
        eng.check_series_args(0, 12, 4, ("T",), np.zeros(7))


def _bare_run(pkg, step_index=0):
    ensemble = import_module(pkg.__name__ + ".ensemble")
    run = ensemble.EnsembleRun.__new__(ensemble.EnsembleRun)
    run.st = pkg.SpaceTime("sin", 18, 100, 1)
    run.engine = bare_engine(pkg)
    run.has_schedules = False
    run.step_index = step_index
    run.ncol = 3
    return run


@pytest.mark.parametrize("kw, msg", BAD)
def test_ensemble_checks_before_the_device(pkg, kw, msg):
    run = _bare_run(pkg, step_index=40)
    args = dict(nsteps=12, every=4, names=("T", "phi"))
    args.update({k: v for k, v in kw.items() if k != "first_step"})
    with pytest.raises(ValueError, match=msg):
        run.series(**args)
    assert run.step_index == 40
