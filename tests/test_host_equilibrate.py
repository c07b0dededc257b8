"""CPU tests of ebm_equilibrate (step each column until its seasonal cycle repeats): the symbol in the header, the library
and the bindings; its null-handle refusal without a GPU; the Python argument checks of Engine.equilibrate and
EnsembleRun.equilibrate, which run before any device call."""
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
    assert re.search(r"\bint\s+ebm_equilibrate\s*\(\s*ebm_handle_t\s+h\s*,\s*int\s+nt\s*,\s*int\s+max_years\s*,\s*int\s+min_years\s*,"
                     r"\s*const\s+double\s*\*\s*f_year\s*,\s*int\s+nvars\s*,\s*const\s+int\s*\*\s*fields\s*,"
                     r"\s*const\s+double\s*\*\s*tol\s*,\s*int\s*\*\s*years\s*,\s*int\s*\*\s*converged\s*,"
                     r"\s*double\s*\*\s*resid\s*\)\s*;", hdr)
    assert "ebm_equilibrate" in pkg.EXPORTS
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "ebm_equilibrate")
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(_lib.load().ebm_equilibrate.argtypes) == 11
    assert re.search(r"\bebm_equilibrate\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_null_handle_is_refused_without_a_gpu(pkg):
    _lib = sys.modules[pkg.__name__ + "._lib"]
    lib = _lib.load()
    fields = (ctypes.c_int * 1)(_lib.FIELD["T"])
    tol = np.array([1e-3])
    years = (ctypes.c_int * 4)()
    conv = (ctypes.c_int * 4)()
    assert lib.ebm_equilibrate(None, 10, 5, 2, None, 1, fields, _lib.dptr(tol), years, conv, None) == -1
    assert b"bad argument" in lib.ebm_last_error()


@pytest.mark.parametrize("kw, exc, msg", [
    (dict(tol={"T0": 1e-3}), ValueError, "unknown field 'T0'"),
    (dict(tol={"Tg": 1e-3}), ValueError, "unknown field 'Tg'"),
    (dict(tol={"T": -1e-3}), ValueError, "must be >= 0"),
    (dict(tol={"T": float("nan")}), ValueError, "must be >= 0"),
    (dict(tol={}), ValueError, "expected a dict"),
    (dict(tol=[1e-3]), ValueError, "expected a dict"),
    (dict(max_years=0), ValueError, "max_years = 0"),
    (dict(f_year=np.zeros(7)), ValueError, "shape"),
])
def test_engine_checks_before_the_device(pkg, kw, exc, msg):
    eng = bare_engine(pkg)
    args = dict(nt=10, max_years=5, tol={"T": 1e-3})
    args.update(kw)
    with pytest.raises(exc, match=msg):
        eng.equilibrate(**args)


def test_engine_check_accepts_every_solution_variable(pkg):
    eng = bare_engine(pkg)
    names, ids, tols, f = eng.check_equilibrate_args(10, 3, {"Ei": 0.0, "T": 1e-3, "n": 2.0}, 2, np.zeros(10))
    assert names == ("Ei", "T", "n") and ids == [0, 10, 8] and list(tols) == [0.0, 1e-3, 2.0] and f.shape == (10,)
    classic = bare_engine(pkg, "Classic")
    assert classic.check_equilibrate_args(10, 3, {"E": 1.0, "Tg": 1.0, "T": 1.0, "h": 1.0})[1] == [9, 11, 10, 2]
    with pytest.raises(ValueError, match="unknown field 'phi'"):
        classic.check_equilibrate_args(10, 3, {"phi": 1.0})


def _bare_run(pkg, schedules=False, step_index=0):
    ensemble = import_module(pkg.__name__ + ".ensemble")
    run = ensemble.EnsembleRun.__new__(ensemble.EnsembleRun)
    run.st = pkg.SpaceTime("sin", 18, 100, 1)
    run.engine = bare_engine(pkg)
    run.has_schedules = schedules
    run.step_index = step_index
    run.ncol = 3
    return run


def test_ensemble_checks_before_the_device(pkg):
    ramp = pkg.Forcing(0.0, 10.0, -10.0, (1, 1), (1.0, -1.0))
    assert not ramp.constant
    cases = [(_bare_run(pkg, schedules=True), dict(max_years=5), "built with forcings="),
             (_bare_run(pkg), dict(max_years=5, forcing=ramp), "constant forcing"),
             (_bare_run(pkg, step_index=7), dict(max_years=5), "starts a year"),
             (_bare_run(pkg), dict(max_years=5, tol={"Q": 1.0}), "unknown field 'Q'"),
             (_bare_run(pkg), dict(max_years=5, tol={"T": -1.0}), "must be >= 0"),
             (_bare_run(pkg), dict(max_years=0), "max_years")]
    for run, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            run.equilibrate(**kw)
