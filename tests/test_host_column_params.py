"""CPU tests of per-column parameter sets (ebm_set_column_params): the symbol in the header, the library and the
bindings; its null-handle refusal without a GPU; the host helpers that build the [ncol, 25] rows
(engine.param_matrix) and check an ensemble's member counts before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_symbol_is_declared_exported_and_bound(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebm_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ebm_set_column_params\s*\(\s*ebm_handle_t\s+h\s*,\s*const\s+double\s*\*\s*params\s*\)\s*;", hdr)
    assert "ebm_set_column_params" in pkg.EXPORTS
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "ebm_set_column_params")
    assert re.search(r"\bebm_set_column_params\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_null_handle_is_refused_without_a_gpu(pkg):
    import sys
    _lib = sys.modules[pkg.__name__ + "._lib"]
    lib = _lib.load()
    row = np.zeros((1, 25))
    assert lib.ebm_set_column_params(None, _lib.dptr(row)) == -1
    assert b"null handle" in lib.ebm_last_error()
    assert lib.ebm_set_column_params(None, None) == -1


def test_param_matrix_order_defaults_and_overrides(pkg):
    from importlib import import_module
    engine = import_module(pkg.__name__ + ".engine")
    order = engine.PARAM_ORDER
    assert len(order) == 25 and order[0] == "D" and order[16] == "Tm" and order[24] == "kappa"
    par = pkg.default_parameters("MIZ")                 # no F, cg, tau: those come from the defaults
    par["A"] = 190.0
    rows = [{"D": 0.5}, pkg.Collection(kappa=1e5, alpha=0.7), {}, None, {"F": 3.0, "D": 0.6}]
    m = engine.param_matrix(rows, par, pkg.default_parval)
    assert m.shape == (5, 25) and m.dtype == np.float64
    base = engine.param_vector(par, pkg.default_parval)
    assert base[order.index("A")] == 190.0 and base[order.index("cg")] == pkg.default_parval["cg"]
    want = np.tile(base, (5, 1))
    want[0, order.index("D")] = 0.5
    want[1, order.index("kappa")] = 1e5
    want[1, order.index("alpha")] = 0.7
    want[4, order.index("F")] = 3.0
    want[4, order.index("D")] = 0.6
    assert np.array_equal(m, want)
    assert engine.param_matrix([], par, pkg.default_parval).shape == (0, 25)


def test_param_matrix_refuses_unknown_names(pkg):
    from importlib import import_module
    engine = import_module(pkg.__name__ + ".engine")
    par = pkg.default_parameters("MIZ")
    with pytest.raises(ValueError, match="member 1: unknown parameter 'd'"):
        engine.param_matrix([{"D": 0.5}, {"d": 0.5}], par, pkg.default_parval)
    with pytest.raises(TypeError, match="member 0"):
        engine.param_matrix([0.5], par, pkg.default_parval)


def test_member_params_counts_are_checked_before_the_device(pkg):
    """EnsembleRun(member_params=...) refuses member counts that disagree with init, fcol or forcings — before it creates
    a handle (there is no GPU here: reaching ebm_create would raise EBMError instead)."""
    from importlib import import_module
    ensemble = import_module(pkg.__name__ + ".ensemble")
    st = pkg.SpaceTime("sin", 18, 100, 1)
    par = pkg.default_parameters("MIZ")
    flat = {k: np.zeros(st.nx) for k in ("Ei", "Ew", "h", "D", "phi")}
    per = {k: np.zeros((3, st.nx)) for k in ("Ei", "Ew", "h", "D", "phi")}
    mp = [{"D": d} for d in (0.5, 0.6, 0.7)]
    f = pkg.Forcing(0.0)
    cases = [(dict(init=per, member_params=mp[:2]), r"init\['Ei'\] has 3 columns"),
             (dict(init=flat, member_params=mp, fcol=np.zeros(2)), "fcol has 2"),
             (dict(init=flat, member_params=mp, forcings=[f, f]), "forcings has 2"),
             (dict(init=flat, member_params=[]), "at least one member"),
             (dict(init=flat, member_params=[{"Dee": 1.0}] * 3), "unknown parameter")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            pkg.EnsembleRun("MIZ", st, par, **kw)
    rows = ensemble.member_param_rows(mp, par, per, np.zeros(3), [f, f, f])
    assert rows.shape == (3, 25) and list(rows[:, 0]) == [0.5, 0.6, 0.7]
