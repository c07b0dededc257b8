"""CPU tests of the column scalars (ebm_column_scalars, ebm_run_series_scalars, ebm_run_until_scalar): the NumPy restatement
tests/column_scalars_ref.py against ensemble.hemispheric_mean and hand-made rows (every corner of the edge rule), the
band -> cell mapping of ensemble.scalar_spec, every refusal of Engine.check_scalar_args — which run before any device call —
and the four symbols in the header, the library, the signature table, the Julia shim and INTEGRATION.md."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import column_scalars_ref as ref
from conftest import ROOT
from support import bare_engine, same_bits

SYMBOLS = {
    "ebm_column_scalars": ["ebm_handle_t h", "int nscal", "const int *spec", "const double *level", "double *out"],
    "ebm_column_scalars_device": ["ebm_handle_t h", "int nscal", "const int *spec", "const double *level", "double *dev_out"],
    "ebm_run_series_scalars": ["ebm_handle_t h", "long long first_step", "int nsteps", "const double *f_steps", "int every",
                               "int steps_per_launch", "int nscal", "const int *spec", "const double *level", "double *series"],
    "ebm_run_until_scalar": ["ebm_handle_t h", "long long first_step", "int max_samples", "int every", "const double *f_steps",
                             "int steps_per_launch", "const int *spec", "double scalar_level", "const double *level",
                             "const int *direction", "int *samples", "int *crossed", "double *value"],
}


# ---- the restatement -----------------------------------------------------------------------------------------------------

def test_full_range_integral_is_the_hemispheric_mean(pkg):
    rng = np.random.default_rng(5)
    for nlat in (2, 3, 65, 514):
        x = np.sort(rng.uniform(0.0, 1.0, nlat))
        f = rng.normal(size=(4, nlat)) * 10.0 ** rng.integers(-3, 4, size=(4, 1))
        f[3, nlat // 2] = np.nan                              # a NaN in the band gives NaN
        want = pkg.hemispheric_mean(f, x)
        got = ref.column_scalars({"T": f}, x, [("integral", "T", 0, nlat - 1)])[0]
        assert same_bits(got, want) and np.isnan(got[3]) and np.isfinite(got[:3]).all()


def test_band_integral_and_mean_by_hand():
    x = np.array([0.0, 0.25, 0.5, 1.0])
    f = np.array([1.0, 3.0, 5.0, 9.0])
    assert ref.scalar(f, x, "integral", 1, 3) == (3.0 + 5.0) * 0.25 / 2.0 + (5.0 + 9.0) * 0.5 / 2.0
    assert ref.scalar(f, x, "mean", 1, 3) == ((3.0 + 5.0) * 0.25 / 2.0 + (5.0 + 9.0) * 0.5 / 2.0) / 0.75
    assert ref.scalar(f, x, "integral", 0, 1) == 0.5 and ref.scalar(f, x, "mean", 0, 1) == 2.0
    # sequential, left to right: the sum of three terms is ((t0 + t1) + t2)
    g = np.array([1e16, 1.0, -1e16, 3.0])
    u = np.array([0.0, 2.0, 4.0, 6.0])
    t = [(g[i] + g[i + 1]) * 2.0 / 2.0 for i in range(3)]
    assert ref.scalar(g, u, "integral", 0, 3) == (0.0 + t[0] + t[1]) + t[2]


def test_edge_corner_cases():
    inf, nan = np.inf, np.nan
    x = np.array([0.1, 0.2, 0.4, 0.8, 0.9])
    f = np.array([0.0, 0.1, 0.3, 0.7, 1.0])
    assert ref.scalar(f, x, "edge_ge", 0, 4, 2.0) == inf                       # no hit: no edge in the band
    assert ref.scalar(f, x, "edge_ge", 0, 2, 0.5) == inf                       # ... the band ends before the hit
    assert ref.scalar(f, x, "edge_le", 1, 4, 0.05) == inf
    assert ref.scalar(f, x, "edge_ge", 0, 4, 0.0) == 0.1                       # a hit at k0: x[k0], no interpolation
    assert ref.scalar(f, x, "edge_ge", 2, 4, 0.2) == 0.4                       # ... at an interior k0, whatever f[k0-1] is
    assert ref.scalar(f, x, "edge_ge", 0, 4, 0.5) == 0.4 + ((0.5 - 0.3) / (0.7 - 0.3)) * (0.8 - 0.4)
    assert ref.scalar(f, x, "edge_ge", 0, 4, 0.3) == 0.2 + ((0.3 - 0.1) / (0.3 - 0.1)) * (0.4 - 0.2)      # level == a cell: t = 1
    assert ref.scalar(f, x, "edge_ge", 0, 4, 0.3) == 0.4
    assert ref.scalar(f[::-1].copy(), x, "edge_le", 0, 4, 0.3) == 0.2 + ((0.3 - 0.7) / (0.3 - 0.7)) * (0.4 - 0.2)
    assert ref.scalar(f, x, "edge_ge", 3, 3, 0.7) == 0.8 and ref.scalar(f, x, "edge_ge", 3, 3, 0.71) == inf    # one cell
    assert ref.scalar(f, x, "edge_le", 0, 0, 0.0) == 0.1
    for bad in (nan, inf, -inf):                                              # a neighbour that is not finite: x[K]
        g = f.copy()
        g[2] = bad
        want = 0.4 if bad == inf else 0.8                                      # +Inf is itself the first hit, at k = 2
        assert ref.scalar(g, x, "edge_ge", 0, 4, 0.5) == want, bad
    g = f.copy()
    g[3] = inf                                                                # K's own value is not finite: x[K]
    assert ref.scalar(g, x, "edge_ge", 0, 4, 0.5) == 0.8
    g = np.array([nan, nan, 0.3, nan, 1.0])                                   # NaN never hits, in either direction
    assert ref.scalar(g, x, "edge_ge", 0, 4, 0.2) == 0.4 and ref.scalar(g, x, "edge_le", 0, 4, 0.2) == inf
    assert ref.scalar(np.full(5, nan), x, "edge_le", 0, 4, 0.0) == inf
    # the first hit, not the last and not the nearest: f rises, falls, rises
    g = np.array([0.0, 0.6, 0.1, 0.9, 1.0])
    assert ref.scalar(g, x, "edge_ge", 0, 4, 0.5) == 0.1 + ((0.5 - 0.0) / (0.6 - 0.0)) * (0.2 - 0.1)


# ---- scalar_spec ---------------------------------------------------------------------------------------------------------

def test_scalar_spec_maps_a_band_to_the_cells_inside(pkg):
    st = pkg.SpaceTime("identity", 10, 2000, 1)              # x = 0.05, 0.15, ..., 0.95
    x = st.x
    assert pkg.scalar_spec(st, "integral", "T") == ("integral", "T", 0, 9)
    assert pkg.scalar_spec(st, "edge_ge", "phi", None, 0.15) == ("edge_ge", "phi", 0, 9, 0.15)
    assert pkg.scalar_spec(st, "mean", "h", (0.5, 1.0)) == ("mean", "h", 5, 9)
    assert pkg.scalar_spec(st, "mean", "h", (float(x[2]), float(x[4]))) == ("mean", "h", 2, 4)      # both ends inclusive
    assert pkg.scalar_spec(st, "edge_ge", "h", (np.nextafter(x[2], 1.0), np.nextafter(x[4], 0.0)), 1.0) == ("edge_ge", "h", 3, 3, 1.0)
    assert pkg.scalar_spec(st, "edge_le", "T", (0.3, 0.32 + 0.1), -2.0) == ("edge_le", "T", 3, 3, -2.0)   # one cell: an edge may
    for band, msg in (((0.96, 1.0), "no cell"), ((0.16, 0.24), "no cell"), ((0.5, 0.4), "x_lo <= x_hi")):
        with pytest.raises(ValueError, match=msg):
            pkg.scalar_spec(st, "mean", "T", band)
    with pytest.raises(ValueError, match="one cell"):
        pkg.scalar_spec(st, "mean", "T", (0.3, 0.4))
    for level in (None, np.nan):
        with pytest.raises(ValueError, match="level"):
            pkg.scalar_spec(st, "edge_ge", "phi", None, level)


# ---- the argument checks ---------------------------------------------------------------------------------------------------

def test_check_scalar_args_accepts_and_packs(pkg):
    eng = bare_engine(pkg)                                   # MIZ, 18 latitudes
    spec, level = eng.check_scalar_args([("integral", "T", 0, 17), ("mean", "phi", 3, 4, None), ("edge_ge", "phi", 0, 17, 0.15),
                                         ("edge_le", "T", 5, 5, -np.inf), ("edge_ge", "phi", 2, 9, 0.5)])
    F = sys.modules[pkg.__name__ + "._lib"].FIELD
    assert spec.dtype == np.int32 and spec.flags.c_contiguous and level.dtype == np.float64
    assert spec.tolist() == [[0, F["T"], 0, 17], [1, F["phi"], 3, 4], [2, F["phi"], 0, 17], [3, F["T"], 5, 5], [2, F["phi"], 2, 9]]
    assert level.tolist() == [0.0, 0.0, 0.15, -np.inf, 0.5]
    spec, _ = bare_engine(pkg, "Classic").check_scalar_args([("integral", "Tg", 0, 1)] * 12)      # twelve, one field repeated
    assert spec.shape == (12, 4)


@pytest.mark.parametrize("specs,msg", [
    ([], "between 1 and 12"),
    ([("integral", "T", 0, 1)] * 13, "between 1 and 12"),
    (None, "between 1 and 12"),
    (("integral", "T", 0, 17), "wrap it in a list"),
    ([("integral", "T", 0)], r"scalar 0: expected \(kind"),
    ([("integral", "T", 0, 17), ("median", "T", 0, 17)], "scalar 1: unknown kind 'median'"),
    ([(0, "T", 0, 17)], "scalar 0: unknown kind"),
    ([("integral", "T0", 0, 17)], "scalar 0: unknown field 'T0'"),
    ([("integral", "Tg", 0, 17)], "scalar 0: unknown field 'Tg'"),
    ([("mean", "T", 0, 17), ("mean", "T", -1, 17)], "scalar 1: the band k0 = -1, k1 = 17"),
    ([("mean", "T", 0, 18)], "scalar 0: the band k0 = 0, k1 = 18"),
    ([("mean", "T", 9, 8)], "scalar 0: the band k0 = 9, k1 = 8"),
    ([("mean", "T", 0.0, 8)], "scalar 0: the band .* cell indices"),
    ([("mean", "T", True, 8)], "scalar 0: the band .* cell indices"),
    ([("integral", "T", 4, 4)], "scalar 0: an integral over one cell"),
    ([("edge_ge", "phi", 0, 17), ("mean", "T", 4, 4)], "scalar 0: an edge needs a level"),
    ([("edge_ge", "phi", 0, 17, 0.1), ("mean", "T", 4, 4)], "scalar 1: an integral over one cell"),
    ([("edge_le", "phi", 0, 17, np.nan)], "scalar 0: an edge needs a level"),
    ([("edge_le", "phi", 0, 17, None)], "scalar 0: an edge needs a level"),
])
def test_check_scalar_args_refuses(pkg, specs, msg):
    eng = bare_engine(pkg)
    with pytest.raises(ValueError, match=msg):
        eng.check_scalar_args(specs)
    for call in (lambda: eng.column_scalars(specs), lambda: eng.column_scalars_device(specs, 4096),
                 lambda: eng.run_series_scalars(0, 10, 5, specs)):
        with pytest.raises(ValueError, match=msg):          # ... before the library is reached (NoDevice)
            call()


def test_series_and_until_checks_run_before_any_device_call(pkg):
    eng = bare_engine(pkg)
    ok = [("edge_ge", "phi", 0, 17, 0.15)]
    for kw, msg in ((dict(every=0), "every = 0"), (dict(nsteps=7), "not a multiple"), (dict(first_step=-1), "must be >= 0"),
                    (dict(steps_per_launch=0), "steps_per_launch = 0")):
        args = dict(first_step=0, nsteps=10, every=5, specs=ok, steps_per_launch=4)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            eng.run_series_scalars(**args)
    lev, d = np.zeros(3), np.ones(3, dtype=np.int64)
    sp, sl, lev2, d2, f = eng.check_until_scalar_args(0, 4, 5, ok[0], lev, -2 * d)
    assert sp.tolist() == [2, 4, 0, 17] and sl == 0.15 and d2.tolist() == [-1, -1, -1] and f is None
    for a, msg in (((0, 0, 5, ok[0], lev, d), "max_samples = 0"), ((0, 4, 0, ok[0], lev, d), "every = 0"),
                   ((0, 4, 5, ("edge_ge", "phi", 0, 18, 0.1), lev, d), "scalar 0: the band"),
                   ((0, 4, 5, ok[0], np.array([0.0, np.nan, 0.0]), d), "level: NaN"), ((0, 4, 5, ok[0], lev, 0 * d), "direction: 0"),
                   ((0, 4, 5, ok[0], lev[:2], d), "shape")):
        with pytest.raises(ValueError, match=msg):
            eng.run_until_scalar(*a)


def test_null_refusals_without_a_gpu(pkg):
    """The C entry points refuse a null handle before they touch a device."""
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    spec, level, out = (ctypes.c_int * 4)(0, 10, 0, 1), (ctypes.c_double * 1)(0.0), (ctypes.c_double * 4)()
    ints = (ctypes.c_int * 4)()
    assert lib.ebm_column_scalars(None, 1, spec, level, out) == -1 and b"ebm_column_scalars: null argument" in lib.ebm_last_error()
    assert lib.ebm_column_scalars_device(None, 1, spec, level, None) == -1
    assert lib.ebm_run_series_scalars(None, 0, 4, None, 2, 1, 1, spec, level, out) == -1
    assert b"ebm_run_series_scalars: null argument" in lib.ebm_last_error()
    assert lib.ebm_run_until_scalar(None, 0, 4, 2, None, 1, spec, 0.0, level, ints, ints, ints, out) == -1
    assert b"ebm_run_until_scalar: null argument" in lib.ebm_last_error()


# ---- the symbols -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_declared_exported_bound_and_documented(pkg, name):
    hdr_text = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"include/ebm_hip.h does not declare {name}"
    assert [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")] == SYMBOLS[name]
    assert name in pkg.EXPORTS and hasattr(ctypes.CDLL(pkg.LIB_PATH), name)
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(_lib.SIGNATURES[name]) == len(SYMBOLS[name])
    assert re.search(r"ccall\(\(:" + name + r", libebm\)", open(os.path.join(ROOT, "julia", "EBMHip.jl")).read())
    assert re.search(r"\b" + name + r"\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    for doc in ("README.md", "DESIGN.md"):
        assert re.search(r"\b" + name + r"\b", open(os.path.join(ROOT, doc)).read()), doc


def test_header_states_the_definition_and_the_kinds(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    text = hdr[hdr.index("COLUMN SCALARS"):hdr.index("int ebm_column_scalars(")]
    assert "THIS TEXT IS THE DEFINITION" in text
    assert re.search(r"enum ebm_scalar_kind \{ EBM_S_INTEGRAL = 0, EBM_S_MEAN = 1, EBM_S_EDGE_GE = 2, EBM_S_EDGE_LE = 3, EBM_S_COUNT \}", text)
    kinds = sys.modules[pkg.__name__ + "._lib"].SCALAR_KIND
    assert kinds == {"integral": 0, "mean": 1, "edge_ge": 2, "edge_le": 3} and tuple(kinds) == ref.KINDS
