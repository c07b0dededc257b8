"""CPU tests of the ensemble Kalman update (ebm_update_columns, include/ebm_hip.h): the NumPy restatement against exact
rational sums, the two symbols in the header, the library, the signature table, the Julia shim and INTEGRATION.md, the
NULL-handle refusal through the loaded library, the Gaspari-Cohn taper, the Python argument checks before any device call,
and EnsembleRun.enkf on a stand-in engine for a small linear-Gaussian case, alone and over two ranks."""
import ctypes
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from support import bare_engine, same_bits
from test_host_ensemble_cov import Standin, TwoRanks
from update_columns_ref import clamp, innovations, update_bound, update_exact, update_ref

NAMES = ("ebm_update_columns", "ebm_update_columns_device")


def test_restatement_against_exact_sums():
    rng = np.random.default_rng(1)
    ncol, nlat = 5, 7
    xo = rng.normal(0.0, 3.0, (ncol, nlat))
    xo[1, 2] = np.nan
    y = rng.normal(0.0, 3.0, nlat)
    y[4] = np.nan
    e = rng.normal(0.0, 1.0, (ncol, nlat))
    g = rng.normal(0.0, 1.0, (nlat, nlat)) * 2.0 ** rng.integers(-20, 20, (nlat, nlat))
    g[3, 1] = 0.0
    for scale, pert in ((1.0, None), (0.5, e), (-3.0, e)):
        d = innovations(xo, y, scale, pert)
        assert (d[:, 4] == 0.0).all() and d[1, 2] == 0.0 and not np.signbit(d[1, 2]), "the masks give +0.0"
        c, j = 2, 3                                                    # each operation rounded once, as stated
        t = y[j] + pert[c, j] if pert is not None else y[j]
        assert d[c, j] == t - np.float64(scale) * xo[c, j]
        acc, T, n = update_ref(d, g)
        for c in range(ncol):
            for k in range(nlat):
                exact = sum(Fraction(float(d[c, j])) * Fraction(float(g[k, j])) for j in range(nlat))
                absum = sum(abs(Fraction(float(d[c, j])) * Fraction(float(g[k, j]))) for j in range(nlat))
                assert n[c, k] == sum(1 for j in range(nlat) if d[c, j] != 0.0 and g[k, j] != 0.0)
                hi = float(acc[c, k])                                  # the longdouble as an exact rational: two doubles
                got = Fraction(hi) + Fraction(float(acc[c, k] - np.longdouble(hi)))
                assert abs(got - exact) <= Fraction(2) ** -60 * absum * nlat
                assert abs(float(T[c, k]) - float(absum)) <= 2.0 ** -50 * float(absum)
                assert update_bound(T, n)[c, k] >= 0.0
    # the integer path is exact, and the clamp strict
    xi = rng.integers(-1024, 1025, (ncol, nlat)).astype(np.float64)
    di = rng.integers(-100, 101, (ncol, nlat)).astype(np.float64)
    gi = rng.integers(-8, 9, (nlat, nlat)).astype(np.float64)
    want = np.array([[xi[c, k] + sum(int(di[c, j]) * int(gi[k, j]) for j in range(nlat)) for k in range(nlat)] for c in range(ncol)])
    assert same_bits(update_exact(xi, di, gi), want + 0.0)
    assert same_bits(update_exact(xi, di, gi, -50.0, 60.0), np.clip(want, -50.0, 60.0) + 0.0)
    assert same_bits(clamp(np.array([-0.0, np.nan, 5.0, -5.0]), 0.0, 1.0), np.array([-0.0, np.nan, 1.0, 0.0]))


def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    flat = " ".join(hdr.replace(" * ", " ").split())
    assert "ENSEMBLE KALMAN UPDATE" in hdr and "n_obs 2^-53 sum_j |d g| (1 + 2^-4)" in flat
    assert "ebm_update_columns*, the other writer of prognostic fields" in flat, "the Validity paragraph names the writer"
    assert "-0.0 with acc = +0.0 becomes +0.0" in flat
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
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name
    assert protos[NAMES[0]] == ["ebm_handle_t h", "int nvars", "const int *fields", "int obs_field", "const double *gain",
                                "const double *target", "double scale", "const double *dev_perturb", "const double *lo", "const double *hi"]
    assert protos[NAMES[1]] == protos[NAMES[0]][:4] + ["const double *dev_gain"] + protos[NAMES[0]][5:]
    C = ctypes
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert lib.ebm_update_columns.argtypes == [C.c_void_p, C.c_int, ip, C.c_int, dp, dp, C.c_double, C.c_void_p, dp, dp]
    assert lib.ebm_update_columns_device.argtypes == [C.c_void_p, C.c_int, ip, C.c_int, C.c_void_p, dp, C.c_double, C.c_void_p, dp, dp]
    assert "ebm_update.hip" in open(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "Makefile")).read()


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    g, y = np.zeros(4), np.zeros(2)
    ids = (ctypes.c_int * 1)(0)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.ebm_update_columns(None, 1, ids, 0, g.ctypes.data_as(dp), y.ctypes.data_as(dp), 1.0, None, None, None) == -1
    assert b"ebm_update_columns" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
    assert lib.ebm_update_columns_device(None, 1, ids, 0, ctypes.c_void_p(16), y.ctypes.data_as(dp), 1.0, None, None, None) == -1
    assert b"ebm_update_columns_device" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()


def test_gaspari_cohn(pkg):
    gc = pkg.gaspari_cohn
    r = np.linspace(0.0, 3.0, 3001)
    v = gc(r)
    assert v[0] == 1.0 and (v[r >= 2.0] == 0.0).all() and (v >= 0.0).all() and (v <= 1.0).all()
    assert (np.diff(v) <= 0.0).all() and (np.diff(v[r < 2.0]) < 0.0).all(), "monotone, strictly inside the support"
    assert abs(gc(1.0) - 5.0 / 24.0) < 1e-15 and abs(v[1000] - gc(np.nextafter(1.0, 2.0))) < 1e-14, "continuous at r = 1"
    assert gc(np.array([[-0.5]]))[0, 0] == gc(0.5) and gc(0.5) > 0.68, "even; near exp(-r^2 / (2 * 0.3)) at small r"
    # a Schur product with it keeps a covariance positive semi-definite
    x = np.linspace(0.0, 1.0, 40)
    assert np.linalg.eigvalsh(gc(np.abs(x[:, None] - x[None, :]) / 0.2)).min() > -1e-12


def test_engine_checks_raise_before_any_device_call(pkg):
    eng = bare_engine(pkg, "MIZ", ncol=3)                             # 18 latitudes
    g, y = np.zeros((2, 18, 18)), np.zeros(18)
    ok = eng.check_update_args(("Ei", "h"), "T", g, y, 0.5, None, {"h": (0.0, None)})
    assert ok[1] == [0, 2] and ok[2] == 10 and ok[5] == 0.5 and ok[7].tolist() == [-np.inf, 0.0] and ok[8].tolist() == [np.inf, np.inf]
    assert eng.check_update_args("phi", "phi", np.zeros((18, 18)), y)[3].shape == (1, 18, 18), "one field: [nlat, nlat] is taken"
    bad_g, bad_y = g.copy(), y.copy()
    bad_g[1, 7, 5], bad_y[11] = np.nan, np.inf
    for args, says in (((("Ei", "T"), "T", g, y), "not a prognostic"), ((("Ei", "Ei"), "T", g, y), "twice"),
                       ((("Ei", "h"), "T0", g, y), "T0"), ((("Ei", "h"), "T", g[:1], y), "gain"),
                       ((("Ei", "h"), "T", bad_g, y), "field h, k = 7, j = 5"), ((("Ei", "h"), "T", g, bad_y), "target[11]"),
                       ((("Ei", "h"), "T", g, y, np.nan), "scale"), ((("Ei", "h"), "T", g, y, 1.0, np.zeros((3, 18))), "perturb"),
                       ((("Ei", "h"), "T", g, y, 1.0, None, {"h": (1.0, 0.0)}), "bounds"),
                       ((("Ei", "h"), "T", g, y, 1.0, None, {"D": (0.0, 1.0)}), "bounds"),
                       (((), "T", g, y), "between 1 and 5")):
        with pytest.raises(ValueError) as err:
            eng.update_columns(*args)
        assert says in str(err.value), (says, str(err.value))
    with pytest.raises(ValueError):
        bare_engine(pkg, "Classic").update_columns(("Ei",), "T", np.zeros((18, 18)), y)


# ---- enkf on a stand-in: a small linear-Gaussian case ----------------------------------------------------------------------------

class KalmanStandin(Standin):
    """Standin with the one writer ``KalmanMixin`` needs: update_columns by the restatement on the host fields."""

    def __init__(self, ensemble, fields, x):
        super().__init__(ensemble, fields)
        me = self
        self.updates = []

        class Run(ensemble.KalmanMixin):
            st = type("St", (), {"x": x})()

            def ensemble_sums(s, names, weights=None, center=None):
                return me.sums(names, weights, center)

            def ensemble_covariance(s, a, b=None, weights=None, ca=None, cb=None):
                return me.cov(a, b, weights, ca, cb)

            def update_columns(s, names, obs_name, gain, target, scale=1.0, perturb=None, bounds=None):
                me.updates.append((tuple(names), obs_name, np.array(gain), np.array(target), scale, perturb, dict(bounds or {})))
                d = innovations(me.fields[obs_name], target, scale, perturb)
                new = {n: clamp(me.fields[n] + np.asarray(update_ref(d, gain[v])[0], dtype=np.float64), *(bounds or {}).get(n, (None, None)))
                       for v, n in enumerate(names)}
                me.fields.update(new)

            def obs_noise(s, sd, generator=None):
                return generator.normal(0.0, 1.0, me.fields["T"].shape) * sd
        self.mixin = Run()


def linear_gaussian(ncol, nlat, seed):
    rng = np.random.default_rng(seed)
    L = rng.normal(0.0, 1.0, (2 * nlat, 2 * nlat)) / np.sqrt(nlat)
    z = rng.normal(0.0, 1.0, (ncol, 2 * nlat)) @ L.T + rng.normal(0.0, 2.0, 2 * nlat)
    return {"T": z[:, :nlat].copy(), "Ei": z[:, nlat:].copy()}


def test_denkf_on_a_standin_is_the_textbook_analysis(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    ncol, nlat = 60, 8
    x = np.linspace(0.05, 0.95, nlat)
    f = linear_gaussian(ncol, nlat, 3)
    prior = {k: v.copy() for k, v in f.items()}
    obs = np.random.default_rng(5).normal(1.0, 1.0, nlat)
    obs[[2, 6]] = np.nan
    J = ~np.isnan(obs)
    R = 0.3
    s = KalmanStandin(ensemble, f, x)
    out = s.mixin.enkf(("T", "Ei"), "T", obs, R)
    assert out["gain_shape"] == (2, nlat, nlat) and out["observed"] == 6 and out["members"] == ncol
    names, obs_name, G, target, scale, perturb, bounds = s.updates[0]
    assert len(s.updates) == 1 and perturb is None and scale == 0.5 and bounds == {}
    assert (G[:, :, ~J] == 0.0).all() and np.abs(G[:, :, J]).min() > 0.0, "unobserved cells: zero gain columns"
    # the textbook: z = (T, Ei), H picks the observed cells of T, P the unbiased ensemble covariance
    Z = np.concatenate([prior["T"], prior["Ei"]], axis=1)
    P = np.cov(Z.T, ddof=1)
    H = np.zeros((int(J.sum()), 2 * nlat))
    H[np.arange(J.sum()), np.flatnonzero(J)] = 1.0
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T + R * np.eye(J.sum()))
    assert np.allclose(np.concatenate([G[0][:, J], G[1][:, J]]), K, rtol=1e-9, atol=1e-12)
    Za = np.concatenate([f["T"], f["Ei"]], axis=1)
    mean_a = Z.mean(axis=0) + K @ (obs[J] - H @ Z.mean(axis=0))
    assert np.allclose(Za.mean(axis=0), mean_a, rtol=1e-10, atol=1e-12), "the mean moves by the full gain"
    Pa = (np.eye(2 * nlat) - K @ H) @ P + 0.25 * K @ H @ P @ H.T @ K.T
    assert np.allclose(np.cov(Za.T, ddof=1), Pa, rtol=1e-9, atol=1e-11), "(I - KH) P + 1/4 K HPH' K'"
    assert out["posterior"]["rmse"] < out["prior"]["rmse"] and out["posterior"]["spread"] < out["prior"]["spread"]
    # localisation and inflation enter the gain as stated
    s2 = KalmanStandin(ensemble, {k: v.copy() for k, v in prior.items()}, x)
    k2 = s2.mixin.kalman_gains(("Ei",), "T", obs, R, localize=0.2, inflation=1.1)
    rho = pkg.gaspari_cohn(np.abs(x[:, None] - x[None, :]) / 0.2)
    P_oo, P_fo = P[:nlat, :nlat], P[nlat:, :nlat]
    S = 1.1 * (rho * P_oo)[np.ix_(J, J)] + R * np.eye(J.sum())
    assert np.allclose(k2["gain"][0][:, J], 1.1 * (rho * P_fo)[:, J] @ np.linalg.inv(S), rtol=1e-9, atol=1e-12)
    assert (k2["gain"][0][:, ~J] == 0.0).all()
    # the perturbed-observation filter: target = obs, scale 1, noise of the stated size on the observed cells only
    s3 = KalmanStandin(ensemble, {k: v.copy() for k, v in prior.items()}, x)
    s3.mixin.enkf(("T", "Ei"), "T", obs, R, method="perturbed", generator=np.random.default_rng(1))
    _, _, G3, target3, scale3, e3, _ = s3.updates[0]
    assert scale3 == 1.0 and same_bits(target3, obs) and same_bits(G3, G) and (e3[:, ~J] == 0.0).all()
    assert abs(e3[:, J].std() - np.sqrt(R)) < 0.1
    assert np.allclose(np.concatenate([s3.fields["T"], s3.fields["Ei"]], axis=1).mean(axis=0), mean_a + K @ e3[:, J].mean(axis=0), rtol=1e-9)
    for bad in (dict(method="etkf"), dict(inflation=0.0), dict(localize=-1.0)):
        with pytest.raises(ValueError):
            s.mixin.enkf(("T",), "T", obs, R, **bad)
    with pytest.raises(ValueError, match="obs_var"):
        s.mixin.enkf(("T",), "T", obs, 0.0)
    doc = " ".join(ensemble.KalmanMixin.enkf.__doc__.split())
    assert "src/miz.jl:109-117, 74-80" in doc and "0 <= D <= Dmax" in doc and "Sakov and Oke" in doc


def test_two_shards_apply_the_same_gain(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    ncol, nlat = 41, 6
    x = np.linspace(0.1, 0.9, nlat)
    f = linear_gaussian(ncol, nlat, 7)
    obs = np.random.default_rng(2).normal(0.0, 1.0, nlat)
    obs[3] = np.nan
    shards = [pkg.shard_columns(ncol, 2, r) for r in (0, 1)]
    group = TwoRanks()
    stand = [KalmanStandin(ensemble, {k: v[sl].copy() for k, v in f.items()}, x) for sl in shards]
    group.run(lambda r: stand[r].mixin.enkf(("T", "Ei"), "T", obs, 0.5, localize=0.5, dist=group))
    assert same_bits(stand[0].updates[0][2], stand[1].updates[0][2]) and same_bits(stand[0].updates[0][3], stand[1].updates[0][3])
    alone = KalmanStandin(ensemble, {k: v.copy() for k, v in f.items()}, x)
    alone.mixin.enkf(("T", "Ei"), "T", obs, 0.5, localize=0.5)
    assert np.allclose(stand[0].updates[0][2], alone.updates[0][2], rtol=1e-9, atol=1e-13), "the gain of the whole ensemble"
    for n in ("T", "Ei"):
        assert np.allclose(np.concatenate([stand[0].fields[n], stand[1].fields[n]]), alone.fields[n], rtol=1e-9, atol=1e-12)
