"""Host-side tests of ebm_spd_solve_device / ebm_kalman_gain_device (no GPU): the ABI rows and symbols, the NULL-handle refusal,
the NumPy restatements (tests/kalman_gain_ref.py) against numpy.linalg.solve and against the system ``kalman_gains`` builds
today, and that the exact cases of tests/test_gpu_kalman_gain.py really are free of rounding in the blocked algorithm."""
import ctypes
import sys

import numpy as np
import pytest

from kalman_gain_ref import (assemble_ref, backward_errors, bidiagonal_case, blocked_solve_ref, diagonal_case, pad_system, random_spd,
                             round_up, scatter_ref)
from support import same_bits
from test_host_ensemble_cov import TwoRanks
from test_host_update_columns import KalmanStandin, linear_gaussian

NAMES = ("ebm_spd_solve_device", "ebm_kalman_gain_device", "ebm_kalman_gain_phases")
SIZES = (1, 2, 63, 64, 65, 128, 130, 200)


def test_symbols_are_bound_and_exported(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"]
    P, v, i, ll, d = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    assert lib.SIGNATURES[NAMES[0]] == [v, i, ll, v, ll, v, ll, P(i)]
    assert lib.SIGNATURES[NAMES[1]] == [v, i, P(d), P(d), d, d, v, P(v), v, P(i)]
    assert lib.SIGNATURES[NAMES[2]] == [v, P(ctypes.c_float)]
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    for n in NAMES:
        assert n in pkg.EXPORTS and hasattr(cdll, n)


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    info = ctypes.c_int(7)
    y = np.zeros(4)
    dp = y.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    addr = (ctypes.c_void_p * 1)(16)
    assert lib.ebm_spd_solve_device(None, 64, 1, ctypes.c_void_p(16), 64, ctypes.c_void_p(16), 64, ctypes.byref(info)) == -1
    assert b"ebm_spd_solve_device" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
    assert lib.ebm_kalman_gain_device(None, 1, dp, dp, 0.0, 1.0, ctypes.c_void_p(16), addr, ctypes.c_void_p(16), ctypes.byref(info)) == -1
    assert b"ebm_kalman_gain_device" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
    assert info.value == 7, "a refusal writes nothing"
    assert lib.ebm_kalman_gain_phases(None, (ctypes.c_float * 4)()) == -1 and b"ebm_kalman_gain_phases" in lib.ebm_last_error()


@pytest.mark.parametrize("m", (1, 63, 65, 130))
def test_restatement_against_numpy(m):
    """The blocked algorithm in np.longdouble solves what numpy.linalg.solve solves, with a backward error no larger."""
    S = random_spd(m, 6.0, m)
    B = np.random.default_rng(m + 1).normal(size=(7, m))
    Sp, Bp = pad_system(S, B)
    L, X, info = blocked_solve_ref(Sp, Bp)
    assert info == 0 and np.array_equal(L, np.tril(L)) and np.array_equal(X[:, m:], np.zeros((7, round_up(m) - m)))
    assert np.allclose(np.asarray(L @ L.T, dtype=np.float64), Sp, rtol=1e-13, atol=1e-16)
    want = np.linalg.solve(S, B.T).T
    eta, eta_np = backward_errors(S, X[:, :m], B), backward_errors(S, want, B)
    assert eta.max() <= max(eta_np.max(), 2.0 ** -53), (eta.max(), eta_np.max())
    # forward, normwise: cond_2 = 1e6 (cond_inf within a factor m of it) times the two backward errors, doubled (eta's denominator)
    diff = np.max(np.abs(np.asarray(X[:, :m], dtype=np.float64) - want), axis=1)
    assert (diff <= 4.0 * m * 1e6 * (eta + eta_np + 2.0 ** -53) * np.max(np.abs(want), axis=1)).all()


def test_restatement_reports_the_first_bad_pivot():
    Sp, Bp = pad_system(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones((1, 2)))
    assert blocked_solve_ref(Sp, Bp)[2] == 2
    S = random_spd(70, 2.0, 3)
    S[66, 66] = np.nan
    assert blocked_solve_ref(*pad_system(S, np.ones((1, 70))))[2] == 67


def test_assembly_restatement_is_the_system_kalman_gains_builds(pkg, monkeypatch):
    """S and B as ``kalman_gains`` hands them to numpy.linalg.solve today, bit for bit: P scaled to the unbiased estimate
    first and factor = inflation, which is the host's operation order."""
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    ncol, nlat = 40, 9
    x = np.linspace(0.05, 0.95, nlat)
    obs = np.random.default_rng(5).normal(1.0, 1.0, nlat)
    obs[[1, 4]] = np.nan
    R = np.linspace(0.2, 0.5, nlat)
    seen = []
    solve = np.linalg.solve
    monkeypatch.setattr(np.linalg, "solve", lambda a, b: (seen.append((a.copy(), b.copy())), solve(a, b))[1])
    for localize, inflation in ((None, 1.0), (0.3, 1.25)):
        del seen[:]
        s = KalmanStandin(ensemble, linear_gaussian(ncol, nlat, 3), x)
        k = s.mixin.kalman_gains(("Ei", "T"), "T", obs, R, localize, inflation)
        unbias = ncol / (ncol - 1.0)
        P_oo = s.mixin.covariance("T")["cov"] * unbias
        P_fo = [s.mixin.covariance("Ei", "T")["cov"] * unbias, P_oo]
        J, S, B = assemble_ref(x, obs, R, localize, inflation, P_oo, P_fo, pkg.gaspari_cohn)
        m = J.size
        assert m == 7 and len(seen) == 2 and np.array_equal(J, np.flatnonzero(k["observed"]))
        assert same_bits(S[:m, :m], seen[0][0]) and same_bits(S[:m, :m], seen[1][0])
        for v in range(2):
            assert same_bits(B[v * nlat:(v + 1) * nlat, :m], seen[v][1].T), (localize, v)
        assert np.array_equal(S[m:, m:], np.eye(round_up(m) - m)) and not S[:m, m:].any() and not S[m:, :m].any() and not B[:, m:].any()
        # ... and solved by the blocked restatement and scattered, it is the gain of today
        X = blocked_solve_ref(S, B)[1]
        assert np.allclose(scatter_ref(X, J, 2, nlat), k["gain"], rtol=1e-9, atol=1e-13)
        assert not scatter_ref(X, J, 2, nlat)[:, :, [1, 4]].any()


@pytest.mark.parametrize("m", SIZES)
def test_the_bidiagonal_factor_is_exact_in_double(m):
    """S = L L^T with L bidiagonal (2, 1): the blocked algorithm in float64 leaves exactly L — and in longdouble the same
    numbers, so nothing was rounded on the way."""
    S, L = bidiagonal_case(m)
    Sp, Bp = pad_system(S, np.zeros((1, m)))
    for dtype in (np.float64, np.longdouble):
        got, _, info = blocked_solve_ref(Sp, Bp, dtype)
        assert info == 0 and np.array_equal(got[:m, :m], L), (m, dtype)
        assert np.array_equal(got[m:, m:], np.eye(round_up(m) - m)) and not got[m:, :m].any()


@pytest.mark.parametrize("m", SIZES)
def test_the_diagonal_solve_is_exact_in_double(m):
    S, B, X = diagonal_case(m, 5, m)
    Sp, Bp = pad_system(S, B)
    for dtype in (np.float64, np.longdouble):
        got = blocked_solve_ref(Sp, Bp, dtype)[1]
        assert np.array_equal(got[:, :m], X) and not got[:, m:].any(), (m, dtype)
    assert same_bits(np.asarray(blocked_solve_ref(Sp, Bp, np.float64)[1][:, :m]), X)


def test_solver_argument_is_checked_and_defaults_to_host(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    nlat = 6
    s = KalmanStandin(ensemble, linear_gaussian(20, nlat, 1), np.linspace(0.1, 0.9, nlat))
    with pytest.raises(ValueError, match="solver"):
        s.mixin.kalman_gains(("T",), "T", np.zeros(nlat), 1.0, solver="gpu")
    assert isinstance(s.mixin.kalman_gains(("T",), "T", np.zeros(nlat), 1.0)["gain"], np.ndarray)
    with pytest.raises(ValueError, match="one shard"):
        s.mixin.kalman_gains(("T",), "T", np.zeros(nlat), 1.0, dist=TwoRanks(), solver="device")
    import inspect
    assert inspect.signature(ensemble.KalmanMixin.enkf).parameters["solver"].default == "host"
