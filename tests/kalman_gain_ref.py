"""NumPy restatements of ebm_kalman_gain_device and ebm_spd_solve_device (include/ebm_hip.h): the assembly of the compacted,
padded system in float64 with the header's operation order, and the same blocked algorithm (nb = 64, right-looking, explicit
inverses of the diagonal blocks) in any dtype — np.longdouble for a reference, np.float64 to show that the exact cases are
exact.  Shared by tests/test_host_kalman_gain.py and tests/test_gpu_kalman_gain.py."""
import numpy as np

NB = 64


def round_up(m):
    return (m + NB - 1) // NB * NB


def assemble_ref(x, obs, obs_var, localize, factor, P_oo, P_fo, taper):
    """(J, S [mp, mp], B [nvars * nlat, mp]): S = (rho * P_oo[J, J]) * factor + diag(R[J]) with the identity in the padding,
    B_v = (factor * rho[:, J]) * P_fo_v[:, J] (a non-finite entry as +0.0) with +0.0 in the padding columns.  `taper`: the
    package's gaspari_cohn."""
    x = np.asarray(x, dtype=np.float64)
    nlat = x.shape[0]
    J = np.flatnonzero(~np.isnan(np.asarray(obs, dtype=np.float64)))
    R = np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (nlat,))
    m, mp = J.size, round_up(J.size)
    rho = np.ones((nlat, nlat)) if localize is None or not localize > 0.0 else taper(np.abs(x[:, None] - x[None, :]) / float(localize))
    S = np.eye(mp)
    S[:m, :m] = (rho[np.ix_(J, J)] * np.asarray(P_oo)[np.ix_(J, J)]) * float(factor) + np.diag(R[J])
    B = np.zeros((len(P_fo) * nlat, mp))
    for v, P in enumerate(P_fo):
        P = np.asarray(P)[:, J]
        B[v * nlat:(v + 1) * nlat, :m] = (float(factor) * rho[:, J]) * np.where(np.isfinite(P), P, 0.0)
    return J, S, B


def scatter_ref(X, J, nvars, nlat):
    gain = np.zeros((nvars, nlat, nlat))
    gain[:, :, J] = np.asarray(X, dtype=np.float64).reshape(nvars, nlat, -1)[:, :, :J.size]
    return gain


def pad_system(S, B):
    """The caller's duty for ebm_spd_solve_device: S with the identity, B with zeros, up to a multiple of 64."""
    m, mp = S.shape[0], round_up(S.shape[0])
    Sp = np.eye(mp)
    Sp[:m, :m] = S
    Bp = np.zeros((B.shape[0], mp))
    Bp[:, :m] = B
    return Sp, Bp


def blocked_solve_ref(S, B, dtype=np.longdouble):
    """(L, X, info) of X . S = B by the algorithm of the header on padded inputs (pad_system): L lower triangular (zeros
    above), info the 1-based index of the first pivot that is not > 0 (then L and X are unspecified)."""
    A = np.array(S, dtype=dtype)
    X = np.array(B, dtype=dtype)
    mp = A.shape[0]
    assert mp % NB == 0 and A.shape == (mp, mp) and X.shape[1] == mp
    T = mp // NB
    inv = []
    info = 0
    for k in range(T):
        d = slice(k * NB, (k + 1) * NB)
        a = A[d, d].copy()
        for j in range(NB):
            if not a[j, j] > 0 and not info:
                info = k * NB + j + 1
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.sqrt(a[j, j])
                a[j + 1:, j] = a[j + 1:, j] / s
            for c in range(j + 1, NB):
                a[c:, c] = a[c:, c] - a[c:, j] * a[c, j]
            a[j, j] = s
        if info:
            return np.tril(A), X, info
        L = np.tril(a)
        A[d, d] = L
        W = np.zeros((NB, NB), dtype=dtype)
        for i in range(NB):
            acc = np.zeros(NB, dtype=dtype)
            acc[i] = 1
            for j in range(i):
                acc = acc - L[i, j] * W[j]            # column c of W: zero terms for j < c
            W[i] = acc / L[i, i]
        inv.append(W)
        below = slice((k + 1) * NB, mp)
        A[below, d] = A[below, d] @ W.T
        for i in range(k + 1, T):
            for j in range(k + 1, i + 1):
                ti, tj = slice(i * NB, (i + 1) * NB), slice(j * NB, (j + 1) * NB)
                A[ti, tj] = A[ti, tj] - A[ti, d] @ A[tj, d].T
    L = np.tril(A)
    for k in range(T):
        d = slice(k * NB, (k + 1) * NB)
        X[:, d] = (X[:, d] - X[:, :k * NB] @ L[d, :k * NB].T) @ inv[k].T
    for k in range(T - 1, -1, -1):
        d = slice(k * NB, (k + 1) * NB)
        X[:, d] = (X[:, d] - X[:, (k + 1) * NB:] @ L[(k + 1) * NB:, d]) @ inv[k]
    return L, X, 0


def backward_errors(S, X, B):
    """eta per right-hand side (row): ||x S - b||_inf / (||S||_inf ||x||_inf + ||b||_inf), in np.longdouble."""
    S, X, B = (np.asarray(a, dtype=np.longdouble) for a in (S, X, B))
    r = np.max(np.abs(X @ S - B), axis=1)
    den = np.max(np.sum(np.abs(S), axis=1)) * np.max(np.abs(X), axis=1) + np.max(np.abs(B), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, r / den, 0).astype(np.float64)


# ---- the exact cases ---------------------------------------------------------------------------------------------------------

def bidiagonal_case(m):
    """(S, L): L with diagonal 2 and subdiagonal 1, S = L L^T — every pivot, quotient and block inverse a power of two or a
    small integer."""
    L = 2.0 * np.eye(m) + np.diag(np.ones(m - 1), -1) if m > 1 else np.array([[2.0]])
    return L @ L.T, L


def diagonal_case(m, nrhs, seed):
    """(S, B, X): S diagonal with entries 4^p, B integers, X = B / s exactly."""
    rng = np.random.default_rng(seed)
    s = 4.0 ** rng.integers(0, 6, m)
    B = rng.integers(-2 ** 20, 2 ** 20, (nrhs, m)).astype(np.float64)
    return np.diag(s), B, B / s


def random_spd(m, log10_cond, seed):
    """A dense SPD matrix with eigenvalues spread evenly in log over `log10_cond` decades."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    S = (Q * 10.0 ** np.linspace(0.0, -log10_cond, m)) @ Q.T
    return (S + S.T) / 2.0
