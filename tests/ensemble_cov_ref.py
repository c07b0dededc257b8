"""NumPy restatement of the TERMS of ebm_ensemble_covariance (include/ebm_hip.h) — the float64 a and b of every member exactly
as the definition rounds them — and of the mirror rule.  The ORDER inside a matrix instruction is the hardware's, so the sums
here are taken in np.longdouble (64-bit mantissa on x86) and the device is held to the derived bound
    |out[i][j] - exact| <= (n + nblocks) * 2^-53 * T_ij * (1 + 2^-4),
n the members with nonzero weight, nblocks = ceil(ncol / K_COV_BLOCK), T_ij = sum |a * b| (covariance_bound).  The reference's
own error — n roundings of relative 2^-64 — is inside the last factor: n 2^-64 <= (n + 1) 2^-53 2^-4 for every n."""
import numpy as np

K_COV_BLOCK = 512            # kCovBlock of the header


def terms(xa, xb, w=None, center_a=None, center_b=None):
    """(a, b): float64 [ncol, nlat] each.  a = w_c * (x - center_a), b = y - center_b, each operation rounded once; +0.0
    where w_c == 0.0 or the cell is NaN."""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    ncol = xa.shape[0]
    w = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        da = xa if center_a is None else xa - np.asarray(center_a, dtype=np.float64)[None, :]
        a = w[:, None] * da
        b = xb if center_b is None else xb - np.asarray(center_b, dtype=np.float64)[None, :]
    out = w[:, None] == 0.0
    return np.where(out | np.isnan(xa), 0.0, a), np.where(out | np.isnan(xb), 0.0, b)


def is_symmetric_call(same_field, center_a, center_b):
    """Rule 6: one field against itself, the centers both absent or equal bit for bit."""
    if not same_field:
        return False
    if center_a is None or center_b is None:
        return center_a is None and center_b is None
    ca, cb = np.ascontiguousarray(center_a, dtype=np.float64), np.ascontiguousarray(center_b, dtype=np.float64)
    return ca.shape == cb.shape and np.array_equal(ca.view(np.uint64), cb.view(np.uint64))


def mirror(m):
    """The upper triangle (j >= i) copied onto the lower."""
    m = np.array(m)
    i, j = np.tril_indices(m.shape[0], -1)
    m[i, j] = m[j, i]
    return m


def ensemble_cov_ref(xa, xb, w=None, center_a=None, center_b=None, same_field=False):
    """(out, T, n): out [nlat, nlat] float64 = the np.longdouble sums of a * b rounded to double, T [nlat, nlat] = sum |a * b|,
    n = the number of members with w != 0.  With same_field and centers that make the call symmetric (rule 6) out and T are
    mirrored from j >= i."""
    a, b = terms(xa, xb, w, center_a, center_b)
    with np.errstate(all="ignore"):
        out = (a.astype(np.longdouble).T @ b.astype(np.longdouble)).astype(np.float64)
        T = (np.abs(a).astype(np.longdouble).T @ np.abs(b).astype(np.longdouble)).astype(np.float64)
    n = a.shape[0] if w is None else int(np.count_nonzero(np.asarray(w)))
    if is_symmetric_call(same_field, center_a, center_b):
        out, T = mirror(out), mirror(T)
    return out, T, n


def covariance_bound(T, n, ncol):
    nblocks = -(-ncol // K_COV_BLOCK)
    return (n + nblocks) * 2.0 ** -53 * T * (1.0 + 2.0 ** -4)
