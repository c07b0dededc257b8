"""NumPy restatement of the stated terms of ebm_update_columns (include/ebm_hip.h), shared by the GPU and the host tests.

innovations     d[c, j] = (target[j] + e[c, j]) - scale * xo[c, j], each operation rounded once in float64; +0.0 where target
                or xo is NaN.
update_exact    integer data: every product and partial sum is an integer far below 2^53, so x + sum_j d g in int64 IS the
                result, bit for bit, whatever the order inside the matrix instruction.
update_ref      real data: the sum of the float64 products' exact values in np.longdouble (64-bit mantissa on x86), the
                absolute sum T = sum_j |d g| and n_obs, the number of nonzero terms; update_bound is the header's bound
                n_obs 2^-53 T (1 + 2^-4) on the accumulator.
clamp           the strict comparisons of the write; NaN passes."""
import numpy as np


def innovations(xo, target, scale, perturb=None):
    xo, target = np.asarray(xo, dtype=np.float64), np.asarray(target, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.float64(scale) * xo
        t = target[None, :] + perturb if perturb is not None else np.broadcast_to(target[None, :], xo.shape)
        d = t - s
    return np.where(np.isnan(target)[None, :] | np.isnan(xo), 0.0, d)


def clamp(x, lo=None, hi=None):
    lo = -np.inf if lo is None else lo
    hi = np.inf if hi is None else hi
    with np.errstate(invalid="ignore"):
        x = np.where(x < lo, lo, x)
        return np.where(x > hi, hi, x)


def update_exact(x, d, gain, lo=None, hi=None):
    """x [ncol, nlat], d [ncol, nlat], gain [nlat, nlat] of integers: x + d @ gain.T in int64, then one float64 add with the
    sign of zero the device's add gives (x + acc with acc = +0.0 for an integer zero), then the clamp."""
    assert (d == np.rint(d)).all() and (gain == np.rint(gain)).all()
    acc = d.astype(np.int64) @ gain.astype(np.int64).T
    assert np.abs(d).max(initial=0.0) * np.abs(gain).max(initial=0.0) * d.shape[1] < 2.0 ** 52
    with np.errstate(invalid="ignore"):
        return clamp(x + acc.astype(np.float64), lo, hi)


def update_ref(d, gain):
    """(acc, T, n_obs), each [ncol, nlat(k)]: the longdouble sum over j of d[c, j] * gain[k, j] (the float64 product of two
    float64 numbers is exact in longdouble only up to its 64 bits: the bound's factor 1 + 2^-4 covers that), the sum of the
    absolute terms and the number of nonzero terms."""
    dl, gl = np.asarray(d, dtype=np.longdouble), np.asarray(gain, dtype=np.longdouble)
    acc = dl @ gl.T
    T = np.abs(dl) @ np.abs(gl).T
    n = (np.asarray(d) != 0.0).astype(np.float64) @ (np.asarray(gain) != 0.0).astype(np.float64).T
    return acc, T, n


def update_bound(T, n_obs):
    return n_obs * 2.0 ** -53 * np.asarray(T, dtype=np.float64) * (1.0 + 2.0 ** -4)
