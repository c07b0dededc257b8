"""NumPy restatement of ebm_ensemble_sums (the definition is the header text, include/ebm_hip.h): an explicit loop over the
blocks of 32 columns and over the columns of a block, vectorised over latitude only, so that NumPy performs the same IEEE
operations in the same order as the definition states them — every product and every sum a separate, once-rounded ufunc call
(NumPy fuses nothing across calls).  The GPU tests compare with it bit for bit."""
import numpy as np

from support import bits

BLOCK = 32


def ensemble_sums_ref(x, w=None, center=None):
    """x [nvars, ncol, nlat] (the fields in natural latitude order), w [ncol] or None (all 1.0), center [nvars, nlat] or None:
    returns [nvars, 3, nlat] = S0, S1, S2."""
    x = np.asarray(x, dtype=np.float64)
    nvars, ncol, nlat = x.shape
    w = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty((nvars, 3, nlat))
    with np.errstate(all="ignore"):
        for v in range(nvars):
            total = [np.zeros(nlat) for _ in range(3)]
            for b in range(0, ncol, BLOCK):
                part = [np.zeros(nlat) for _ in range(3)]
                for c in range(b, min(b + BLOCK, ncol)):
                    if w[c] == 0.0:
                        continue                                  # a zero weight removes the member
                    xc = x[v, c]
                    d = xc - center[v] if center is not None else xc
                    t1 = w[c] * d
                    t2 = t1 * d
                    ok = ~np.isnan(xc)                            # the NaN sentinels do not contribute
                    part[0] = np.where(ok, part[0] + w[c], part[0])
                    part[1] = np.where(ok, part[1] + t1, part[1])
                    part[2] = np.where(ok, part[2] + t2, part[2])
                for q in range(3):
                    total[q] = total[q] + part[q]                 # a block without a contributor adds its 0.0
            out[v] = total
    return out


def adds_per_term(m):
    """D(m): the rounded adds a term of a call over m columns can pass through — at most min(m, 32) - 1 inside its block (the
    first add of a block, to 0.0, is exact) and ceil(m / 32) - 1 over the blocks (the first, to 0.0, is exact again).  A sum
    whose every term passes through at most D rounded adds differs from the exact sum of its terms by at most
    gamma(D) sum|terms|, gamma(D) = D 2^-53 / (1 - D 2^-53) (Higham, Accuracy and Stability of Numerical Algorithms, 4.2)."""
    return 0 if m < 1 else min(m, BLOCK) + -(-m // BLOCK) - 2


def gamma(d):
    return d * 2.0 ** -53 / (1.0 - d * 2.0 ** -53)


def abs_term_sums(x, w=None, center=None):
    """[nvars, 3, nlat]: the sum of |t0|, |t1|, |t2| over the contributing columns (math.fsum-free, plain float64: it only
    scales error bounds)."""
    x = np.asarray(x, dtype=np.float64)
    nvars, ncol, nlat = x.shape
    w = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    d = x - center[:, None, :] if center is not None else x
    ok = ~np.isnan(x) & (w != 0.0)[None, :, None]
    t1 = w[None, :, None] * d
    terms = np.stack([np.broadcast_to(w[None, :, None], x.shape), t1, t1 * d], axis=1)      # [nvars, 3, ncol, nlat]
    return np.where(ok[:, None], np.abs(terms), 0.0).sum(axis=2)


def same_bits(a, b):
    """Bit for bit, except that NaN positions only have to coincide (a NaN's payload is not part of the definition)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return np.array_equal(bits(a)[keep], bits(b)[keep])
