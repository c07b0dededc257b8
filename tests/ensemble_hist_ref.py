"""NumPy restatement of ebm_ensemble_range and ebm_ensemble_histogram (the definitions are the header text,
include/ebm_hip.h), loop for loop: an explicit loop over the blocks of columns and over the columns of a block, vectorised
over latitude only, every difference, product and sum a separate, once-rounded ufunc call, the comparisons strict where the
definition says so.  The GPU tests compare with it bit for bit (same_bits of ensemble_sums_ref.py)."""
import numpy as np

from ensemble_sums_ref import same_bits  # noqa: F401  (re-exported: the comparison of every test of these calls)

HIST_BLOCK = 256
RANGE_BLOCK = 32                     # any blocking gives the same bits: the tests also walk with 1 and with ncol


def ensemble_range_ref(x, w=None, block=RANGE_BLOCK):
    """x [nvars, ncol, nlat], w [ncol] or None: returns [nvars, 3, nlat] = n, min, max."""
    x = np.asarray(x, dtype=np.float64)
    nvars, ncol, nlat = x.shape
    w = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty((nvars, 3, nlat))
    for v in range(nvars):
        n, mn, mx = np.zeros(nlat), np.full(nlat, np.inf), np.full(nlat, -np.inf)
        for b in range(0, ncol, block):
            pn, pmn, pmx = np.zeros(nlat), np.full(nlat, np.inf), np.full(nlat, -np.inf)
            for c in range(b, min(b + block, ncol)):
                if w[c] == 0.0:
                    continue                                      # a zero weight removes the member
                xc = x[v, c]
                ok = ~np.isnan(xc)
                with np.errstate(invalid="ignore"):
                    pn = np.where(ok, pn + 1.0, pn)
                    pmn = np.where(ok & (xc < pmn), xc, pmn)      # strict: the first of equal extremes keeps its bits
                    pmx = np.where(ok & (xc > pmx), xc, pmx)
            n = n + pn
            mn = np.where(pmn < mn, pmn, mn)
            mx = np.where(pmx > mx, pmx, mx)
        out[v] = n, mn, mx
    return out


def slots_ref(xc, lo, hi, nbins):
    """The slot of every value of xc [nlat] that is not NaN (NaN: any slot, never used): 0 below lo, nbins + 1 at or above
    hi, else 1 + min(int(t), nbins - 1), t = (x - lo) * s, s = nbins / (hi - lo).  Returns (slot, t)."""
    s = float(nbins) / (hi - lo)                                  # one IEEE division
    with np.errstate(all="ignore"):
        d = xc - lo                                               # a rounded difference ...
        t = d * s                                                 # ... times a rounded product
        below, above = xc < lo, xc >= hi
        inner = ~(below | above | np.isnan(xc))
        i = np.minimum(np.where(inner, t, 0.0).astype(np.int64), nbins - 1)
    return np.where(below, 0, np.where(above, nbins + 1, 1 + i)), t


def ensemble_histogram_ref(x, lo, hi, nbins, w=None):
    """x [nvars, ncol, nlat] (entry v's field: a repeated field is a repeated row), lo, hi [nvars, nlat], w [ncol] or None:
    returns [nvars, nbins + 2, nlat]."""
    x = np.asarray(x, dtype=np.float64)
    nvars, ncol, nlat = x.shape
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    w = np.ones(ncol) if w is None else np.asarray(w, dtype=np.float64)
    out = np.empty((nvars, nbins + 2, nlat))
    lat = np.arange(nlat)
    for v in range(nvars):
        total = np.zeros((nbins + 2, nlat))
        for b in range(0, ncol, HIST_BLOCK):
            part = np.zeros((nbins + 2, nlat))
            for c in range(b, min(b + HIST_BLOCK, ncol)):
                if w[c] == 0.0:
                    continue
                xc = x[v, c]
                ok = ~np.isnan(xc)
                slot, _ = slots_ref(xc, lo[v], hi[v], nbins)
                part[slot[ok], lat[ok]] = part[slot[ok], lat[ok]] + w[c]         # one slot per latitude: no repeated index
            total = total + part                                  # a block without a contributor adds its 0.0
        out[v] = total
    return out
