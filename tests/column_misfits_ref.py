"""NumPy restatement of ebm_column_misfits (the definition is the header text, include/ebm_hip.h): the 128 chains (l, e) as one
array [ncol, 128] indexed by 2l + e = k mod 128, an explicit loop over the variables in the order of the call and over the
rounds i = 0, 1, ... of 128 cells within each, then the parity add and the tree over s = 32, 16, 8, 4, 2, 1 — vectorised over
the columns and the chains only, so that NumPy performs the same IEEE operations in the same order as the definition states
them, every difference, product and sum a separate, once-rounded ufunc call.  The GPU tests compare with it bit for bit."""
import numpy as np

from ensemble_sums_ref import same_bits  # noqa: F401  (the comparison of every user of this file)

LANES = 64


def rounds_of(nlat):
    """ceil(U / 64) with U = ceil(nlat / 2): the units a lane walks per variable, at most."""
    return -(-((nlat + 1) // 2) // LANES)


def column_misfits_ref(x, targets, rw=None):
    """x [nvars, ncol, nlat] (the fields in natural latitude order), targets [ntargets, nvars, nlat] (NaN: no observation),
    rw [nvars, nlat] or None (all 1.0): returns [ntargets, 2, ncol] = J, N."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(targets, dtype=np.float64)
    nvars, ncol, nlat = x.shape
    ntargets = y.shape[0]
    assert y.shape == (ntargets, nvars, nlat)
    r = np.ones((nvars, nlat)) if rw is None else np.asarray(rw, dtype=np.float64)
    assert r.shape == (nvars, nlat)
    rounds, width = rounds_of(nlat), 2 * LANES
    pad = rounds * width - nlat                          # cells that do not exist: NaN never contributes
    xp = np.concatenate([x, np.full((nvars, ncol, pad), np.nan)], axis=2)
    yp = np.concatenate([y, np.full((ntargets, nvars, pad), np.nan)], axis=2)
    rp = np.concatenate([r, np.zeros((nvars, pad))], axis=1)
    out = np.empty((ntargets, 2, ncol))
    with np.errstate(all="ignore"):
        for t in range(ntargets):
            chain, count = np.zeros((ncol, width)), np.zeros((ncol, width))
            for v in range(nvars):                       # one accumulator runs across the variables
                for i in range(rounds):
                    cells = slice(width * i, width * (i + 1))
                    xs, ys, rs = xp[v, :, cells], yp[t, v, cells][None, :], rp[v, cells][None, :]
                    d = xs - ys
                    t1 = rs * d
                    t2 = t1 * d
                    ok = (rs != 0.0) & ~np.isnan(ys) & ~np.isnan(xs)
                    chain = np.where(ok, chain + t2, chain)
                    count = np.where(ok, count + 1.0, count)
            for acc, q in ((chain, 0), (count, 1)):
                lane = acc[:, 0::2] + acc[:, 1::2]      # chain(l, 0) + chain(l, 1)
                s = LANES // 2
                while s >= 1:
                    lane[:, :s] = lane[:, :s] + lane[:, s:2 * s]
                    s //= 2
                out[t, q] = lane[:, 0]
    return out


def column_misfits_fast(x, targets, rw=None):
    """The same quantity in whatever order NumPy likes (not bit for bit): what a caller would write on downloaded fields."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(targets, dtype=np.float64)
    r = np.ones(x.shape[::2]) if rw is None else np.asarray(rw, dtype=np.float64)
    out = np.empty((y.shape[0], 2, x.shape[1]))
    with np.errstate(all="ignore"):
        for t in range(y.shape[0]):
            d = x - y[t][:, None, :]
            ok = (r != 0.0)[:, None, :] & ~np.isnan(d)
            out[t, 0] = np.where(ok, r[:, None, :] * d * d, 0.0).sum(axis=(0, 2))
            out[t, 1] = ok.sum(axis=(0, 2))
    return out
