"""The column scalars of include/ebm_hip.h (ebm_column_scalars: "THIS TEXT IS THE DEFINITION") restated in NumPy, one
operation per line of the definition, sequential sums, nothing vectorised across a reduction: the reference of
tests/test_gpu_column_scalars.py, itself held against ensemble.hemispheric_mean and hand-made rows by
tests/test_host_column_scalars.py.  A plain module, no fixtures."""
import numpy as np

KINDS = ("integral", "mean", "edge_ge", "edge_le")


def band_integral(f, x, k0, k1):
    """0.0, then + ((f[i] + f[i+1]) * (x[i+1] - x[i])) / 2.0 for i = k0 .. k1 - 1, strictly left to right."""
    acc = np.float64(0.0)
    for i in range(k0, k1):
        acc = acc + ((f[i] + f[i + 1]) * (x[i + 1] - x[i])) / np.float64(2.0)
    return acc


def edge(f, x, k0, k1, level, ge):
    """The first k in k0 .. k1 with f[k] >= level (ge) or f[k] <= level, interpolated; +Inf without one."""
    level = np.float64(level)
    K = None
    for k in range(k0, k1 + 1):
        if (f[k] >= level) if ge else (f[k] <= level):       # False for NaN
            K = k
            break
    if K is None:
        return np.float64(np.inf)
    if K == k0:
        return x[k0]
    a, b = f[K - 1], f[K]
    if not np.isfinite(a) or not np.isfinite(b):
        return x[K]
    t = (level - a) / (b - a)
    return x[K - 1] + t * (x[K] - x[K - 1])


def scalar(f, x, kind, k0, k1, level=0.0):
    """One scalar of one row f [nlat] on the grid x [nlat]."""
    f, x = np.asarray(f, dtype=np.float64), np.asarray(x, dtype=np.float64)
    assert kind in KINDS and 0 <= k0 <= k1 <= len(x) - 1 and f.shape == x.shape
    with np.errstate(all="ignore"):
        if kind in ("integral", "mean"):
            assert k0 < k1
            acc = band_integral(f, x, k0, k1)
            return acc if kind == "integral" else acc / (x[k1] - x[k0])
        assert not np.isnan(level)
        return edge(f, x, k0, k1, level, kind == "edge_ge")


def column_scalars(fields, x, specs):
    """[len(specs), ncol]: fields maps a name to [ncol, nlat]; specs are (kind, name, k0, k1[, level])."""
    ncol = next(iter(fields.values())).shape[0]
    out = np.empty((len(specs), ncol))
    for s, one in enumerate(specs):
        kind, name, k0, k1 = one[:4]
        level = one[4] if len(one) > 4 and one[4] is not None else 0.0
        for c in range(ncol):
            out[s, c] = scalar(fields[name][c], x, kind, k0, k1, level)
    return out
