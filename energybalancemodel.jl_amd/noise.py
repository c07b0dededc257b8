"""Host restatement of the forcing noise's definition (include/ebm_hip.h, ebm_set_column_noise).

The stepping never uses this module: the noise is drawn on the device, inside the step kernels.  It is here so that a
caller (and the test suite) can check the device's innovations and recompute a member's N_c sequence on the host:
``philox4x32_10`` and ``uniforms`` agree with the device bit for bit; ``innovations`` to a few ulps (NumPy has no
``cospi``, so ``cos(2 pi u2)`` stands in for it).
"""
from __future__ import annotations

import math

import numpy as np

from ._lib import as_f64

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): ``counter`` [..., 4] and ``key`` [..., 2] of 32-bit words (broadcast against each
    other); returns the [..., 4] uint32 output words."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m0, m1 = np.uint64(PHILOX_M[0]), np.uint64(PHILOX_M[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(PHILOX_W[0])) & _MASK
            k1 = (k1 + np.uint64(PHILOX_W[1])) & _MASK
        p0, p1 = m0 * c0, m1 * c2                    # < 2^64: exact
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniforms(w):
    """(u1, u2) of the definition's step 2 from output words ``w`` [..., 4]: u1 in (0, 1], u2 in [0, 1), exact."""
    w = np.asarray(w, dtype=np.uint64)
    a = (w[..., 0] << np.uint64(21)) | (w[..., 1] >> np.uint64(11))
    b = (w[..., 2] << np.uint64(21)) | (w[..., 3] >> np.uint64(11))
    return (a + np.uint64(1)).astype(np.float64) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53


def words(seed: int, streams, first_step: int, nsteps: int):
    """Philox output words [len(streams), nsteps, 4] for steps first_step .. first_step + nsteps - 1."""
    s = np.asarray(streams, dtype=np.uint64).reshape(-1, 1)
    n = np.arange(int(first_step), int(first_step) + int(nsteps), dtype=np.uint64).reshape(1, -1)
    ctr = np.stack(np.broadcast_arrays(n & _MASK, n >> np.uint64(32), s & _MASK, s >> np.uint64(32)), axis=-1)
    seed = np.uint64(int(seed))
    return philox4x32_10(ctr, np.array([seed & _MASK, seed >> np.uint64(32)], dtype=np.uint64))


def innovations(seed: int, streams, first_step: int, nsteps: int):
    """xi(seed, stream, n) [len(streams), nsteps]: the device's ``ebm_noise_innovations`` to a few ulps."""
    u1, u2 = uniforms(words(seed, streams, first_step, nsteps))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def ar1(xi, sigma, rho, N0=None):
    """The recurrence N <- rho*N + s*xi, s = sigma*sqrt(1 - rho^2), for innovations ``xi`` [ncol, nsteps]: returns
    N [ncol, nsteps] (N after each step) exactly as the device rounds it (two products and one sum)."""
    xi = np.asarray(xi, dtype=np.float64)
    ncol = xi.shape[0]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (ncol,))
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), (ncol,))
    s = sigma * np.sqrt(1.0 - rho * rho)
    N = np.zeros(ncol) if N0 is None else np.array(N0, dtype=np.float64)
    out = np.empty_like(xi)
    for i in range(xi.shape[1]):
        N = rho * N + s * xi[:, i]
        out[:, i] = N
    return out


def rho_from_tau(tau_years, dt_years):
    """Lag-one-step autocorrelation of an AR(1) process with e-folding time ``tau`` (years) at step ``dt`` (years)."""
    tau = np.asarray(tau_years, dtype=np.float64)
    if not np.all(np.isfinite(tau)) or np.any(tau <= 0.0):
        raise ValueError(f"tau must be finite and > 0 (years), got {tau_years!r}")
    return np.exp(-float(dt_years) / tau)


def check_args(ncol, dt, sigma, rho=None, seed=0, streams=None, tau=None):
    """The host-side checks of ``Engine.set_column_noise`` for ``ncol`` columns stepped with ``dt`` (years): returns the
    [ncol] arrays sigma, rho, streams (uint64, or None for the default stream_c = c) and the seed."""
    sig = np.array(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (ncol,))) if np.ndim(sigma) == 0 \
        else as_f64(sigma, (ncol,))
    if not np.all(np.isfinite(sig)) or np.any(sig < 0.0):
        raise ValueError("sigma: the stationary standard deviation must be finite and >= 0 (W m^-2)")
    if rho is not None and tau is not None:
        raise ValueError("give rho or tau, not both")
    if tau is not None:
        r = rho_from_tau(np.broadcast_to(np.asarray(tau, dtype=np.float64), (ncol,)), dt)
    else:
        r = np.zeros(ncol) if rho is None else np.asarray(rho, dtype=np.float64)
        r = np.array(np.broadcast_to(r, (ncol,))) if r.ndim == 0 else as_f64(r, (ncol,))
    r = np.ascontiguousarray(r, dtype=np.float64)
    if not np.all(np.isfinite(r)) or np.any(r < 0.0) or np.any(r >= 1.0):
        raise ValueError("rho: the lag-one-step autocorrelation must lie in [0, 1)")
    st = None
    if streams is not None:
        raw = np.asarray(streams)
        if raw.shape != (ncol,):
            raise ValueError(f"streams: expected {ncol} stream ids, got shape {raw.shape}")
        if raw.dtype.kind not in "ui" or (raw.dtype.kind == "i" and np.any(raw < 0)):
            raise ValueError("streams: expected non-negative integer stream ids")
        st = np.ascontiguousarray(raw, dtype=np.uint64)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed: expected an integer in [0, 2^64)")
    return sig, r, st, seed
