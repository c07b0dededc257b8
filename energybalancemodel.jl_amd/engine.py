"""Engine: a thin object wrapper over one ebm_handle_t (include/ebm_hip.h).

Owns the device-resident state of ``ncol`` independent meridians (longitudes and/or ensemble
members) of ``nlat`` cells, including the T0 warm start that the reference keeps in a
module-level closure (reference src/miz.jl:47,64).
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib, noise
from ._lib import FIELD, GRID, MODEL, PARAM_ORDER, as_f64, check, dptr, field_ids, iptr

MIZ_PROGNOSTIC = ("Ei", "Ew", "h", "D", "phi")
MIZ_DIAGNOSTIC = ("Tw", "Ti", "n", "E", "T")
CLASSIC_PROGNOSTIC = ("E", "Tg")
CLASSIC_DIAGNOSTIC = ("T", "h")
_HOST = object()        # the destination of a reduction whose result comes back as a new host array (Engine._reduced)


def as_names(names) -> tuple:
    """A caller's field list as a tuple; one field may be given as its name."""
    return (names,) if isinstance(names, str) else tuple(names)


def _refuse_repeats(names):
    if len(set(names)) != len(names):
        raise ValueError(f"names: a field is listed twice in {names}")


def schedule_words(forcing):
    """The 9 words of one column's schedule (include/ebm_hip.h): base, peak, cool, the two rates
    and Forcing.domain[1:]; a constant Forcing is a schedule that never leaves its first hold."""
    if forcing.constant:
        return [forcing.base, forcing.base, forcing.base, 0.0, 0.0, np.inf, np.inf, np.inf, np.inf]
    d = forcing.domain
    return [forcing.base, forcing.peak, forcing.cool, float(forcing.rates[0]), float(forcing.rates[1]),
            float(d[1]), float(d[2]), float(d[3]), float(d[4])]


def cos2pit(t: float) -> float:
    """cos(2.0*pi*t) exactly as the reference writes it (src/miz.jl:11, src/classic.jl:24)."""
    return math.cos(2.0 * math.pi * t)


def param_vector(par, defaults) -> np.ndarray:
    get = par.get if hasattr(par, "get") else (lambda k, d: getattr(par, k, d))
    return np.array([get(k, defaults[k]) for k in PARAM_ORDER], dtype=np.float64)


def param_matrix(rows, base, defaults) -> np.ndarray:
    """The [len(rows), 25] parameter rows of ebm_set_column_params: row m is ``base`` (a dict / Collection of parameter
    values, missing names from ``defaults``, as ``param_vector``) with the overrides of ``rows[m]`` — a dict or
    Collection of parameter name -> value, e.g. ``[{"D": d} for d in Ds]``; None or {} keeps ``base``.  Unknown
    names raise ValueError."""
    rows = list(rows)
    out = np.empty((len(rows), len(PARAM_ORDER)), dtype=np.float64)
    out[:] = param_vector(base, defaults)
    index = {k: i for i, k in enumerate(PARAM_ORDER)}
    for m, row in enumerate(rows):
        if row is None:
            continue
        if not hasattr(row, "items"):
            raise TypeError(f"member {m}: expected a dict of parameter overrides, got {type(row).__name__}")
        for k, v in row.items():
            if k not in index:
                raise ValueError(f"member {m}: unknown parameter {k!r} (expected one of {', '.join(PARAM_ORDER)})")
            out[m, index[k]] = float(v)
    return out


def _env_int(name):
    v = os.environ.get(name)
    return None if v in (None, "") else int(v)


def _flag(v) -> int:
    return int(bool(v))


class Engine:
    """``cells_per_thread`` (2 or 4; default 4), ``use_graph`` (True / False; default: by size), ``prefetch_cols`` and
    ``launch_chains`` (1 or 2; default 1), ``integrate_steps_per_launch`` (default 64; 1 = ``integrate`` launches every step),
    ``fused_state_in_lds`` (True / False; default: by column count) and ``elide_zero_lines`` (True / False; default: on
    where the one-step kernel that derives phi is) are the launch options of ``ebm_create_ex`` (include/ebm_hip.h: struct ebm_options).
    The LIBRARY reads no environment variable; this mirror maps EBM_CELLS_PER_THREAD, EBM_GRAPH and
    EBM_PREFETCH_COLS to those options when the corresponding argument is left at None — the knobs of the
    test suite and of the A/B timing scripts under tests/tools/."""

    def __init__(self, model: str, grid_kind: str, x, params25, dt: float, ncol: int = 1,
                 device: int = 0, *, cells_per_thread=None, use_graph=None, prefetch_cols=None, launch_chains=None,
                 integrate_steps_per_launch=None, fused_state_in_lds=None, elide_zero_lines=None):
        if model not in MODEL:
            raise ValueError(f"unknown model {model!r}: expected 'MIZ', 'Classic' or the extension 'MIZ_IMEX'")
        self.lib = _lib.load()
        self.model, self.grid_kind = model, grid_kind
        self.device = int(device)
        self.x = as_f64(x)
        self.nlat, self.ncol, self.dt = int(self.x.shape[0]), int(ncol), float(dt)
        self.params = as_f64(params25, (len(PARAM_ORDER),))
        opt = _lib.Options()
        check(self.lib.ebm_options_default(C.byref(opt)), "ebm_options_default")
        if cells_per_thread is None:
            cells_per_thread = _env_int("EBM_CELLS_PER_THREAD")
            if cells_per_thread == 2 and (self.nlat > 1536 or model == "MIZ_IMEX"):
                cells_per_thread = None              # the knob asks for 2 "where it exists"
        if use_graph is None and _env_int("EBM_GRAPH") is not None:
            use_graph = bool(_env_int("EBM_GRAPH"))
        if prefetch_cols is None:
            prefetch_cols = _env_int("EBM_PREFETCH_COLS")
        for name, value, conv in (("cells_per_thread", cells_per_thread, int), ("use_graph", use_graph, _flag),
                                  ("prefetch_cols", prefetch_cols, lambda v: max(0, int(v))), ("launch_chains", launch_chains, int),
                                  ("integrate_steps_per_launch", integrate_steps_per_launch, int),
                                  ("fused_state_in_lds", fused_state_in_lds, _flag), ("elide_zero_lines", elide_zero_lines, _flag)):
            if value is not None:                    # None: the library's default stays
                setattr(opt, name, conv(value))
        h = C.c_void_p()
        gk = GRID["identity"] if grid_kind == "identity" else GRID["nonuniform"]
        check(self.lib.ebm_create_ex(C.byref(h), MODEL[model], gk, self.nlat, self.ncol,
                                     dptr(self.x), dptr(self.params), self.dt, int(device), C.byref(opt)),
              "ebm_create")
        self._h = h
        self.nt = None

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.ebm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ------------------------------------------------------------------------
    @property
    def prognostic(self):
        return MIZ_PROGNOSTIC if self.model.startswith("MIZ") else CLASSIC_PROGNOSTIC

    @property
    def diagnostic(self):
        return MIZ_DIAGNOSTIC if self.model.startswith("MIZ") else CLASSIC_DIAGNOSTIC

    def set_field(self, name: str, values):
        a = as_f64(values).reshape(self.ncol, self.nlat)
        check(self.lib.ebm_set_field(self._h, FIELD[name], dptr(a)), f"ebm_set_field({name})")

    def get_field(self, name: str) -> np.ndarray:
        out = np.empty((self.ncol, self.nlat))
        check(self.lib.ebm_get_field(self._h, FIELD[name], dptr(out)), f"ebm_get_field({name})")
        return out

    def get_field_as_of(self, name: str, step: int) -> np.ndarray:
        """The field as written by global step ``step`` (0-based), however far the state has moved on since;
        StaleFieldError if another step wrote it last (ebm_get_field_as_of)."""
        out = np.empty((self.ncol, self.nlat))
        check(self.lib.ebm_get_field_as_of(self._h, FIELD[name], int(step), dptr(out)), f"ebm_get_field_as_of({name})")
        return out

    def field_step(self, name: str) -> dict:
        """dict(written_step, state_step, current): which step last wrote the field, where the state is, and
        whether the field may be read now (ebm_field_step)."""
        w, s_, c = C.c_longlong(), C.c_longlong(), C.c_int()
        check(self.lib.ebm_field_step(self._h, FIELD[name], C.byref(w), C.byref(s_), C.byref(c)), "ebm_field_step")
        return dict(written_step=w.value, state_step=s_.value, current=bool(c.value))

    def set_state(self, state: dict):
        for k, v in state.items():
            self.set_field(k, v)

    def get_state(self, names=None) -> dict:
        names = names or (self.prognostic + self.diagnostic)
        return {k: self.get_field(k) for k in names}

    def hemispheric_mean(self, name: str) -> np.ndarray:
        """Per-column hemispheric mean of a field, reduced on the device (ebm_hemispheric_mean)."""
        return self._reduced("ebm_hemispheric_mean", (self.ncol,), _HOST, FIELD[name])

    def hemispheric_mean_device(self, name: str, dev_ptr: int):
        """Same reduction, result left on the device at ``dev_ptr`` (``ncol`` doubles, e.g. the
        ``data_ptr()`` of a torch tensor on this engine's device)."""
        check(self.lib.ebm_hemispheric_mean_device(self._h, FIELD[name], C.c_void_p(dev_ptr)),
              "ebm_hemispheric_mean_device")

    def _fields(self, names, arg="names", most=None, what="fields", t0_note=True, repeats=True):
        """(names, field ids) of a caller's field list, or ValueError: more than ``most`` entries or none (None: no bound), a
        name that is not a solution variable of this model, a field listed twice (unless ``repeats``)."""
        names = as_names(names)
        allowed = self.prognostic + self.diagnostic
        if most is not None and not 1 <= len(names) <= most:
            raise ValueError(f"{arg}: expected between 1 and {most} {what} of the {self.model} model")
        for n in names:
            if not isinstance(n, str) or n not in allowed:
                raise ValueError(f"{arg}: unknown field {n!r} for the {self.model} model (expected one of {', '.join(allowed)}"
                                 + ("; the warm start T0 is not a solution variable)" if t0_note else ")"))
        if not repeats:
            _refuse_repeats(names)
        return names, [FIELD[n] for n in names]

    def _check_weights(self, weights):
        """The member weights of the ensemble reductions as a contiguous float64 array [ncol], or None."""
        w = None if weights is None else as_f64(weights, (self.ncol,))
        if w is not None and not np.isfinite(w).all():
            c = int(np.flatnonzero(~np.isfinite(w))[0])
            raise ValueError(f"weights[{c}] = {w[c]} is not finite (negative and zero weights are legal)")
        return w

    def _check_sums_args(self, names, weights=None, center=None):
        """The host-side checks of ``ensemble_sums`` (no device call): returns (names, field ids, weights [ncol] or None,
        center [nvars, nlat] or None) with contiguous float64 arrays.  A field listed twice is refused before the weights
        are looked at."""
        names, ids = self._fields(names, most=12, repeats=False)
        w = self._check_weights(weights)
        ctr = None if center is None else as_f64(center, (len(names), self.nlat))
        if ctr is not None and not np.isfinite(ctr).all():
            raise ValueError("center: expected finite values")
        return names, ids, w, ctr

    def _check_range_args(self, names, weights=None):
        """The host-side checks of ``ensemble_range`` (no device call): returns (names, field ids, weights [ncol] or None).  A
        field listed twice is refused after the weights have been looked at."""
        names, ids = self._fields(names, most=12, what="entries of fields")
        w = self._check_weights(weights)
        _refuse_repeats(names)
        return names, ids, w

    def _check_histogram_args(self, names, lo, hi, nbins, weights=None):
        """The host-side checks of ``ensemble_histogram`` (no device call): returns (names, field ids, weights [ncol] or
        None, (lo, hi)), the edges each [len(names), nlat], with contiguous float64 arrays.  A field may be listed several
        times."""
        names, ids = self._fields(names, most=12, what="entries of fields")
        w = self._check_weights(weights)
        if isinstance(nbins, (bool, np.bool_)) or not isinstance(nbins, (int, np.integer)) or not 1 <= int(nbins) <= 64:
            raise ValueError(f"nbins: expected an int between 1 and 64, got {nbins!r}")
        lo, hi = as_f64(lo, (len(names), self.nlat)), as_f64(hi, (len(names), self.nlat))
        with np.errstate(all="ignore"):
            width = hi - lo
            ok = np.isfinite(lo) & np.isfinite(hi) & (lo < hi) & np.isfinite(width) & np.isfinite(float(nbins) / width)
        if not ok.all():
            v, k = (int(i[0]) for i in np.nonzero(~ok))
            raise ValueError(f"lo[{v}][{k}] = {lo[v, k]}, hi[{v}][{k}] = {hi[v, k]}: expected finite edges with lo < hi "
                             "(and finite hi - lo and nbins / (hi - lo))")
        return names, ids, w, (lo, hi)

    @staticmethod
    def _check_dev_ptr(dev_ptr):
        if not isinstance(dev_ptr, (int, np.integer)) or isinstance(dev_ptr, (bool, np.bool_)) or int(dev_ptr) == 0:
            raise ValueError(f"dev_ptr: expected a device address (int), got {dev_ptr!r}")
        return C.c_void_p(int(dev_ptr))

    def _reduced(self, fn, shape, dev_ptr, *args):
        """The call of a host / ``_device`` pair, after the pair's checks.  Each ``x_device`` method is the body of its pair and
        ``x`` calls it with _HOST for an address: then ``fn(handle, *args, out)`` writes a new host array of ``shape``, which
        is returned; else ``fn_device(handle, *args, dev_ptr)`` leaves the same packed result at that device address."""
        if dev_ptr is _HOST:
            out = np.full(shape, np.nan)
            check(getattr(self.lib, fn)(self._h, *args, dptr(out)), fn)
            return out
        ptr = self._check_dev_ptr(dev_ptr)
        check(getattr(self.lib, fn + "_device")(self._h, *args, ptr), fn + "_device")

    def ensemble_sums(self, names, weights=None, center=None) -> np.ndarray:
        """ebm_ensemble_sums (the definition is in include/ebm_hip.h): the weighted sums ACROSS the columns, per latitude,
        reduced on the device — ndarray [len(names), 3, nlat] of S0 = sum w_c, S1 = sum w_c d and S2 = sum (w_c d) d with
        d = x - center[v, k] (d = x without ``center``), over the columns with w_c != 0 whose cell is not NaN (the sentinels
        of Ti and Tw; a zero weight removes the member; +-Inf propagates).  ``weights`` [ncol] (None: all 1.0; negative ones
        are legal), ``center`` [len(names), nlat].  Every product and sum is rounded once, in a fixed order — blocks of 32
        columns in ascending column order, then the block partials in ascending order — so the bits do not depend on the run,
        the launch geometry or the layout the handle holds the rows in; no field is converted.  StaleFieldError for a stale
        diagnostic field, as ``hemispheric_mean``.  The step clock, the counters and ``field_step`` are unchanged."""
        return self.ensemble_sums_device(names, _HOST, weights, center)

    def ensemble_sums_device(self, names, dev_ptr: int, weights=None, center=None):
        """Same reduction, the packed [len(names), 3, nlat] result left on the device at ``dev_ptr`` (e.g. the ``data_ptr()``
        of a torch tensor on this engine's device: the payload of an all-reduce between shards)."""
        names, ids, w, ctr = self._check_sums_args(names, weights, center)
        return self._reduced("ebm_ensemble_sums", (len(names), 3, self.nlat), dev_ptr, len(ids), field_ids(ids), dptr(w), dptr(ctr))

    def ensemble_range(self, names, weights=None) -> np.ndarray:
        """ebm_ensemble_range (the definition is in include/ebm_hip.h): ndarray [len(names), 3, nlat] of the number n of
        contributing columns, their minimum and their maximum, per latitude, reduced on the device.  A column contributes iff
        its weight is not 0 and its cell is not NaN (``weights`` [ncol], None: all 1.0; a weight acts only through being zero
        or not).  +-Inf is data; no contributor gives n = 0, min = +Inf, max = -Inf; of several equal extremes (+0.0, -0.0)
        the first in ascending column order gives the bits.  Rows are read where they lie: no field is converted, the step
        clock, the counters and ``field_step`` are unchanged.  StaleFieldError for a stale diagnostic field."""
        return self.ensemble_range_device(names, _HOST, weights)

    def ensemble_range_device(self, names, dev_ptr: int, weights=None):
        """Same reduction, the packed [len(names), 3, nlat] result left on the device at ``dev_ptr``."""
        names, ids, w = self._check_range_args(names, weights)
        return self._reduced("ebm_ensemble_range", (len(names), 3, self.nlat), dev_ptr, len(ids), field_ids(ids), dptr(w))

    def ensemble_histogram(self, names, lo, hi, nbins: int, weights=None) -> np.ndarray:
        """ebm_ensemble_histogram (the definition is in include/ebm_hip.h): ndarray [len(names), nbins + 2, nlat], per entry
        and latitude the summed weights of the contributing columns whose value x falls below ``lo`` (slot 0), into bin
        min(int((x - lo) * s), nbins - 1) with s = nbins / (hi - lo) (slots 1 ... nbins), or at and above ``hi`` (slot
        nbins + 1).  ``lo``, ``hi`` [len(names), nlat]: finite, lo < hi; 1 <= nbins <= 64.  A field may be listed several
        times, each entry with its own edges.  The weights of a slot are added in a fixed order — blocks of 256 columns in
        ascending column order, then the block partials in ascending order; with ``weights`` None every slot is an exact
        count, so the histograms of shards add to the unsharded one bit for bit."""
        return self.ensemble_histogram_device(names, lo, hi, nbins, _HOST, weights)

    def ensemble_histogram_device(self, names, lo, hi, nbins: int, dev_ptr: int, weights=None):
        """Same reduction, the packed [len(names), nbins + 2, nlat] result left on the device at ``dev_ptr``."""
        names, ids, w, (lo, hi) = self._check_histogram_args(names, lo, hi, nbins, weights)
        return self._reduced("ebm_ensemble_histogram", (len(names), int(nbins) + 2, self.nlat), dev_ptr, len(ids), field_ids(ids),
                             dptr(w), int(nbins), dptr(lo), dptr(hi))

    def check_covariance_args(self, name_a, name_b=None, weights=None, center_a=None, center_b=None):
        """The host-side checks of ``ensemble_covariance`` (no device call; the rules of ebm_ensemble_covariance in
        include/ebm_hip.h): returns (field id of ``name_a``, field id of ``name_b`` — of ``name_a`` again when ``name_b`` is
        None —, weights [ncol] or None, center_a [nlat] or None, center_b [nlat] or None) with contiguous float64 arrays.
        The fields are looked at first, then the weights, then the centers; the message names the offending column or the
        center and its latitude."""
        ids = []
        for arg, n in (("name_a", name_a), ("name_b", name_a if name_b is None else name_b)):
            if not isinstance(n, str):
                raise ValueError(f"{arg}: expected one field name, got {n!r}")
            ids.append(self._fields((n,), arg=arg)[1][0])
        w = self._check_weights(weights)
        centers = []
        for arg, c in (("center_a", center_a), ("center_b", center_b)):
            c = None if c is None else as_f64(c, (self.nlat,))
            if c is not None and not np.isfinite(c).all():
                k = int(np.flatnonzero(~np.isfinite(c))[0])
                raise ValueError(f"{arg}[{k}] = {c[k]} is not finite")
            centers.append(c)
        return ids[0], ids[1], w, centers[0], centers[1]

    def ensemble_covariance(self, name_a, name_b=None, weights=None, center_a=None, center_b=None) -> np.ndarray:
        """ebm_ensemble_covariance (the definition is in include/ebm_hip.h): ndarray [nlat, nlat], ``[i, j]`` = the sum over
        the columns of a * b with a = w_c * (x - center_a[i]), x the cell of ``name_a`` at latitude i, and b = y -
        center_b[j], y the cell of ``name_b`` (None: ``name_a``) at latitude j, reduced on the device with the fp64 matrix
        instruction.  a and b are +0.0 where w_c == 0 or the cell is NaN (the sentinels of Ti and Tw): a zero weight removes
        the member; +-Inf follows IEEE (Inf * 0 is NaN).  ``weights`` [ncol] (None: all 1.0; negative ones are legal),
        ``center_a``, ``center_b`` [nlat] (None: nothing is subtracted).  The order is fixed — blocks of 512 columns, inside
        a block one matrix instruction per four columns in ascending order, then the block partials in ascending order — so
        the bits do not depend on the run, the launch geometry or the layout the handle holds the rows in; no field is
        converted.  One field against itself about one center (both None, or equal bit for bit) is computed for j >= i only
        and mirrored: symmetric to the bit.  Each element is within (n + ceil(ncol / 512)) * 2^-53 * sum|a * b| * (1 + 2^-4)
        of the exact sum of its terms, n the members with nonzero weight.  StaleFieldError for a stale diagnostic field, as
        ``hemispheric_mean``.  The step clock, the counters and ``field_step`` are unchanged."""
        return self.ensemble_covariance_device(name_a, name_b, weights, center_a, center_b, _HOST)

    def ensemble_covariance_device(self, name_a, name_b, weights, center_a, center_b, dev_ptr: int):
        """Same reduction, the packed [nlat, nlat] result left on the device at ``dev_ptr`` (e.g. the ``data_ptr()`` of a
        torch tensor on this engine's device: the payload of an all-reduce between shards)."""
        fa, fb, w, ca, cb = self.check_covariance_args(name_a, name_b, weights, center_a, center_b)
        return self._reduced("ebm_ensemble_covariance", (self.nlat, self.nlat), dev_ptr, fa, fb, dptr(w), dptr(ca), dptr(cb))

    def _check_misfit_args(self, names, targets, rweights=None):
        """The host-side checks of ``column_misfits`` (no device call): returns (names, field ids, targets [ntargets, nvars,
        nlat], rweights [nvars, nlat] or None) with contiguous float64 arrays.  The field rules are those of
        ``_check_sums_args``; a single target may be given as [nvars, nlat]."""
        names, ids = self._fields(names, most=12, repeats=False)
        y = np.ascontiguousarray(targets, dtype=np.float64)
        if y.ndim == 2:
            y = y[None]
        if y.ndim != 3 or y.shape[1:] != (len(names), self.nlat) or not 1 <= y.shape[0] <= 8:
            raise ValueError(f"targets: expected [ntargets, {len(names)}, {self.nlat}] with 1 <= ntargets <= 8 "
                             f"(or one target as [{len(names)}, {self.nlat}]), got {y.shape}")
        if np.isinf(y).any():
            t, v, k = (int(i[0]) for i in np.nonzero(np.isinf(y)))
            raise ValueError(f"targets[{t}][{v}][{k}] = {y[t, v, k]}: expected finite values, or NaN for no observation")
        r = None if rweights is None else as_f64(rweights, (len(names), self.nlat))
        if r is not None and not (np.isfinite(r) & (r >= 0.0)).all():
            v, k = (int(i[0]) for i in np.nonzero(~(np.isfinite(r) & (r >= 0.0))))
            raise ValueError(f"rweights[{v}][{k}] = {r[v, k]}: expected finite values >= 0")
        return names, ids, np.ascontiguousarray(y), r

    def column_misfits(self, names, targets, rweights=None) -> np.ndarray:
        """ebm_column_misfits (the definition is in include/ebm_hip.h): ndarray [ntargets, 2, ncol] — for every target t and
        column c, ``[t, 0, c]`` = J = sum over the fields in ``names`` and over latitude of (r * d) * d with d = x - target,
        and ``[t, 1, c]`` = N, the number of cells that entered it, reduced along each column on the device.  ``targets``
        [ntargets, len(names), nlat] (one target: [len(names), nlat]; 1 <= ntargets <= 8), finite or NaN = "no observation
        here"; ``rweights`` [len(names), nlat], finite and >= 0 (quadrature weight / sigma^2, or a 0 / 1 band mask), None:
        all 1.0.  A cell contributes iff its rweight is not 0 and neither the target nor the cell is NaN (the sentinels of
        Ti and Tw); +-Inf in a contributing cell propagates.  The adds run in a fixed order — 128 chains by cell index mod
        128, then a fixed tree — so the bits do not depend on the run, the launch geometry or the layout the handle holds the
        rows in; no field is converted.  StaleFieldError for a stale diagnostic field, as ``hemispheric_mean``.  The step
        clock, the counters and ``field_step`` are unchanged."""
        return self.column_misfits_device(names, targets, _HOST, rweights)

    def column_misfits_device(self, names, targets, dev_ptr: int, rweights=None):
        """Same reduction, the packed [ntargets, 2, ncol] result left on the device at ``dev_ptr`` (e.g. the ``data_ptr()`` of
        a torch tensor on this engine's device: the payload of an all-gather between shards)."""
        names, ids, y, r = self._check_misfit_args(names, targets, rweights)
        return self._reduced("ebm_column_misfits", (y.shape[0], 2, self.ncol), dev_ptr, len(ids), field_ids(ids), int(y.shape[0]),
                             dptr(y), dptr(r))

    def _device_index(self) -> int:
        return int(getattr(self, "device", 0))

    def _on_my_gpu(self, tensor) -> bool:
        """Is the torch tensor on the GPU this engine was created on (the device index counts, not only the device type)?"""
        return bool(tensor.is_cuda) and tensor.device.index == self._device_index()

    def check_update_args(self, names, obs_name, gain, target, scale=1.0, perturb=None, bounds=None):
        """The host-side checks of ``update_columns`` (no device call; the rules of ebm_update_columns in include/ebm_hip.h):
        returns (names, field ids, field id of ``obs_name``, gain, target [nlat], scale, perturb, lo [nvars], hi [nvars]).
        ``gain`` comes back as a contiguous float64 ndarray [nvars, nlat, nlat] or, given a torch tensor on a GPU, as that
        tensor (checked for shape, dtype and contiguity; its entries are not looked at); ``perturb`` as the torch tensor or
        None.  The fields are looked at first, then the gain, the target, the scale, the perturbation and the bounds."""
        names = as_names(names)
        if not 1 <= len(names) <= 5:
            raise ValueError(f"names: expected between 1 and 5 prognostic fields of the {self.model} model")
        for n in names:
            if not isinstance(n, str) or n not in self.prognostic:
                raise ValueError(f"names: {n!r} is not a prognostic field of the {self.model} model (expected some of "
                                 f"{', '.join(self.prognostic)})")
        _refuse_repeats(names)
        if not isinstance(obs_name, str):
            raise ValueError(f"obs_name: expected one field name, got {obs_name!r}")
        obs_id = self._fields((obs_name,), arg="obs_name")[1][0]
        shape = (len(names), self.nlat, self.nlat)
        if hasattr(gain, "data_ptr"):                    # a torch tensor: the _device call
            if not self._on_my_gpu(gain) or str(gain.dtype) != "torch.float64" or not gain.is_contiguous():
                raise ValueError(f"gain: a tensor must be a contiguous float64 tensor on the engine's GPU (cuda:{self._device_index()})")
            if tuple(gain.shape) not in (shape, shape[1:] if len(names) == 1 else shape):
                raise ValueError(f"gain: expected shape {shape}, got {tuple(gain.shape)}")
        else:
            gain = np.ascontiguousarray(gain, dtype=np.float64)
            if len(names) == 1 and gain.shape == shape[1:]:
                gain = gain[None]
            if gain.shape != shape:
                raise ValueError(f"gain: expected shape {shape}, got {gain.shape}")
            if not np.isfinite(gain).all():
                v, k, j = (int(i[0]) for i in np.nonzero(~np.isfinite(gain)))
                raise ValueError(f"gain[{v}][{k}][{j}] = {gain[v, k, j]} is not finite (field {names[v]}, k = {k}, j = {j})")
        y = as_f64(target, (self.nlat,))
        if np.isinf(y).any():
            j = int(np.flatnonzero(np.isinf(y))[0])
            raise ValueError(f"target[{j}] = {y[j]}: expected finite values, or NaN for no observation")
        if not np.isfinite(float(scale)):
            raise ValueError(f"scale = {scale!r} is not finite")
        if perturb is not None:
            if not hasattr(perturb, "data_ptr") or not self._on_my_gpu(perturb) or str(perturb.dtype) != "torch.float64" \
                    or not perturb.is_contiguous() or tuple(perturb.shape) != (self.ncol, self.nlat):
                raise ValueError(f"perturb: expected a contiguous float64 tensor [{self.ncol}, {self.nlat}] on the engine's GPU "
                                 f"(cuda:{self._device_index()})")
        lo, hi = np.full(len(names), -np.inf), np.full(len(names), np.inf)
        for n, b in (bounds or {}).items():
            if n not in names:
                raise ValueError(f"bounds: {n!r} is not one of the updated fields")
            l, h = (-np.inf if b[0] is None else float(b[0])), (np.inf if b[1] is None else float(b[1]))
            if np.isnan(l) or np.isnan(h) or l > h:
                raise ValueError(f"bounds[{n!r}] = {b!r}: expected (lo, hi) with lo <= hi, None or +-Inf for no bound")
            lo[names.index(n)], hi[names.index(n)] = l, h
        return names, [FIELD[n] for n in names], obs_id, gain, y, float(scale), perturb, lo, hi

    def update_columns(self, names, obs_name, gain, target, scale=1.0, perturb=None, bounds=None):
        """ebm_update_columns (the definition is in include/ebm_hip.h): every member moved by a linear map of its own
        innovation, on the device — for each field f of ``names`` (prognostic ones), ``x_f[c, k] += sum_j gain[f, k, j] *
        d[c, j]`` with ``d[c, j] = (target[j] + perturb[c, j]) - scale * xo[c, j]``, xo the cell of ``obs_name`` (any solution
        variable; it may be one of ``names``: the innovations are formed from the state at entry).  d is +0.0 where ``target``
        is NaN ("no observation here") or xo is NaN.  ``gain`` [len(names), nlat, nlat]: an ndarray, or a contiguous float64
        torch tensor on the engine's GPU, which is taken where it lies (ebm_update_columns_device); ``perturb``: None or a
        float64 torch tensor [ncol, nlat] on the engine's GPU; ``bounds``: dict name -> (lo, hi), applied to the new value
        with strict comparisons (NaN passes; None or +-Inf: no bound).  The sum runs on the fp64 matrix instruction in a
        fixed order — four observation cells per instruction, ascending — so the bits do not depend on the run, the launch
        geometry or the layout the handle holds the rows in; no field is converted; ``x + acc`` is one rounded add.
        Afterwards the handle is as after ``set_field`` of every listed field: the diagnostic fields and T0 are stale, the
        step clock, the counters and the noise state are unchanged.  StaleFieldError for a stale ``obs_name``."""
        names, ids, obs_id, g, y, scale, e, lo, hi = self.check_update_args(names, obs_name, gain, target, scale, perturb, bounds)
        eptr = None if e is None else C.c_void_p(e.data_ptr())
        if isinstance(g, np.ndarray):
            check(self.lib.ebm_update_columns(self._h, len(ids), field_ids(ids), obs_id, dptr(g), dptr(y), scale, eptr, dptr(lo), dptr(hi)),
                  "ebm_update_columns")
        else:
            check(self.lib.ebm_update_columns_device(self._h, len(ids), field_ids(ids), obs_id, C.c_void_p(g.data_ptr()), dptr(y), scale,
                                                     eptr, dptr(lo), dptr(hi)), "ebm_update_columns_device")

    def _check_gpu_matrix(self, t, arg, shape=None):
        """A contiguous float64 torch tensor on the engine's GPU (of ``shape``, if given), as ``check_update_args`` asks of a
        device gain."""
        if not hasattr(t, "data_ptr") or not self._on_my_gpu(t) or str(t.dtype) != "torch.float64" or not t.is_contiguous():
            raise ValueError(f"{arg}: expected a contiguous float64 tensor on the engine's GPU (cuda:{self._device_index()})")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{arg}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    @staticmethod
    def _raise_with_info(rc, info, what):
        try:
            check(rc, what)
        except _lib.EBMError as err:
            err.info = int(info.value)
            raise

    def spd_solve(self, S, B, m=None):
        """ebm_spd_solve_device (the definition is in include/ebm_hip.h): X . S = B for a symmetric positive definite ``S``, in
        place, by a blocked Cholesky factorisation on the fp64 matrix instruction.  ``S`` [rows, lds] and ``B`` [nrhs, ldb]:
        contiguous float64 torch tensors on the engine's GPU; the system is the leading ``m`` x ``m`` of S (None: all of its
        rows) and rows, lds and ldb must be >= m rounded up to 64, S padded with the identity and B with zeros by the caller.
        On return the lower triangle of S holds L and the rows of B hold X.  EBMError (``.info`` = the 1-based index of the
        first bad pivot) where S is not positive definite.  The handle's fields, clock and counters are untouched.  torch's
        current stream is awaited first (here and in ``kalman_gain_tensor``): the handle's own stream does not wait for it."""
        S, B = self._check_gpu_matrix(S, "S"), self._check_gpu_matrix(B, "B")
        if S.dim() != 2 or B.dim() != 2:
            raise ValueError(f"S, B: expected two matrices, got shapes {tuple(S.shape)} and {tuple(B.shape)}")
        m = int(S.shape[0]) if m is None else int(m)
        mp = (m + 63) // 64 * 64
        if m < 1 or min(S.shape[0], S.shape[1], B.shape[1]) < mp:
            raise ValueError(f"S {tuple(S.shape)}, B {tuple(B.shape)}: expected m >= 1 and the rows and the row length of S and the "
                             f"row length of B >= m rounded up to 64 = {mp} (pad S with the identity and B with zeros)")
        import torch
        torch.cuda.current_stream(self._device_index()).synchronize()      # the handle's stream does not wait for torch's
        info = C.c_int(0)
        rc = self.lib.ebm_spd_solve_device(self._h, m, int(B.shape[0]), C.c_void_p(S.data_ptr()), int(S.shape[1]),
                                           C.c_void_p(B.data_ptr()), int(B.shape[1]), C.byref(info))
        self._raise_with_info(rc, info, "ebm_spd_solve_device")

    def kalman_gain_tensor(self, obs, obs_var, localize, factor, P_oo, P_fo):
        """ebm_kalman_gain_device (the definition is in include/ebm_hip.h): the Kalman gains [len(P_fo), nlat, nlat] as a new
        torch tensor on the engine's GPU — what ``update_columns`` takes — from covariances already there.  ``obs`` [nlat]
        (NaN: not observed), ``obs_var`` scalar or [nlat], ``localize``: the half-width in x of the Gaspari-Cohn taper (None
        or <= 0: none), ``factor``: what multiplies both covariances (inflation * n / (n - 1) for sums divided by n), ``P_oo``
        and every entry of ``P_fo`` (1 to 5; an entry may be ``P_oo`` itself): contiguous float64 [nlat, nlat] tensors on the
        engine's GPU.  Assembly, factorisation, solve and scatter run on the device in a fixed order: the same bits on every
        run.  EBMError (``.info`` = the bad pivot; the message names the observed latitude) where the innovation covariance
        is not positive definite.  The handle's fields, clock and counters are untouched."""
        import torch
        nlat = self.nlat
        y = as_f64(obs, (nlat,))
        R = np.ascontiguousarray(np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (nlat,)))
        P_fo = list(P_fo)
        if not 1 <= len(P_fo) <= 5:
            raise ValueError(f"P_fo: expected between 1 and 5 matrices, got {len(P_fo)}")
        self._check_gpu_matrix(P_oo, "P_oo", (nlat, nlat))
        for v, p in enumerate(P_fo):
            self._check_gpu_matrix(p, f"P_fo[{v}]", (nlat, nlat))
        gain = torch.empty((len(P_fo), nlat, nlat), dtype=torch.float64, device=P_oo.device)
        addr = (C.c_void_p * len(P_fo))(*[p.data_ptr() for p in P_fo])
        torch.cuda.current_stream(self._device_index()).synchronize()      # the handle's stream does not wait for torch's
        info = C.c_int(0)
        rc = self.lib.ebm_kalman_gain_device(self._h, len(P_fo), dptr(y), dptr(R), 0.0 if localize is None else float(localize),
                                             float(factor), C.c_void_p(P_oo.data_ptr()), addr, C.c_void_p(gain.data_ptr()), C.byref(info))
        self._raise_with_info(rc, info, "ebm_kalman_gain_device")
        return gain

    def kalman_gain_phases(self) -> dict:
        """ebm_kalman_gain_phases: milliseconds between HIP events around the assembly, the factorisation, the two solves
        and the scatter of this engine's last ``kalman_gain_tensor`` that ran a solve."""
        ms = (C.c_float * 4)()
        check(self.lib.ebm_kalman_gain_phases(self._h, ms), "ebm_kalman_gain_phases")
        return dict(zip(("assembly", "factor", "solve", "scatter"), (float(v) for v in ms)))

    def get_field_device(self, name: str, dev_ptr: int):
        """Device-to-device copy of a field, packed [ncol][nlat], to ``dev_ptr``."""
        check(self.lib.ebm_get_field_device(self._h, FIELD[name], C.c_void_p(dev_ptr)),
              "ebm_get_field_device")

    def diffusion(self, temp, base=None) -> np.ndarray:
        """``diffusion!(base, temp, st, par)`` / ``diffusion(T, st, par)`` (reference
        src/infrastructure.jl:495-533) per column on the device: base + D d/dx[(1-x^2) d temp/dx]."""
        t = as_f64(temp).reshape(self.ncol, self.nlat)
        b = None if base is None else as_f64(base).reshape(self.ncol, self.nlat)
        out = np.empty((self.ncol, self.nlat))
        check(self.lib.ebm_diffusion(self._h, dptr(t), dptr(b), dptr(out)), "ebm_diffusion")
        return out

    def zonal_diffusion(self, temp, nlon: int):
        """The zonal partner of ``diffusion`` as a backward-Euler substep over dt (ebm_zonal_diffusion; an extension, not in
        the reference): the columns are read as members of ``nlon`` longitudes each (column = member*nlon + longitude,
        periodic); returns (U, Z) for ``temp`` [ncol, nlat] — the zonally diffused field and the heat-flux convergence
        (U - temp) cw/dt = D/((1-x^2) dlambda^2) d2U/dl2."""
        t = as_f64(temp).reshape(self.ncol, self.nlat)
        U, Z = np.empty((self.ncol, self.nlat)), np.empty((self.ncol, self.nlat))
        check(self.lib.ebm_zonal_diffusion(self._h, int(nlon), dptr(t), dptr(U), dptr(Z)), "ebm_zonal_diffusion")
        return U, Z

    def field_device_ptr(self, name: str):
        p, pitch = C.c_void_p(), C.c_longlong()
        check(self.lib.ebm_field_device_ptr(self._h, FIELD[name], C.byref(p), C.byref(pitch)),
              "ebm_field_device_ptr")
        return p.value, pitch.value

    def set_column_forcing(self, fcol):
        a = None if fcol is None else as_f64(fcol, (self.ncol,))
        check(self.lib.ebm_set_column_forcing(self._h, dptr(a)), "ebm_set_column_forcing")

    def set_column_schedules(self, forcings):
        """Per-column Forcing schedules evaluated on the device (ebm_set_column_schedule):
        ``forcings`` is a sequence of ``ncol`` Forcing objects, or None to clear."""
        a = None
        if forcings is not None:
            if len(forcings) != self.ncol:
                raise ValueError(f"expected {self.ncol} Forcing objects, got {len(forcings)}")
            a = np.array([schedule_words(f) for f in forcings], dtype=np.float64)
        check(self.lib.ebm_set_column_schedule(self._h, dptr(a)), "ebm_set_column_schedule")

    def set_column_params(self, matrix):
        """Per-column parameter rows (ebm_set_column_params): ``matrix`` [ncol, 25] in PARAM_ORDER (see
        ``param_matrix``), or None to return every column to the vector the engine was created with.  Column c then
        gives the bits of an engine created with row c; distinct rows share nothing but the launch."""
        a = None if matrix is None else as_f64(matrix)
        if a is not None and a.shape != (self.ncol, len(PARAM_ORDER)):
            raise ValueError(f"expected parameter rows of shape {(self.ncol, len(PARAM_ORDER))}, got {a.shape}")
        check(self.lib.ebm_set_column_params(self._h, dptr(a)), "ebm_set_column_params")

    def check_noise_args(self, sigma, rho=None, seed=0, streams=None, tau=None):
        """The host-side checks of ``set_column_noise`` (no device call): see ``noise.check_args``."""
        return noise.check_args(self.ncol, self.dt, sigma, rho, seed, streams, tau)

    def set_column_noise(self, sigma, rho=None, seed=0, streams=None, tau=None):
        """Per-column AR(1) forcing noise drawn on the device (ebm_set_column_noise; the definition is in
        include/ebm_hip.h): ``sigma`` the stationary standard deviation (W m^-2; scalar or [ncol]), ``rho`` the lag-one-step
        autocorrelation in [0, 1) (default 0: white) or ``tau`` its e-folding time in years (rho = exp(-dt/tau)), ``seed``
        the handle's seed and ``streams`` the [ncol] stream ids (default 0 .. ncol-1; a shard passes its members' global
        indices).  Resets the noise state to 0.  ``sigma=None`` clears the noise."""
        sig, r, st, seed = (None, None, None, 0) if sigma is None else self.check_noise_args(sigma, rho, seed, streams, tau)
        sp = None if st is None else st.ctypes.data_as(C.POINTER(C.c_ulonglong))
        check(self.lib.ebm_set_column_noise(self._h, dptr(sig), dptr(r), sp, C.c_ulonglong(seed)), "ebm_set_column_noise")

    def noise_state(self) -> np.ndarray:
        """N_c [ncol], the noise added to each column's forcing at the last step (0 without noise)."""
        out = np.empty(self.ncol)
        check(self.lib.ebm_get_noise_state(self._h, dptr(out)), "ebm_get_noise_state")
        return out

    def set_noise_state(self, N):
        """Restore N_c [ncol] (checkpoint / restart; needs noise installed)."""
        a = as_f64(N, (self.ncol,))
        if not np.all(np.isfinite(a)):
            raise ValueError("noise state: expected finite values")
        check(self.lib.ebm_set_noise_state(self._h, dptr(a)), "ebm_set_noise_state")

    def noise_innovations(self, first_step: int, nsteps: int) -> np.ndarray:
        """xi [ncol, nsteps] of global steps first_step .. first_step + nsteps - 1, computed on the device by the function
        the step kernels use (ebm_noise_innovations)."""
        if int(first_step) < 0 or int(nsteps) < 0:
            raise ValueError("noise_innovations: first_step and nsteps must be >= 0")
        out = np.empty((self.ncol, int(nsteps)))
        check(self.lib.ebm_noise_innovations(self._h, int(first_step), int(nsteps), dptr(out)), "ebm_noise_innovations")
        return out

    def set_step_clock(self, step: int):
        check(self.lib.ebm_set_step_clock(self._h, int(step)), "ebm_set_step_clock")

    def set_time_table(self, t_in_year):
        """t_in_year = st.t; uploads cos(2.0*pi*t_i)."""
        tab = np.array([cos2pit(float(t)) for t in t_in_year], dtype=np.float64)
        self.nt = len(tab)
        self.ttab = tab
        check(self.lib.ebm_set_time_table(self._h, self.nt, dptr(tab)), "ebm_set_time_table")

    # -- stepping ---------------------------------------------------------------------
    def step(self, ct: float, ct_next: float, f: float, write_diag: bool = True):
        check(self.lib.ebm_step(self._h, ct, ct_next, f, int(write_diag)), "ebm_step")

    def run(self, first_step: int, nsteps: int, f_steps=None, diag_last: bool = True,
            steps_per_launch: int = 1):
        """``nsteps`` steps from global step ``first_step``.  ``steps_per_launch`` = K > 1 fuses K
        consecutive steps into one launch (ebm_run_fused; bit-identical results, no per-step
        output in between)."""
        a = None if f_steps is None else as_f64(f_steps, (nsteps,))
        if steps_per_launch > 1:
            check(self.lib.ebm_run_fused(self._h, int(first_step), int(nsteps), dptr(a), int(diag_last),
                                         int(steps_per_launch)), "ebm_run_fused")
        else:
            check(self.lib.ebm_run(self._h, int(first_step), int(nsteps), dptr(a), int(diag_last)),
                  "ebm_run")

    @staticmethod
    def _check_sampling(who, first_step, nsteps, every, f_steps, steps_per_launch):
        """The step arguments of ``run_series`` and ``run_series_scalars`` (no device call): returns f_steps."""
        if int(first_step) < 0 or int(nsteps) < 0:
            raise ValueError(f"{who}: first_step and nsteps must be >= 0")
        if int(every) < 1:
            raise ValueError(f"every = {every}: a sample is taken every `every` >= 1 steps")
        if int(nsteps) % int(every):
            raise ValueError(f"nsteps = {nsteps} is not a multiple of every = {every}")
        if int(steps_per_launch) < 1:
            raise ValueError(f"steps_per_launch = {steps_per_launch}: need at least one step per launch")
        return None if f_steps is None else as_f64(f_steps, (int(nsteps),))

    def check_series_args(self, first_step, nsteps, every, names, f_steps=None, steps_per_launch=64):
        """The host-side checks of ``run_series`` (no device call): returns (names, field ids, f_steps)."""
        names, ids = self._fields(names, most=len(self.prognostic + self.diagnostic), repeats=False)
        return names, ids, self._check_sampling("run_series", first_step, nsteps, every, f_steps, steps_per_launch)

    def run_series(self, first_step, nsteps, every, names, f_steps=None, steps_per_launch=64):
        """ebm_run_series: ``nsteps`` steps from global step ``first_step`` exactly as ``run`` takes them (``diag_last`` iff
        one of ``names`` is a diagnostic field), with the per-column hemispheric mean (reference src/utilities.jl:397-403)
        of every field in ``names`` sampled on the device after every ``every`` steps — ndarray [len(names),
        nsteps // every, ncol]; sample j is the state after step first_step + (j+1)*every - 1, bit for bit what
        ``hemispheric_mean`` returns there.  One download at the end; nothing is synchronised between samples."""
        names, ids, f = self.check_series_args(first_step, nsteps, every, names, f_steps, steps_per_launch)
        nv, ns = len(names), int(nsteps) // int(every)
        out = np.full((nv, ns, self.ncol), np.nan)
        check(self.lib.ebm_run_series(self._h, int(first_step), int(nsteps), dptr(f), int(every), int(steps_per_launch), nv,
                                      field_ids(ids), dptr(out)), "ebm_run_series")
        return out

    def integrate(self, nt, dur, f_steps, lastonly, winter_inx, summer_inx, names,
                  want_raw=True, want_seasonal=True, want_avg=True, out=None):
        """ebm_integrate: returns dict(raw, winter, summer, avg), each [nvars, n, ncol, nlat].
        Outputs that are not wanted are None; with neither raw nor avg the diagnostic fields are
        only written on the steps whose snapshot is taken.  ``out``: a dict returned by an earlier call of the
        same shape, whose arrays are filled again instead of allocating new ones (a caller that integrates year
        after year into the same buffers)."""
        nv = len(names)
        fields = field_ids([FIELD[n] for n in names])
        nraw = nt if lastonly else nt * dur
        f = None if f_steps is None else as_f64(f_steps, (nt * dur,))
        shape = (nv, dur, self.ncol, self.nlat)

        def reuse(key, wanted, shp):
            a = None if out is None else out.get(key)
            if not wanted:
                return None
            if a is not None and (a.shape != shp or a.dtype != np.float64 or not a.flags.c_contiguous):
                raise ValueError(f"out[{key!r}] must be a C-contiguous float64 array of shape {shp}")
            return a
        raw = reuse("raw", want_raw, (nv, nraw, self.ncol, self.nlat))
        if want_raw and raw is None:
            raw = np.empty((nv, nraw, self.ncol, self.nlat))
        def mk(key, wanted):
            a = reuse(key, wanted, shape)
            return a if (a is not None or not wanted) else np.full(shape, np.nan)
        winter, summer, avg = mk("winter", want_seasonal), mk("summer", want_seasonal), mk("avg", want_avg)
        check(self.lib.ebm_integrate(self._h, nt, dur, dptr(f), int(lastonly), int(winter_inx),
                                     int(summer_inx), nv, fields, dptr(raw), dptr(winter),
                                     dptr(summer), dptr(avg)), "ebm_integrate")
        return dict(raw=raw, winter=winter, summer=summer, avg=avg)

    def integrate_hemispheric(self, nt, dur, f_steps, winter_inx, summer_inx, names):
        """ebm_integrate_hemispheric: per variable, year and column the hemispheric mean (reference
        src/utilities.jl:397-403) of the winter snapshot, the summer snapshot and the annual mean, reduced
        on the device — dict(winter, summer, avg), each [nvars, dur, ncol].  The data of the reference's
        hysteresis plot (src/plot.jl:173-225) for every column, without the fields crossing the bus."""
        nv = len(names)
        fields = field_ids([FIELD[n] for n in names])
        f = None if f_steps is None else as_f64(f_steps, (nt * dur,))
        out = {k: np.full((nv, dur, self.ncol), np.nan) for k in ("winter", "summer", "avg")}
        check(self.lib.ebm_integrate_hemispheric(self._h, nt, dur, dptr(f), int(winter_inx), int(summer_inx), nv, fields,
                                                 dptr(out["winter"]), dptr(out["summer"]), dptr(out["avg"])),
              "ebm_integrate_hemispheric")
        return out

    def check_equilibrate_args(self, nt, max_years, tol, min_years=2, f_year=None):
        """The host-side checks of ``equilibrate`` (no device call): returns (names, field ids, tolerances, f_year)."""
        if not hasattr(tol, "items") or len(tol) < 1:
            raise ValueError("tol: expected a dict of field name -> absolute tolerance, e.g. {'T': 1e-3}")
        names, ids = self._fields(tuple(tol), "tol", t0_note=False)
        tols = np.array([float(tol[n]) for n in names], dtype=np.float64)
        for n, t in zip(names, tols):
            if not t >= 0.0:
                raise ValueError(f"tol[{n!r}] = {t}: a tolerance must be >= 0 (and not NaN)")
        if int(max_years) < 1:
            raise ValueError(f"max_years = {max_years}: need at least one year")
        if int(nt) < 1:
            raise ValueError(f"nt = {nt}: need at least one step per year")
        f = None if f_year is None else as_f64(f_year, (int(nt),))
        return names, ids, tols, f

    def equilibrate(self, nt, max_years, f_year=None, tol=None, min_years=2):
        """ebm_equilibrate: whole years of ``nt`` steps (forcing ``f_year[i] + fcol[c]``, the same every year) until each
        column's year-end fields repeat — ``max |S(y) - S(y-1)| <= tol[name]`` for every named field, first tested after
        year max(2, min_years) — or ``max_years``.  A column stops at its own equilibrium year, its state bit for bit that
        of plain stepping for that many years.  ``tol``: dict field name -> absolute tolerance (default ``{"T": 1e-3}``).
        Returns dict(years [ncol] int, converged [ncol] bool, resid {name: [ncol]}: the last distance compared, NaN if
        none)."""
        tol = {"T": 1e-3} if tol is None else tol
        names, ids, tols, f = self.check_equilibrate_args(nt, max_years, tol, min_years, f_year)
        nv = len(names)
        years = np.zeros(self.ncol, dtype=np.int32)
        conv = np.zeros(self.ncol, dtype=np.int32)
        resid = np.full((nv, self.ncol), np.nan)
        check(self.lib.ebm_equilibrate(self._h, int(nt), int(max_years), int(min_years), dptr(f), nv, field_ids(ids), dptr(tols),
                                       iptr(years), iptr(conv), dptr(resid)), "ebm_equilibrate")
        return dict(years=years.astype(np.int64), converged=conv.astype(bool), resid={n: resid[i] for i, n in enumerate(names)})

    def _check_passage(self, who, what, first_step, max_samples, every, level, direction, f_steps, steps_per_launch):
        """The arguments of ``run_until`` and ``run_until_scalar`` but the tested quantity `what` (no device call): returns
        (level [ncol] float64, direction [ncol] int32, f_steps)."""
        if int(first_step) < 0:
            raise ValueError(f"{who}: first_step must be >= 0")
        if int(max_samples) < 1:
            raise ValueError(f"max_samples = {max_samples}: need at least one round")
        if int(every) < 1:
            raise ValueError(f"every = {every}: the {what} is tested every `every` >= 1 steps")
        if int(steps_per_launch) < 1:
            raise ValueError(f"steps_per_launch = {steps_per_launch}: need at least one step per launch")
        lev = as_f64(level, (self.ncol,))
        if np.isnan(lev).any():
            raise ValueError("level: NaN (+-inf is legal: never, or at the first sample)")
        d = np.asarray(direction)
        if d.shape != (self.ncol,) or d.dtype.kind not in "iu":
            raise ValueError(f"direction: expected {self.ncol} integers, > 0 upward and < 0 downward")
        if (d == 0).any():
            raise ValueError("direction: 0 is neither upward (> 0) nor downward (< 0)")
        d = np.ascontiguousarray(np.sign(d), dtype=np.int32)
        f = None if f_steps is None else as_f64(f_steps, (int(max_samples) * int(every),))
        return lev, d, f

    def check_until_args(self, first_step, max_samples, every, name, level, direction, f_steps=None, steps_per_launch=64):
        """The host-side checks of ``run_until`` (no device call): returns (field id, level [ncol] float64, direction [ncol]
        int32, f_steps)."""
        _, (fid,) = self._fields((name,), "name")
        return (fid, *self._check_passage("run_until", "mean", first_step, max_samples, every, level, direction, f_steps, steps_per_launch))

    def run_until(self, first_step, max_samples, every, name, level, direction, f_steps=None, steps_per_launch=64):
        """ebm_run_until: rounds of ``every`` steps from global step ``first_step``, at most ``max_samples`` of them; after
        each the per-column hemispheric mean of field ``name`` is taken on the device and a column whose mean has crossed
        its ``level`` (``direction`` > 0: mean >= level, < 0: mean <= level; NaN never crosses) takes no further step, its
        state bit for bit that of ``run`` over its own number of steps.  Returns dict(samples [ncol] int: rounds taken,
        crossed [ncol] bool, value [ncol]: the last mean, steps: the steps the slowest column took).  One stream
        synchronisation per round."""
        fid, lev, d, f = self.check_until_args(first_step, max_samples, every, name, level, direction, f_steps, steps_per_launch)
        samples = np.zeros(self.ncol, dtype=np.int32)
        crossed = np.zeros(self.ncol, dtype=np.int32)
        value = np.full(self.ncol, np.nan)
        check(self.lib.ebm_run_until(self._h, int(first_step), int(max_samples), int(every), dptr(f), int(steps_per_launch), fid,
                                     dptr(lev), iptr(d), iptr(samples), iptr(crossed), dptr(value)), "ebm_run_until")
        samples = samples.astype(np.int64)
        return dict(samples=samples, crossed=crossed.astype(bool), value=value, steps=int(samples.max()) * int(every))

    # -- column scalars -----------------------------------------------------------------
    def check_scalar_args(self, specs):
        """The host-side checks of the column-scalar calls (no device call; the rules of ebm_column_scalars in
        include/ebm_hip.h).  ``specs``: between 1 and 12 scalars, each ``(kind, name, k0, k1)`` or ``(kind, name, k0, k1,
        level)`` — kind one of "integral", "mean", "edge_ge", "edge_le"; name a solution variable of the model; 0 <= k0 <= k1
        <= nlat - 1 the band's first and last cell, both inclusive, k0 < k1 for the integral kinds; level not NaN for the
        edge kinds (ignored, and 0.0 if absent, otherwise).  The message names the first offending scalar.  Returns (spec
        int32 [n, 4] = kind, field id, k0, k1; level float64 [n])."""
        specs = list(specs) if isinstance(specs, (list, tuple)) else None
        if specs is not None and len(specs) in (4, 5) and isinstance(specs[0], str):
            raise ValueError("specs: expected a sequence of scalars, got one (wrap it in a list)")
        if specs is None or not 1 <= len(specs) <= 12:
            raise ValueError("specs: expected between 1 and 12 column scalars (kind, name, k0, k1[, level])")
        allowed = self.prognostic + self.diagnostic
        spec, level = np.zeros((len(specs), 4), dtype=np.int32), np.zeros(len(specs))
        for s, one in enumerate(specs):
            if not isinstance(one, (list, tuple)) or len(one) not in (4, 5):
                raise ValueError(f"scalar {s}: expected (kind, name, k0, k1[, level]), got {one!r}")
            kind, name, k0, k1 = one[:4]
            lev = 0.0 if len(one) == 4 or one[4] is None else float(one[4])
            if not isinstance(kind, str) or kind not in _lib.SCALAR_KIND:
                raise ValueError(f"scalar {s}: unknown kind {kind!r} (expected one of {', '.join(_lib.SCALAR_KIND)})")
            if not isinstance(name, str) or name not in allowed:
                raise ValueError(f"scalar {s}: unknown field {name!r} for the {self.model} model (expected one of "
                                 f"{', '.join(allowed)}; the warm start T0 is not a solution variable)")
            for k in (k0, k1):
                if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
                    raise ValueError(f"scalar {s}: the band k0 = {k0!r}, k1 = {k1!r} is not a pair of cell indices (int)")
            if not 0 <= k0 <= k1 <= self.nlat - 1:
                raise ValueError(f"scalar {s}: the band k0 = {k0}, k1 = {k1} is not 0 <= k0 <= k1 <= {self.nlat - 1}")
            edge = kind.startswith("edge")
            if not edge and k0 == k1:
                raise ValueError(f"scalar {s}: an integral over one cell (k0 == k1 = {k0})")
            if edge and (len(one) == 4 or one[4] is None or np.isnan(lev)):
                raise ValueError(f"scalar {s}: an edge needs a level that is not NaN")
            spec[s] = (_lib.SCALAR_KIND[kind], FIELD[name], int(k0), int(k1))
            level[s] = lev
        return spec, level

    def column_scalars(self, specs) -> np.ndarray:
        """ebm_column_scalars (the definition is in include/ebm_hip.h): ndarray [len(specs), ncol] of per-column scalars
        reduced ALONG each column on the device — "integral" / "mean" of a field over the cells k0 .. k1 (the trapezoid sum
        of ``hemispheric_mean``, in its order: the full range gives its bits; the mean divides by x[k1] - x[k0]), and
        "edge_ge" / "edge_le": the position x, linearly interpolated between the two cells, where walking poleward from k0
        the field first is >= (<=) the level; +Inf if it never is.  ``specs`` as ``check_scalar_args`` takes them
        (``ensemble.scalar_spec`` builds one from a band in the grid's coordinate).  Fields are made readable as
        ``hemispheric_mean`` does; StaleFieldError for a stale diagnostic field.  The step clock, the counters and
        ``field_step`` are unchanged."""
        return self.column_scalars_device(specs, _HOST)

    def column_scalars_device(self, specs, dev_ptr: int):
        """Same reduction, the packed [len(specs), ncol] result left on the device at ``dev_ptr``."""
        spec, level = self.check_scalar_args(specs)
        return self._reduced("ebm_column_scalars", (len(spec), self.ncol), dev_ptr, len(spec), iptr(spec), dptr(level))

    def run_series_scalars(self, first_step, nsteps, every, specs, f_steps=None, steps_per_launch=64):
        """ebm_run_series_scalars: ``run_series`` with the column scalars ``specs`` for a sample — ndarray [len(specs),
        nsteps // every, ncol]; sample j is bit for bit what ``column_scalars`` returns after step first_step +
        (j+1)*every - 1.  Stepping, the diagnostics rule and the one download at the end are ``run_series``'s."""
        spec, level = self.check_scalar_args(specs)
        f = self._check_sampling("run_series_scalars", first_step, nsteps, every, f_steps, steps_per_launch)
        out = np.full((len(spec), int(nsteps) // int(every), self.ncol), np.nan)
        check(self.lib.ebm_run_series_scalars(self._h, int(first_step), int(nsteps), dptr(f), int(every), int(steps_per_launch),
                                              len(spec), iptr(spec), dptr(level), dptr(out)), "ebm_run_series_scalars")
        return out

    def check_until_scalar_args(self, first_step, max_samples, every, spec, level, direction, f_steps=None, steps_per_launch=64):
        """The host-side checks of ``run_until_scalar`` (no device call): returns (spec int32 [4], the scalar's own level,
        level [ncol] float64, direction [ncol] int32, f_steps)."""
        sp, sl = self.check_scalar_args([spec])
        return (sp[0], float(sl[0]), *self._check_passage("run_until_scalar", "scalar", first_step, max_samples, every, level,
                                                          direction, f_steps, steps_per_launch))

    def run_until_scalar(self, first_step, max_samples, every, spec, level, direction, f_steps=None, steps_per_launch=64):
        """ebm_run_until_scalar: ``run_until`` with the column scalar ``spec`` (one entry of ``check_scalar_args``) in place
        of the hemispheric mean — a member stops when its ice edge has passed ``level``, or its band mean has.  A NaN scalar
        never crosses; the +Inf of a band without an edge crosses an upward test.  Returns ``run_until``'s dict."""
        sp, sl, lev, d, f = self.check_until_scalar_args(first_step, max_samples, every, spec, level, direction, f_steps, steps_per_launch)
        samples = np.zeros(self.ncol, dtype=np.int32)
        crossed = np.zeros(self.ncol, dtype=np.int32)
        value = np.full(self.ncol, np.nan)
        check(self.lib.ebm_run_until_scalar(self._h, int(first_step), int(max_samples), int(every), dptr(f), int(steps_per_launch),
                                            iptr(sp), sl, dptr(lev), iptr(d), iptr(samples), iptr(crossed), dptr(value)),
              "ebm_run_until_scalar")
        samples = samples.astype(np.int64)
        return dict(samples=samples, crossed=crossed.astype(bool), value=value, steps=int(samples.max()) * int(every))

    def check_resample_args(self, parents):
        """The host-side checks of ``resample_columns`` (no device call): returns the parents as a contiguous int32 array
        [ncol]."""
        p = np.asarray(parents)
        if p.dtype.kind not in "iu":          # (a bool array is kind "b": a mask is not a list of parents)
            raise ValueError(f"parents: expected {self.ncol} integers (column indices), got dtype {p.dtype}")
        if p.shape != (self.ncol,):
            raise ValueError(f"parents: expected {self.ncol} integers, one per column, got shape {p.shape}")
        bad = np.flatnonzero((p < 0) | (p >= self.ncol))
        if bad.size:
            c = int(bad[0])
            raise ValueError(f"parents[{c}] = {int(p[c])} is outside [0, {self.ncol})")
        return np.ascontiguousarray(p, dtype=np.int32)

    def resample_columns(self, parents):
        """ebm_resample_columns: for every column c at once, the new state of c is the old state of ``parents[c]`` — the
        prognostic fields, the warm start, the noise state and every field that is current — gathered on the device in
        whatever layout the handle holds.  Column c keeps its own forcing offset, schedule, parameter row and noise stream,
        so a clone parts from its parent at the next step.  The step clock, the counters and the validity of the fields
        are unchanged; ``parents[c] == c`` moves nothing.  Asynchronous."""
        p = self.check_resample_args(parents)
        check(self.lib.ebm_resample_columns(self._h, iptr(p)), "ebm_resample_columns")

    def column_record(self):
        """ebm_column_record: ``(record_doubles, mask)`` — the doubles of one exported column (a function of the model, nlat
        and cells_per_thread only) and the mask an export would return now (bit f: field f is current)."""
        n, m = C.c_longlong(), C.c_uint()
        check(self.lib.ebm_column_record(self._h, C.byref(n), C.byref(m)), "ebm_column_record")
        return int(n.value), int(m.value)

    def check_exchange_args(self, cols, ptr, records=None, mask=None, distinct=False):
        """The host-side checks of ``export_columns`` / ``import_columns`` (no device call): returns the columns, and the
        record indices if given, as contiguous int32 arrays."""
        c = np.asarray(cols)
        if c.size == 0:
            c = c.astype(np.int32)
        if c.dtype.kind not in "iu" or c.ndim != 1:
            raise ValueError(f"cols: expected a vector of integers (column indices), got dtype {c.dtype}, shape {c.shape}")
        bad = np.flatnonzero((c < 0) | (c >= self.ncol))
        if bad.size:
            i = int(bad[0])
            raise ValueError(f"cols[{i}] = {int(c[i])} is outside [0, {self.ncol})")
        if distinct and np.unique(c).size != c.size:
            raise ValueError("cols: a destination column is named twice")
        if not isinstance(ptr, (int, np.integer)) or isinstance(ptr, (bool, np.bool_)):
            raise ValueError(f"ptr: expected a device address (int), got {type(ptr).__name__}")
        if c.size and (int(ptr) == 0 or int(ptr) % 16):
            raise ValueError(f"ptr = {int(ptr):#x}: expected a 16-byte aligned device address")
        r = None
        if records is not None:
            r = np.asarray(records)
            if r.size == 0:
                r = r.astype(np.int32)
            if r.dtype.kind not in "iu" or r.shape != c.shape:
                raise ValueError(f"records: expected {c.size} integers, one per column, got dtype {r.dtype}, shape {r.shape}")
            bad = np.flatnonzero(r < 0)
            if bad.size:
                raise ValueError(f"records[{int(bad[0])}] = {int(r[bad[0]])} is negative")
            r = np.ascontiguousarray(r, dtype=np.int32)
        if mask is not None and (isinstance(mask, (bool, np.bool_)) or not isinstance(mask, (int, np.integer))
                                 or not 0 <= int(mask) < 1 << len(FIELD)):
            raise ValueError(f"mask = {mask!r}: expected the integer an export returned (bit f: field f travels)")
        return np.ascontiguousarray(c, dtype=np.int32), r

    def export_columns(self, cols, ptr):
        """ebm_export_columns: the state of column ``cols[i]`` into record i of the device buffer at address ``ptr``
        (``len(cols) * column_record()[0]`` doubles, 16-byte aligned) — every field in the natural layout, the warm start,
        N_c.  Returns the mask (bit f: the slot of field f was written).  Changes nothing in the handle.  Asynchronous."""
        c, _ = self.check_exchange_args(cols, ptr)
        m = C.c_uint()
        check(self.lib.ebm_export_columns(self._h, len(c), iptr(c), C.c_void_p(int(ptr)), C.byref(m)), "ebm_export_columns")
        return int(m.value)

    def import_columns(self, cols, ptr, mask, records=None):
        """ebm_import_columns: column ``cols[i]`` (distinct) takes record ``records[i]`` (default i) of the device buffer
        at ``ptr``, in the layout this handle holds; it keeps its own forcing offset, schedule, parameter row and noise
        stream.  ``mask`` is the exporter's.  StaleFieldError if a field that is current here is absent from it.  The
        buffer must be complete before the call and untouched until ``sync``.  Asynchronous."""
        if mask is None:
            raise ValueError("mask: expected the integer the export returned")
        c, r = self.check_exchange_args(cols, ptr, records, mask, distinct=True)
        check(self.lib.ebm_import_columns(self._h, len(c), iptr(c), iptr(r), C.c_void_p(int(ptr)), int(mask)), "ebm_import_columns")

    def sync(self):
        check(self.lib.ebm_sync(self._h), "ebm_sync")

    # -- measurement ------------------------------------------------------------------
    def counters(self) -> dict:
        c = (C.c_longlong * 4)()
        check(self.lib.ebm_get_counters(self._h, c), "ebm_get_counters")
        return dict(steps=c[0], solves=c[1], cap_hits=c[2], launches=c[3])

    def reset_counters(self):
        check(self.lib.ebm_reset_counters(self._h), "ebm_reset_counters")

    def state_conversions(self) -> int:
        """Layout conversions of the prognostic fields so far (ebm_state_conversions)."""
        n = C.c_longlong()
        check(self.lib.ebm_state_conversions(self._h, C.byref(n)), "ebm_state_conversions")
        return int(n.value)

    def zero_line_flags(self):
        """(words, trusted) of ebm_zero_line_flags: uint32 [ncol][threads / 64], and whether every set bit is true now."""
        words = np.zeros((self.ncol, self.launch_info()["threads"] // 64), dtype=np.uint32)
        trusted = C.c_int()
        check(self.lib.ebm_zero_line_flags(self._h, words.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(trusted)),
              "ebm_zero_line_flags")
        return words, bool(trusted.value)

    def timer_start(self):
        check(self.lib.ebm_timer_start(self._h), "ebm_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(self.lib.ebm_timer_stop(self._h, C.byref(ms)), "ebm_timer_stop")
        return float(ms.value)

    def launch_info(self) -> dict:
        info = (C.c_int * 4)()
        check(self.lib.ebm_launch_info(self._h, info), "ebm_launch_info")
        return dict(threads=info[0], cells_per_thread=info[1], lds_bytes=info[2], workgroups=info[3])
