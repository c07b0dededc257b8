"""Ensembles and 2-D (lat x lon) grids: many independent meridians per handle, sharded across
GPUs by column.

The reference has no longitude axis and no ensemble mechanism; columns never
exchange data, so the natural shard is the column.  One process per GPU owns a contiguous
block of columns; the only communication is I/O (broadcast of the grid/parameters, gather of
per-column diagnostics) over ``torch.distributed`` (backend "nccl" = RCCL on ROCm, "gloo" on
CPU for tests).  No collective sits inside the time loop.
"""
from __future__ import annotations

import numpy as np

from ._lib import PARAM_ORDER, StaleFieldError
from .engine import Engine, as_names, param_matrix, param_vector
from .infrastructure import default_parval
from .noise import check_args as check_noise_args


def _sharded(dist) -> bool:
    """More than one rank: ``dist`` (torch.distributed) is given, initialised and its world is larger than one."""
    return dist is not None and dist.is_initialized() and dist.get_world_size() > 1


def _backend(dist) -> str:
    try:
        return str(dist.get_backend())
    except Exception:
        return ""


def _steps_per_launch(k):
    """The steps fused into one launch by ``run``, ``series`` and ``first_passage``: the caller's, 64 if None."""
    return 64 if k is None else k


def shard_columns(ncol: int, world_size: int, rank: int) -> slice:
    """Contiguous block partition of ``ncol`` columns: the first ``ncol % world_size`` ranks
    get one extra column."""
    if not (0 <= rank < world_size):
        raise ValueError("rank out of range")
    base, extra = divmod(ncol, world_size)
    start = rank * base + min(rank, extra)
    return slice(start, start + base + (1 if rank < extra else 0))


def hemispheric_mean(vec: np.ndarray, x: np.ndarray) -> np.ndarray:
    """Trapezoid integral over x of each column (reference src/utilities.jl:397-403), summed
    strictly left to right as the reference's loop does (np.cumsum is sequential)."""
    v = np.asarray(vec, dtype=np.float64)
    return np.cumsum((v[..., :-1] + v[..., 1:]) * (x[1:] - x[:-1]) / 2.0, axis=-1)[..., -1]


def member_param_rows(member_params, par, init, fcol=None, forcings=None) -> np.ndarray:
    """The [members, 25] parameter rows of ``EnsembleRun(..., member_params=...)``, after checking that the per-member
    inputs agree on the member count: 2-D ``init`` arrays, ``fcol`` and ``forcings``.  Host only (no device call)."""
    n = len(member_params)
    if n < 1:
        raise ValueError("member_params: need at least one member")
    for k, v in init.items():
        a = np.asarray(v)
        if a.ndim != 1 and a.shape[0] != n:
            raise ValueError(f"member_params has {n} members but init[{k!r}] has {a.shape[0]} columns")
    if fcol is not None and len(fcol) != n:
        raise ValueError(f"member_params has {n} members but fcol has {len(fcol)}")
    if forcings is not None and len(forcings) != n:
        raise ValueError(f"member_params has {n} members but forcings has {len(forcings)}")
    return param_matrix(member_params, par, default_parval)


def passage_levels(ncol: int, level, direction):
    """The per-member ``level`` [ncol] float64 and ``direction`` [ncol] (+1 upward, -1 downward) of
    ``EnsembleRun.first_passage``: each a scalar (every member) or one entry per member; a direction is "up", "down" or an
    integer other than 0.  Host only (no device call)."""
    lev = np.asarray(level, dtype=np.float64)
    if lev.ndim > 1 or (lev.ndim == 1 and lev.shape[0] != ncol):
        raise ValueError(f"level: expected a scalar or {ncol} values, got shape {lev.shape}")
    lev = np.ascontiguousarray(np.broadcast_to(lev, (ncol,)))
    if np.isnan(lev).any():
        raise ValueError("level: NaN (+-inf is legal: never, or at the first sample)")
    words = {"up": 1, "down": -1}
    d = [direction] if isinstance(direction, str) or np.ndim(direction) == 0 else list(direction)
    if len(d) not in (1, ncol):
        raise ValueError(f"direction: expected a scalar or {ncol} values, got {len(d)}")
    out = np.empty(len(d), dtype=np.int32)
    for i, v in enumerate(d):
        if isinstance(v, str):
            if v not in words:
                raise ValueError(f"direction: {v!r} is neither 'up' nor 'down'")
            out[i] = words[v]
        elif isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v == 0:
            raise ValueError(f"direction: {v!r} is neither 'up' / a positive integer nor 'down' / a negative integer")
        else:
            out[i] = 1 if v > 0 else -1
    return lev, np.ascontiguousarray(np.broadcast_to(out, (ncol,)))


def scalar_spec(st, kind, name, band=None, level=None):
    """One column scalar for ``EnsembleRun.scalars`` / ``scalar_series`` / ``first_passage_scalar`` (the tuple
    ``Engine.check_scalar_args`` takes): ``kind`` "integral", "mean", "edge_ge" or "edge_le" of field ``name`` over ``band`` =
    (x_lo, x_hi) in the grid's coordinate ``st.x`` — the cells whose x lies inside, both ends inclusive; None: the whole
    meridian.  An empty band is refused, and so is a band of one cell for the integral kinds.  ``level``: the edge kinds'.
    Host only (no device call)."""
    x = np.asarray(st.x, dtype=np.float64)
    if band is None:
        k0, k1 = 0, len(x) - 1
    else:
        lo, hi = (float(b) for b in band)
        if not lo <= hi:
            raise ValueError(f"band: expected (x_lo, x_hi) with x_lo <= x_hi, got {band!r}")
        inside = np.flatnonzero((x >= lo) & (x <= hi))
        if inside.size == 0:
            raise ValueError(f"band: no cell of the grid lies in [{lo}, {hi}]")
        k0, k1 = int(inside[0]), int(inside[-1])
    if kind in ("integral", "mean") and k0 == k1:
        raise ValueError(f"band: one cell (x[{k0}] = {x[k0]}) carries no {kind}")
    if kind in ("edge_ge", "edge_le") and (level is None or np.isnan(float(level))):
        raise ValueError(f"{kind}: needs a level that is not NaN")
    return (kind, name, k0, k1) if level is None else (kind, name, k0, k1, float(level))


def selection_parents(weights, rng) -> np.ndarray:
    """Systematic resampling: the parents [n] (int32, ascending) of the next generation of ``n = len(weights)`` members,
    member m getting ``floor(n w_m)`` or ``ceil(n w_m)`` offspring (w: the weights normalised to sum 1).  One uniform
    draw u from ``rng`` (a ``numpy.random.Generator``), then the n pointers u, u + 1, ..., u + n - 1 through the
    cumulative weights scaled to n: pointer j falls into member parents[j]'s interval.  The result is ascending, so a
    survivor stays in its slot, and ``resample`` moves nothing for it, as long as the cumulative weights up to it are
    within one slot of its index — nearly equal weights; once the relative spread of the weights exceeds about
    1 / sqrt(n), most members change slot (tests/tools/resample_cost.py prints the share).  Equal weights give the
    identity (whatever u is) and a member of weight 0 has no offspring.  Host only (no device call).  ValueError for negative or
    non-finite weights and for an all-zero sum."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim != 1 or w.shape[0] < 1:
        raise ValueError(f"weights: expected a vector of at least one weight, got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError("weights: expected finite values")
    if (w < 0.0).any():
        raise ValueError("weights: expected values >= 0")
    n = w.shape[0]
    u = rng.random()                                     # drawn in every case: the caller's stream does not depend on w
    if w.max() == 0.0:
        raise ValueError("weights: all zero (no member to continue from)")
    if (w == w[0]).all():
        return np.arange(n, dtype=np.int32)              # by definition, not up to the rounding of the cumulative sums
    cum = np.cumsum(w)
    cum *= n / cum[-1]
    cum[np.flatnonzero(w > 0.0)[-1]:] = np.inf           # the last pointer cannot fall behind the last live member
    return np.searchsorted(cum, u + np.arange(n), side="right").astype(np.int32)


def assimilation_weights(J, prior_logw=None) -> dict:
    """The particle-filter weights of members whose misfits to an observation are ``J`` [n] (``EnsembleRun.misfits``: J =
    sum (x - y)^2 / sigma^2, so the Gaussian likelihood is exp(-J / 2)): dict(weights [n]: normalised to sum 1; ess: the
    effective sample size (sum w)^2 / sum w^2, n for equal weights and 1 when one member carries everything; log_evidence:
    the log of the prior-weighted mean likelihood, log sum_m p_m exp(-J_m / 2) with p the normalised prior — the increment
    of the log marginal likelihood of this observation).  ``prior_logw`` [n]: log weights carried from earlier
    observations that were not resampled away (None: equal).  A stable softmax of -J / 2 + prior_logw: the largest
    exponent is subtracted first, so a member far from the observation gets weight 0.0 by underflow, never NaN; J = +Inf
    (an Inf cell) gives weight 0.  Host only.  ValueError for a NaN or negative J, a NaN or +Inf prior, and when no member has a
    positive weight."""
    J = np.asarray(J, dtype=np.float64)
    if J.ndim != 1 or J.shape[0] < 1:
        raise ValueError(f"J: expected a vector of at least one misfit, got shape {J.shape}")
    if np.isnan(J).any() or (J < 0.0).any():
        raise ValueError("J: expected misfits >= 0 (not NaN)")
    prior = np.zeros_like(J) if prior_logw is None else np.asarray(prior_logw, dtype=np.float64)
    if prior.shape != J.shape or np.isnan(prior).any() or (prior == np.inf).any():
        raise ValueError(f"prior_logw: expected {J.shape[0]} log weights (finite or -inf)")
    logw = prior - 0.5 * J
    top, top_prior = logw.max(), prior.max()
    if top == -np.inf:
        raise ValueError("every member has weight zero (no member to continue from)")
    w = np.exp(logw - top)
    total = w.sum()
    log_evidence = (top + np.log(total)) - (top_prior + np.log(np.exp(prior - top_prior).sum()))
    return dict(weights=w / total, ess=float(total * total / (w * w).sum()), log_evidence=float(log_evidence))


# ---- genealogical cloning (Giardina-Kurchan-Lecomte-Tailleur), host side ------------------------------------------------------
# EXPERIMENTAL: the three gklt_* functions are here so that examples/rare_transitions_gklt.py and the host tests share one
# statement of the estimator; their signatures may change.  selection_parents and EnsembleRun.resample are the supported part.
# Members are slots 0 .. n-1.  An interval advances every slot and scores it; the selection after it makes slot c continue
# from slot parents[c].  The functions below are pure NumPy: `advance` and `resample` are the caller's (EnsembleRun.series
# and EnsembleRun.resample in examples/rare_transitions_gklt.py, a toy process in tests/test_host_resample.py).

def gklt_run(advance, resample, n, nintervals, k, rng):
    """``nintervals`` rounds of: V = advance(i) — the [n] scores of interval i, the time integral of the tilting observable
    over the interval for every slot; weights exp(k V); parents = selection_parents(weights, rng); resample(parents).
    Returns dict(scores [nintervals, n]: V by slot; parents [nintervals, n] int32: the genealogy; log_norm: the log of the
    product over the intervals of the mean weight).  k = 0 selects nothing: every parents row is the identity."""
    scores = np.empty((nintervals, n))
    parents = np.empty((nintervals, n), dtype=np.int32)
    log_norm = 0.0
    for i in range(nintervals):
        v = np.asarray(advance(i), dtype=np.float64)
        if v.shape != (n,):
            raise ValueError(f"advance({i}) returned shape {v.shape}, expected {(n,)}")
        e = k * v
        top = e.max()
        w = np.exp(e - top)
        log_norm += float(np.log(w.mean()) + top)
        parents[i] = selection_parents(w, rng)
        resample(parents[i])
        scores[i] = v
    return dict(scores=scores, parents=parents, log_norm=log_norm)


def gklt_lineage(parents, values, reduce=np.add) -> np.ndarray:
    """``values`` [nintervals, n] were recorded by slot during each interval (before its selection): returns, for every
    slot after the last selection, ``reduce`` over the intervals of the value of its ANCESTOR in that interval — the sum
    of the scores along the member's line of descent (np.add), the lowest <T> it has seen (np.minimum)."""
    parents, values = np.asarray(parents), np.asarray(values)
    anc = np.arange(parents.shape[1])
    out = None
    for i in range(parents.shape[0] - 1, -1, -1):
        anc = parents[i][anc]                            # the slot that held this line during interval i
        out = values[i][anc] if out is None else reduce(values[i][anc], out)
    return out


def gklt_estimate(observable, score_sum, k, log_norm=0.0) -> dict:
    """The re-weighted expectation of ``observable`` [n] (one value per final member, of its whole line) under the
    UNTILTED dynamics, from a run tilted by exp(k * score): with u_m = exp(-k * score_sum[m]), score_sum the sum of the
    scores along the member's line (gklt_lineage),
        raw(O) = exp(log_norm) * mean(O u)     the GKLT estimator; raw(1) is 1 only in expectation, because a member has a
                                               whole number of offspring
        estimate = raw(O) / raw(1) = sum(O u) / sum(u)    self-normalised: exactly 1 for O = 1, the plain mean for k = 0.
    Returns dict(estimate, norm = raw(1), ess = sum(u)^2 / sum(u^2): the effective number of members)."""
    o = np.asarray(observable, dtype=np.float64)
    e = -(k * np.asarray(score_sum, dtype=np.float64))
    top = e.max()
    u = np.exp(e - top)
    total = np.sum(u)
    return dict(estimate=float(np.sum(o * u) / total), norm=float(np.exp(log_norm + top) * (total / u.shape[0])),
                ess=float(total * total / np.sum(u * u)))


# ---- selection across shards -------------------------------------------------------------------------------------------------
# EnsembleRun.resample is rank-local.  With the ensemble sharded by shard_columns, a parent may live on another rank: the plan
# below splits one global parents vector into, per rank, a rank-local gather and the whole columns that cross ranks, which
# travel as records of ebm_export_columns / ebm_import_columns.  Pure NumPy.

class ResamplePlan:
    """Rank ``rank``'s part of one global selection (``resample_plan``).  With n_r the rank's columns:
    ``send[q]``: the sorted distinct LOCAL columns of this rank that some column of rank q names as parent (empty for q ==
    rank); ``local`` [n_r] int32: the parents within the shard, ``local[c] = c`` for a column fed from another rank;
    ``recv_cols`` / ``recv_src`` / ``recv_idx``: for every remotely fed local column its index, its source rank and its index
    into that rank's send list to this rank; ``recv_counts[q]``: the length of rank q's send list to this rank.  The records a
    rank receives are those send lists concatenated in rank order, so column recv_cols[i] takes record
    ``recv_records[i] = sum(recv_counts[:recv_src[i]]) + recv_idx[i]``."""

    def __init__(self, rank, ncol, send, local, recv_cols, recv_src, recv_idx, recv_counts):
        self.rank, self.ncol, self.send, self.local = rank, ncol, send, local
        self.recv_cols, self.recv_src, self.recv_idx, self.recv_counts = recv_cols, recv_src, recv_idx, recv_counts
        self.send_counts = np.array([len(s) for s in send], dtype=np.int64)
        self.send_cols = np.concatenate(send).astype(np.int32) if send else np.zeros(0, np.int32)
        offsets = np.concatenate([[0], np.cumsum(recv_counts)[:-1]]).astype(np.int64)
        self.recv_records = (offsets[recv_src] + recv_idx).astype(np.int32)


def resample_plan(parents_global, ncol_total: int, world_size: int) -> list:
    """The plans of all ranks, ``[ResamplePlan] * world_size``, for the selection "member c continues from member
    ``parents_global[c]``" over an ensemble of ``ncol_total`` members sharded by ``shard_columns``.  Carried out as: every
    rank exports ``send`` (old state), then gathers ``local`` within its shard, then imports what it received — the result
    is the unsharded ``resample(parents_global)``.  Empty shards (``ncol_total < world_size``) are legal.  Host only; ValueError
    for a wrong length, an out-of-range parent or a non-integer dtype."""
    ncol_total, world_size = int(ncol_total), int(world_size)
    if ncol_total < 1 or world_size < 1:
        raise ValueError(f"resample_plan: need ncol_total >= 1 and world_size >= 1, got {ncol_total} and {world_size}")
    p = np.asarray(parents_global)
    if p.dtype.kind not in "iu":
        raise ValueError(f"parents_global: expected {ncol_total} integers (member indices), got dtype {p.dtype}")
    if p.shape != (ncol_total,):
        raise ValueError(f"parents_global: expected {ncol_total} integers, one per member, got shape {p.shape}")
    bad = np.flatnonzero((p < 0) | (p >= ncol_total))
    if bad.size:
        raise ValueError(f"parents_global[{int(bad[0])}] = {int(p[bad[0]])} is outside [0, {ncol_total})")
    p = p.astype(np.int64)
    shards = [shard_columns(ncol_total, world_size, r) for r in range(world_size)]
    starts = np.array([s.start for s in shards] + [ncol_total])
    owner = np.searchsorted(starts, np.arange(ncol_total), side="right") - 1      # (an empty shard owns nobody)
    # send[r][q]: the parents on r that the columns of q name, as local columns of r
    send = [[np.zeros(0, np.int32) for _ in range(world_size)] for _ in range(world_size)]
    for q in range(world_size):
        mine = p[shards[q]]
        src = owner[mine]
        for r in np.unique(src):
            if r != q:
                send[r][q] = (np.unique(mine[src == r]) - shards[r].start).astype(np.int32)
    plans = []
    for r in range(world_size):
        n = shards[r].stop - shards[r].start
        mine = p[shards[r]]
        src = owner[mine]
        remote = np.flatnonzero(src != r)
        local = np.where(src == r, mine - shards[r].start, np.arange(n)).astype(np.int32)
        idx = np.array([np.searchsorted(send[src[c]][r], mine[c] - shards[src[c]].start) for c in remote], dtype=np.int32)
        counts = np.array([len(send[q][r]) for q in range(world_size)], dtype=np.int64)
        plans.append(ResamplePlan(r, n, send[r], local, remote.astype(np.int32), src[remote].astype(np.int32), idx, counts))
    return plans


class ColumnExchange:
    """The sharded selection in terms of three methods of the class it is mixed into: ``export_tensor(cols) -> (records
    [n, R], mask)``, ``import_tensor(cols, records, mask, records_index)`` and ``resample(parents)``.  EnsembleRun is one."""

    def resample_export(self, plan):
        """First half of a sharded selection: the records of all of ``plan``'s send lists, concatenated in rank order, in
        one tensor, and their mask.  EVERY rank exports before ANY rank imports: remote parents are read in their old state."""
        return self.export_tensor(plan.send_cols)

    def resample_import(self, plan, received, mask):
        """Second half: the rank-local ``resample(plan.local)``, then the import of ``received`` — the send lists of all
        ranks to this one, concatenated in rank order — into the remotely fed columns."""
        self.resample(plan.local)
        if len(plan.recv_cols):
            self.import_tensor(plan.recv_cols, received, mask, plan.recv_records)

    def resample_global(self, parents_global, ncol_total, dist=None):
        """``resample`` over the whole sharded ensemble: member c (global index) continues from member
        ``parents_global[c]``, on whichever rank it lives — export, exchange, import, in that order; the result is the
        unsharded ``resample(parents_global)`` bit for bit.  Every rank passes the same ``parents_global``.  One small
        ``all_gather`` checks that all ranks hold the same mask and record size.  With the "nccl" backend (RCCL) the
        exchange is one ``all_to_all_single`` with the plan's split sizes and the payload stays on the device; with any
        other backend (gloo has no all-to-all) the records go through the host by ``isend`` / ``irecv``.  With ``dist``
        absent or a world of one it is ``resample``."""
        if not _sharded(dist):
            return self.resample(parents_global)
        import torch
        ws, rank = dist.get_world_size(), dist.get_rank()
        plan = resample_plan(parents_global, ncol_total, ws)[rank]
        buf, mask = self.resample_export(plan)
        nccl = _backend(dist) == "nccl"
        mine = torch.tensor([buf.shape[1], mask], dtype=torch.int64, device=buf.device if nccl else "cpu")
        every = [torch.empty_like(mine) for _ in range(ws)]
        dist.all_gather(every, mine)
        for q, t in enumerate(every):
            if t.tolist() != mine.tolist():
                raise RuntimeError(f"resample_global: rank {q} exports records of {int(t[0])} doubles with mask {int(t[1]):#x}, "
                                   f"rank {rank} of {int(mine[0])} with mask {int(mine[1]):#x} (every rank must hold the same "
                                   "model and shape, and the same fields current)")
        n_in, n_out = [int(v) for v in plan.send_counts], [int(v) for v in plan.recv_counts]
        if nccl:
            received = torch.empty((sum(n_out), buf.shape[1]), dtype=buf.dtype, device=buf.device)
            dist.all_to_all_single(received, buf.contiguous(), n_out, n_in)
        else:
            host = buf.cpu().contiguous()
            got = torch.empty((sum(n_out), buf.shape[1]), dtype=buf.dtype)
            work, a, b = [], 0, 0
            for q in range(ws):
                if n_out[q]:
                    work.append(dist.irecv(got[b:b + n_out[q]], src=q))
                if n_in[q]:
                    work.append(dist.isend(host[a:a + n_in[q]], dst=q))
                a, b = a + n_in[q], b + n_out[q]
            for w in work:
                w.wait()
            received = got.to(buf.device)
        self.resample_import(plan, received, mask)


# ---- moments across the members ------------------------------------------------------------------------------------------------
# ebm_ensemble_sums reduces across the columns on the device: S0 = sum w, S1 = sum w d, S2 = sum (w d) d per latitude, d = x -
# center.  The arithmetic from sums to moments is host NumPy on O(nlat) numbers.

def moments_from_sums(sums1, sums2=None) -> dict:
    """Mean and variance from the packed sums [..., 3, nlat] of ebm_ensemble_sums, in two passes: ``sums1`` taken with
    ``center=None`` gives ``weight = S0`` and ``mean = S1 / S0``; ``sums2`` taken with ``center = mean`` (``moments_center``)
    gives ``var = S2 / S0 - (S1 / S0) ** 2``, whose second term is of rounding size by construction (S1 is then the sum of the
    deviations from the mean).  A latitude with S0 == 0 — no contributing member — gives NaN mean and variance.  Without
    ``sums2`` the variance is left out.  Pure NumPy (no device call)."""
    a = np.asarray(sums1, dtype=np.float64)
    if a.ndim < 2 or a.shape[-2] != 3:
        raise ValueError(f"sums1: expected [..., 3, nlat] (S0, S1, S2), got shape {a.shape}")
    with np.errstate(divide="ignore", invalid="ignore"):
        s0 = a[..., 0, :]
        out = dict(weight=s0.copy(), mean=np.where(s0 == 0.0, np.nan, a[..., 1, :] / s0))
        if sums2 is not None:
            b = np.asarray(sums2, dtype=np.float64)
            if b.shape != a.shape:
                raise ValueError(f"sums2: expected the shape of sums1 {a.shape}, got {b.shape}")
            t0 = b[..., 0, :]
            m1 = b[..., 1, :] / t0
            out["var"] = np.where(t0 == 0.0, np.nan, b[..., 2, :] / t0 - m1 * m1)
    return out


def moments_center(mean) -> np.ndarray:
    """The ``center`` of the second pass: ``mean`` with 0.0 where it is not finite (a latitude without a contributor has no
    mean, and a center must be finite; that latitude's variance is NaN whatever is subtracted)."""
    m = np.asarray(mean, dtype=np.float64)
    return np.ascontiguousarray(np.where(np.isfinite(m), m, 0.0))


# ---- quantiles across the members ----------------------------------------------------------------------------------------------
# ebm_ensemble_range and ebm_ensemble_histogram reduce across the columns on the device; the bracketing from histograms to
# quantiles is host NumPy on O(nbins * nlat) numbers.

QUANTILE_NBINS, QUANTILE_PASSES = 32, 4          # the defaults of ``quantiles``
QUANTILE_PAD_ULPS = 16.0


def widened_bracket(lo, hi, nbins):
    """[lo, hi) widened on both sides by QUANTILE_PAD_ULPS ulps of max(|lo|, |hi|) — more than the roundings of the bin edges
    on the host (lo + i * ((hi - lo) / nbins): three) and of t = (x - lo) * s on the device (the difference, s, the product)
    can move a value across an edge, each at most one ulp of max(|lo|, |hi|) or 2^-53 of hi - lo <= 2 max — and to at least
    nbins * 2^-1020, so that nbins / (hi - lo) is finite."""
    pad = QUANTILE_PAD_ULPS * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
    lo, hi = lo - pad, hi + pad
    tiny = nbins * 2.0 ** -1020
    narrow = hi - lo < tiny
    return np.where(narrow, lo - tiny, lo), np.where(narrow, hi + tiny, hi)


def bracket_quantiles(histogram, rng, q, nbins, passes):
    """The bracketing of ``EnsembleMoments.quantiles`` for m entries: ``histogram(lo, hi) -> [m, nbins + 2, nlat]`` with lo,
    hi [m, nlat] (entry i of the call is the field of pair i), ``rng`` [m, 3, nlat] the range of each entry's field, ``q``
    [m] its level.  Returns (value, halfwidth), each [m, nlat].  Pure NumPy but for the calls of ``histogram``."""
    rng, q = np.asarray(rng, dtype=np.float64), np.asarray(q, dtype=np.float64)
    n, mn, mx = rng[:, 0], rng[:, 1], rng[:, 2]
    value, half = np.full(n.shape, np.nan), np.full(n.shape, np.nan)
    with np.errstate(all="ignore"):
        finite = np.isfinite(mn) & np.isfinite(mx) & np.isfinite(mx - mn)
    some = n > 0
    const = some & finite & (mx == mn)
    value[const], half[const] = mn[const], 0.0
    half[some & ~finite] = np.inf
    live = some & finite & (mx > mn)
    if not live.any():
        return value, half
    lo, hi = widened_bracket(np.where(live, mn, 0.0), np.where(live, mx, 1.0), nbins)      # (a dummy [0, 1) elsewhere)
    stuck = "quantiles: the bracket could not be restored (did the fields or the weights change between the passes?)"
    for _ in range(passes):
        for attempt in range(64):
            # [m, nlat, slots]: the slots contiguous, so that the cumulative sums run along memory
            h = np.ascontiguousarray(np.moveaxis(np.asarray(histogram(np.ascontiguousarray(lo), np.ascontiguousarray(hi))), 1, 2))
            cum = np.cumsum(h, axis=2)
            target = q[:, None] * cum[:, :, -1]
            reached = (h > 0.0) & (cum >= target[:, :, None])         # the first slot that holds weight and reaches the target
            slot = np.argmax(reached, axis=2)
            out = live & (~reached.any(axis=2) | (slot == 0) | (slot == nbins + 1))
            if not out.any():
                break
            with np.errstate(over="ignore", invalid="ignore"):
                grow = 4.0 ** attempt * (hi - lo)                     # the sought value left the bracket: widen, repeat the pass
                lo, hi = np.where(out, lo - grow, lo), np.where(out, hi + grow, hi)
                usable = np.isfinite(lo) & np.isfinite(hi) & np.isfinite(hi - lo)
            if not usable.all():
                raise RuntimeError(stuck)
        else:
            raise RuntimeError(stuck)
        step = (hi - lo) / nbins
        a, b = widened_bracket(lo + (slot - 1) * step, lo + slot * step, nbins)
        lo, hi = np.where(live, a, lo), np.where(live, b, hi)
    width = hi - lo
    value[live], half[live] = (lo + width / 2.0)[live], (width / 2.0)[live]
    return value, half


class EnsembleMoments:
    """Moments across the members in terms of two methods of the class it is mixed into: ``ensemble_sums(names, weights,
    center) -> ndarray [nvars, 3, nlat]`` and ``ensemble_sums_tensor(names, weights, center)``, the same as a device tensor.
    EnsembleRun is one."""

    def _across_ranks(self, dist, kind, *args, slot_ops=None) -> np.ndarray:
        """This shard's packed result [entries, slots, nlat] of ``ensemble_<kind>(*args)``, all-reduced over the ranks of
        ``dist``: with the "nccl" backend (RCCL) the payload is the device tensor ``ensemble_<kind>_tensor(*args)`` wrote and
        comes to the host once, afterwards; with any other backend (gloo) it is staged on the CPU, as ``gather_columns``
        does.  One SUM over everything, or slot q on its own with ``ReduceOp`` ``slot_ops[q]``.  With ``dist`` absent or a
        world of one: the shard's own result."""
        if not _sharded(dist):
            return getattr(self, "ensemble_" + kind)(*args)
        import torch
        if _backend(dist) == "nccl":
            t = getattr(self, "ensemble_" + kind + "_tensor")(*args)
        else:
            t = torch.from_numpy(np.ascontiguousarray(getattr(self, "ensemble_" + kind)(*args)))
        if slot_ops is None:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return t.cpu().numpy()
        parts = []
        for q, op in enumerate(slot_ops):
            part = t[:, q].contiguous()
            dist.all_reduce(part, op=getattr(dist.ReduceOp, op))
            parts.append(part.cpu().numpy())
        return np.stack(parts, axis=1)

    def reduced_sums(self, names, weights=None, center=None, dist=None) -> np.ndarray:
        """This shard's packed sums, all-reduced (SUM) over the ranks of ``dist``: with the "nccl" backend (RCCL) the payload
        is the device tensor the reduction wrote and comes to the host once, afterwards; with any other backend (gloo) it is
        staged on the CPU, as ``gather_columns`` does.  With ``dist`` absent or a world of one: the shard's own sums."""
        return self._across_ranks(dist, "sums", names, weights, center)

    def moments(self, names=("T", "phi"), weights=None, dist=None) -> dict:
        """Weighted mean and variance ACROSS the members, per latitude, of every field in ``names``: ``{name: {"weight": S0,
        "mean": ..., "var": ...}}``, each [nlat].  Two passes of ebm_ensemble_sums, reduced on the device — O(nlat) numbers
        leave it, never the fields: pass 1 without a center gives ``mean = S1 / S0``; pass 2 centered on that mean gives
        ``var = S2 / S0 - (S1 / S0) ** 2`` (``moments_from_sums``).  ``weights`` [ncol of this shard]: None for the plain
        ensemble mean, zeros to leave members out (the mean ice profile of the members that tipped), importance weights
        such as ``gklt_estimate``'s exp(-k * score_sum) for the mean under the untilted dynamics; negative weights are
        legal.  A member contributes at a latitude iff its weight is not 0 and its cell is not NaN (the "no ice / no water
        here" sentinels of Ti and Tw); a latitude with S0 == 0 has NaN mean and variance.
        With ``dist`` the packed sums of the shards are all-reduced (SUM) between and after the passes (``reduced_sums``), so
        every rank returns the moments of the whole ensemble.  Each shard's own sums are defined to the bit (blocks of 32
        members in ascending order, then the blocks in ascending order).  Across shards the sums are added in another order
        than the unsharded call adds them, so they are not equal bit for bit: a term of a call over m members passes through
        at most D(m) = min(m, 32) + ceil(m / 32) - 2 rounded adds and the combination of n shards adds n - 1 more, so the
        combined sums agree with the unsharded ones to within (D(ncol) + max_r D(ncol_r) + n - 1) * 2^-53 * sum|terms| per
        latitude, ncol_r the members of shard r."""
        names = as_names(names)
        s1 = np.asarray(self.reduced_sums(names, weights, None, dist))
        center = moments_center(moments_from_sums(s1)["mean"])
        s2 = np.asarray(self.reduced_sums(names, weights, center, dist))
        m = moments_from_sums(s1, s2)
        return {n: {k: m[k][i] for k in ("weight", "mean", "var")} for i, n in enumerate(names)}

    # ---- order statistics across the members: ebm_ensemble_range and ebm_ensemble_histogram ----------------------------------
    # The class it is mixed into also has ``ensemble_range(names, weights)``, ``ensemble_histogram(names, lo, hi, nbins,
    # weights)`` and their ``_tensor`` forms (device tensors, for RCCL).

    def range(self, names, weights=None, dist=None) -> np.ndarray:
        """[len(names), 3, nlat]: the number n of contributing members, their minimum and their maximum per latitude
        (ebm_ensemble_range) — of the whole ensemble with ``dist``: n is all-reduced with SUM, min with MIN, max with MAX,
        which is exact, so every rank holds the bits of the unsharded call (up to which of +0.0 and -0.0 an extreme is)."""
        return self._across_ranks(dist, "range", names, weights, slot_ops=("SUM", "MIN", "MAX"))

    def histogram(self, names, lo, hi, nbins, weights=None, dist=None) -> np.ndarray:
        """[len(names), nbins + 2, nlat]: the weighted histogram across the members per latitude (ebm_ensemble_histogram:
        below ``lo`` | nbins bins | at and above ``hi``) — of the whole ensemble with ``dist`` (all-reduced with SUM; with unit
        weights every slot is an exact count and the result is the unsharded one bit for bit).  A name may be repeated,
        each entry with its own rows of ``lo`` and ``hi``."""
        return self._across_ranks(dist, "histogram", names, lo, hi, nbins, weights)

    def quantiles(self, names=("T", "phi"), q=(0.05, 0.5, 0.95), weights=None, dist=None, nbins=QUANTILE_NBINS,
                  passes=QUANTILE_PASSES) -> dict:
        """Weighted inverted-CDF quantiles ACROSS the members, per latitude: ``{name: {"value": [nq, nlat], "halfwidth": [nq,
        nlat]}}``.  The quantile q is the smallest contributing value whose cumulative weight reaches q * (sum of the
        weights); a member contributes iff its weight is not 0 and its cell is not NaN.  ``weights`` must be >= 0.  Nothing
        but O(nbins * nlat) numbers per pass leaves the device: one ``range`` gives [min, max] per latitude; each of
        ``passes`` ``histogram`` calls finds the slot in which the cumulative weight — the weight below ``lo`` included —
        first reaches the target, and the next pass spreads its bins over that bin, widened by 16 ulps of max(|lo|, |hi|) so
        that the rounding of (x - lo) * s cannot push the sought value out of it; if it lands below or above all the same,
        the bracket is widened and that pass repeated.  All (name, q) pairs refine in ONE histogram call per pass (a field
        may be listed several times there), more than 12 pairs in groups of 12.  ``value`` is the midpoint of the final
        bracket and ``halfwidth`` half its width: the quantile lies within ``value`` +- ``halfwidth``, and halfwidth <=
        (max - min) * nbins ** -passes up to the widening.  A latitude where max == min returns that value with halfwidth 0
        and needs no histogram (ice-free latitudes, phi = 0 in every member); one without a contributor returns NaN; one
        whose min or max is not finite (or whose max - min overflows) returns NaN with halfwidth +Inf.  With weights that
        are not small integers the cumulative weights are the rounded sums of ebm_ensemble_histogram, compared as they are.
        Defaults: nbins = 32, passes = 4 — a final halfwidth of 2^-21 of the range.  Measured on one MI355X (DESIGN.md
        section 5), 32 bins x 4 passes is both finer and faster than 64 bins x 3 passes (2^-19): a histogram call costs up to
        1.3 times as much at 64 bins (66 KiB of LDS per workgroup instead of 34), and the host arithmetic on the O(nbins *
        nlat) slots per pair, which is most of the call's time, doubles.  With ``dist`` every rank returns the quantiles of
        the whole ensemble."""
        names = as_names(names)
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if qs.ndim != 1 or qs.size < 1 or not ((qs >= 0.0) & (qs <= 1.0)).all():
            raise ValueError(f"q: expected quantile levels in [0, 1], got {q!r}")
        if not 1 <= int(nbins) <= 64 or int(passes) < 1:
            raise ValueError(f"expected 1 <= nbins <= 64 and passes >= 1, got nbins = {nbins!r}, passes = {passes!r}")
        if weights is not None and not (np.asarray(weights, dtype=np.float64) >= 0.0).all():
            raise ValueError("weights: quantiles need weights >= 0")
        nbins, passes = int(nbins), int(passes)
        r = np.asarray(self.range(names, weights, dist))
        pairs = [(i, j) for i in range(len(names)) for j in range(qs.size)]
        value = np.full((len(names), qs.size, r.shape[-1]), np.nan)
        half = np.full_like(value, np.nan)
        for g in range(0, len(pairs), 12):
            group = pairs[g:g + 12]
            idx = [i for i, _ in group]
            v, hw = bracket_quantiles(lambda lo, hi: np.asarray(self.histogram([names[i] for i in idx], lo, hi, nbins, weights, dist)),
                                      r[idx], qs[[j for _, j in group]], nbins, passes)
            for m, (i, j) in enumerate(group):
                value[i, j], half[i, j] = v[m], hw[m]
        return {n: {"value": value[i], "halfwidth": half[i]} for i, n in enumerate(names)}


class CovarianceMixin(EnsembleMoments):
    """Covariances and EOFs across the members in terms of two more methods of the class it is mixed into:
    ``ensemble_covariance(name_a, name_b, weights, center_a, center_b) -> ndarray [nlat, nlat]`` and
    ``ensemble_covariance_tensor(...)``, the same as a device tensor — and of ``ensemble_sums`` for the means.  EnsembleRun
    is one."""

    def covariance(self, name_a, name_b=None, weights=None, dist=None) -> dict:
        """The weighted covariance ACROSS the members of ``name_a`` at latitude i with ``name_b`` (None: ``name_a``) at
        latitude j: ``{"mean_a": [nlat], "mean_b": [nlat], "cov": [nlat, nlat], "n": [nlat, nlat]}``.  One pass of
        ebm_ensemble_sums gives S0 and the means S1 / S0 of both fields; one pass of ebm_ensemble_covariance centred on those
        means gives the matrix of sums, which is divided ONCE, on the host, by ``n[i, j] = min(S0_a[i], S0_b[j])`` — the sum
        of the weights wherever no cell is NaN.  (Where the NaN sentinels of Ti or Tw thin a latitude out, the members that
        have both cells of a pair are at most that n; such entries are the sum over those members divided by n.)  A pair
        with n == 0 is NaN, and a latitude without a contributor is centred on 0.0 (``moments_center``).  nlat^2 numbers
        leave the device, never the fields.  ``weights`` [ncol of this shard] as in ``moments``.
        With ``dist`` the sums and then the matrices of the shards are all-reduced (SUM), so every rank returns the
        covariance of the whole ensemble.  Each shard's matrix is defined to the bit (ebm_ensemble_covariance); adding the
        shards' matrices adds the same terms in another order than the unsharded call does, so the two are NOT equal bit for
        bit, for the reason ``moments`` gives for the sums: they agree within the sum of their error bounds, each
        (n_members + blocks) * 2^-53 * sum|terms| * (1 + 2^-4) per element, plus one rounded add per further shard."""
        name_b = name_a if name_b is None else name_b
        names = (name_a,) if name_b == name_a else (name_a, name_b)
        s1 = np.asarray(self.reduced_sums(names, weights, None, dist))
        m = moments_from_sums(s1)
        mean_a, mean_b = m["mean"][0], m["mean"][-1]
        ca = moments_center(mean_a)
        cb = ca if name_b == name_a else moments_center(mean_b)
        c = np.asarray(self._across_ranks(dist, "covariance", name_a, name_b, weights, ca, cb))
        n = np.minimum.outer(m["weight"][0], m["weight"][-1])
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = np.where(n == 0.0, np.nan, c / n)
        return {"mean_a": mean_a, "mean_b": mean_b, "cov": cov, "n": n}

    def eofs(self, name, nmodes, weights=None, quad=None, dist=None) -> dict:
        """The leading ``nmodes`` EOFs (principal components) of ``name`` across the members: ``{"modes": [nmodes, nlat],
        "variance": [nmodes], "explained": [nmodes]}``.  ``covariance(name)`` is taken on the device; rows and columns are
        scaled by the square roots of the quadrature weights ``quad`` [nlat] >= 0 (None: all 1.0), so that the modes are
        orthonormal under sum_k quad_k u_k v_k; ``numpy.linalg.eigh`` runs on the host on that [nlat, nlat] matrix.  The
        modes come back in the field's own units (the eigenvectors divided by sqrt(quad); 0.0 where quad is 0) in
        descending order of variance, each with its largest-magnitude entry positive (the first of several), with their
        eigenvalues and their fractions of the total variance (the trace).  ValueError where the covariance is not finite
        (a latitude without a contributing member, as the NaN sentinels of Ti and Tw can leave one)."""
        c = self.covariance(name, None, weights, dist)["cov"]
        nlat = c.shape[0]
        if isinstance(nmodes, (bool, np.bool_)) or not isinstance(nmodes, (int, np.integer)) or not 1 <= int(nmodes) <= nlat:
            raise ValueError(f"nmodes: expected an int between 1 and {nlat}, got {nmodes!r}")
        q = np.ones(nlat) if quad is None else np.asarray(quad, dtype=np.float64)
        if q.shape != (nlat,) or not (np.isfinite(q) & (q >= 0.0)).all():
            raise ValueError(f"quad: expected {nlat} finite quadrature weights >= 0")
        if not np.isfinite(c).all():
            raise ValueError(f"eofs: the covariance of {name!r} is not finite (a latitude without a contributing member, or Inf in a cell)")
        s = np.sqrt(q)
        vals, vecs = np.linalg.eigh(s[:, None] * c * s[None, :])
        order = np.argsort(vals)[::-1][:int(nmodes)]
        with np.errstate(divide="ignore", invalid="ignore"):
            modes = np.where(s > 0.0, vecs[:, order].T / s, 0.0)
        big = np.argmax(np.abs(modes), axis=1)
        modes = modes * np.where(modes[np.arange(len(order)), big] < 0.0, -1.0, 1.0)[:, None]
        total = float(np.sum(vals))
        return {"modes": modes, "variance": vals[order], "explained": vals[order] / total if total > 0.0 else np.full(len(order), np.nan)}


def gaspari_cohn(r) -> np.ndarray:
    """The Gaspari-Cohn taper (1999, eq. 4.10): the compactly supported fifth-order piecewise rational function of
    r = distance / half-width >= 0 that resembles a Gaussian — 1 at r = 0, decreasing monotonically, exactly 0 for r >= 2.
    The Schur product of a sample covariance with it removes the spurious long-range correlations of a small ensemble and
    keeps the matrix positive semi-definite.  A host function: ``enkf`` applies it to nlat^2 numbers."""
    r = np.abs(np.asarray(r, dtype=np.float64))
    out = np.zeros_like(r)
    a = r <= 1.0
    b = (r > 1.0) & (r < 2.0)
    ra, rb = r[a], r[b]
    out[a] = (((-0.25 * ra + 0.5) * ra + 0.625) * ra - 5.0 / 3.0) * ra ** 2 + 1.0
    out[b] = (((rb / 12.0 - 0.5) * rb + 0.625) * rb + 5.0 / 3.0) * rb ** 2 - 5.0 * rb + 4.0 - 2.0 / (3.0 * rb)
    return np.clip(out, 0.0, 1.0)


MIZ_UPDATE_BOUNDS = {"Ei": (None, 0.0), "Ew": (0.0, None), "h": (0.0, None), "D": (0.0, "Dmax"), "phi": (0.0, 1.0)}


class KalmanMixin(CovarianceMixin):
    """The ensemble Kalman update in terms of the reductions above and ONE writer: ``update_columns(names, obs_name, gain,
    target, scale, perturb, bounds)`` of the class it is mixed into (ebm_update_columns), plus ``st.x`` for the taper and,
    for the perturbed-observation filter, ``obs_noise(sd, generator)`` -> [ncol, nlat] on the device.  EnsembleRun is one."""

    def default_update_bounds(self, names) -> dict:
        """The per-field bounds ``enkf`` applies when given none (none here; EnsembleRun knows its model's)."""
        return {}

    def kalman_gains(self, names, obs_name, obs, obs_var, localize=None, inflation=1.0, dist=None, solver="host") -> dict:
        """The host part of ``enkf``: ``{"gain": [len(names), nlat, nlat], "mean_o": [nlat], "var_o": [nlat], "observed":
        bool [nlat], "members": n}``.  P_oo = ``covariance(obs_name)`` and P_fo = ``covariance(f, obs_name)`` per field, each
        all-reduced over ``dist`` as ``covariance`` does and scaled to the unbiased estimate (n / (n - 1), n the members of the
        whole ensemble); with J the observed cells (``obs`` not NaN): S = rho o P_oo[J, J] * inflation + diag(obs_var[J]),
        G_f[:, J] = inflation * (rho o P_fo[:, J]) S^-1 by one Cholesky-free ``numpy.linalg.solve`` of the m x m system, zeros
        in the columns of unobserved cells.  rho = ``gaspari_cohn(|x_i - x_j| / localize)``, or all ones without ``localize``.
        ``solver="device"``: the same on the device (``_gains_on_device``), ``"gain"`` a torch tensor there, which
        ``update_columns`` takes where it lies; nothing of size nlat^2 touches the host.  Not with ``dist`` (ValueError): a
        sharded run uses the host solver."""
        names = as_names(names)
        if solver not in ("host", "device"):
            raise ValueError(f"solver = {solver!r}: expected 'host' or 'device'")
        x = np.asarray(self.st.x, dtype=np.float64)
        nlat = x.shape[0]
        y = np.asarray(obs, dtype=np.float64)
        if y.shape != (nlat,) or np.isinf(y).any():
            raise ValueError(f"obs: expected [{nlat}] finite values, NaN where nothing was observed")
        R = np.broadcast_to(np.asarray(obs_var, dtype=np.float64), (nlat,))
        J = ~np.isnan(y)
        if not (np.isfinite(R[J]) & (R[J] > 0.0)).all():
            raise ValueError("obs_var: expected finite values > 0 at the observed cells")
        if not (np.isfinite(inflation) and inflation > 0.0):
            raise ValueError(f"inflation = {inflation!r}: expected a finite factor > 0")
        if localize is not None and not (np.isfinite(localize) and localize > 0.0):
            raise ValueError(f"localize = {localize!r}: expected None or a half-width in x > 0")
        if solver == "device":
            if _sharded(dist):
                raise ValueError('solver="device" is for one shard: with `dist` use solver="host" (the all-reduce of the device '
                                 "covariances is not built)")
            return self._gains_on_device(names, obs_name, y, R, J, localize, float(inflation), dist)
        rho = np.ones((nlat, nlat)) if localize is None else gaspari_cohn(np.abs(x[:, None] - x[None, :]) / float(localize))
        oo = self.covariance(obs_name, None, None, dist)
        n = float(np.max(oo["n"]))
        if not n > 1.0:
            raise ValueError("enkf: needs more than one member")
        unbias = n / (n - 1.0)
        P_oo = oo["cov"] * unbias
        if not np.isfinite(P_oo[np.ix_(J, J)]).all():
            raise ValueError(f"enkf: the covariance of {obs_name!r} is not finite at the observed cells (a latitude without a "
                             "contributing member: observe it where it exists, or mark the cell unobserved)")
        S = rho[np.ix_(J, J)] * P_oo[np.ix_(J, J)] * float(inflation) + np.diag(R[J])
        gain = np.zeros((len(names), nlat, nlat))
        for v, f in enumerate(names):
            P_fo = oo["cov"] * unbias if f == obs_name else self.covariance(f, obs_name, None, dist)["cov"] * unbias
            B = float(inflation) * rho[:, J] * np.where(np.isfinite(P_fo[:, J]), P_fo[:, J], 0.0)
            gain[v][:, J] = np.linalg.solve(S, B.T).T if J.any() else 0.0      # S is symmetric
        return {"gain": gain, "mean_o": oo["mean_a"], "var_o": np.diag(P_oo).copy(), "observed": J, "members": int(n)}

    def _gains_on_device(self, names, obs_name, y, R, J, localize, inflation, dist) -> dict:
        """``kalman_gains`` with the covariances, the m x m system, its blocked Cholesky solve and the gain all on the device
        (ebm_kalman_gain_device), in terms of two more methods of the class it is mixed into: ``ensemble_covariance_tensor``
        and ``kalman_gain_tensor``.  One pass of the sums gives the weights and means of all fields, as in ``covariance``;
        every matrix of sums is written by ebm_ensemble_covariance_device and divided on the device by
        n[i, j] = min(S0_a[i], S0_b[j]); ``factor = inflation * n / (n - 1)``.  One shard only: ``kalman_gains`` refuses
        ``dist`` with this solver.  O(nlat) numbers come to the host: the sums, and the
        diagonal of P_oo for ``var_o``.  EBMError where the innovation covariance is not positive definite (a NaN covariance
        at an observed cell is reported so, with its latitude)."""
        import torch
        fields = (obs_name,) + tuple(f for f in names if f != obs_name)
        m = moments_from_sums(np.asarray(self.reduced_sums(fields, None, None, dist)))
        n = float(np.max(m["weight"][0]))
        if not n > 1.0:
            raise ValueError("enkf: needs more than one member")
        unbias = n / (n - 1.0)
        centers = [moments_center(m["mean"][i]) for i in range(len(fields))]

        def cov(i):
            t = self.ensemble_covariance_tensor(fields[i], obs_name, None, centers[i], centers[0])
            wa, wo = (torch.as_tensor(np.ascontiguousarray(m["weight"][q]), device=t.device) for q in (i, 0))
            cnt = torch.minimum(wa[:, None], wo[None, :])
            return torch.where(cnt == 0.0, torch.full_like(t, float("nan")), t / cnt).contiguous()

        P = {0: cov(0)}
        P_fo = []
        for f in names:
            i = fields.index(f)
            if i not in P:
                P[i] = cov(i)
            P_fo.append(P[i])
        gain = self.kalman_gain_tensor(y, R, localize, inflation * unbias, P[0], P_fo)
        var_o = torch.diagonal(P[0]).cpu().numpy() * unbias
        return {"gain": gain, "mean_o": m["mean"][0], "var_o": var_o, "observed": J, "members": int(n)}

    def _innovation_statistics(self, obs_name, obs, J, dist):
        """Mean and spread of ``obs_name`` across the members against ``obs`` at the observed cells J (two passes of the sums)."""
        m = self.moments((obs_name,), None, dist)[obs_name]
        innov = (obs - m["mean"])[J]
        return {"bias": float(np.mean(innov)) if J.any() else np.nan, "rmse": float(np.sqrt(np.mean(innov ** 2))) if J.any() else np.nan,
                "spread": float(np.sqrt(np.mean(m["var"][J]))) if J.any() else np.nan}

    def enkf(self, names, obs_name, obs, obs_var, method="denkf", localize=None, inflation=1.0, bounds=None, generator=None,
             dist=None, solver="host") -> dict:
        """One analysis step of an ensemble Kalman filter on the fields ``names`` (prognostic) from observations ``obs``
        [nlat] of ``obs_name`` (NaN: not observed) with error variance ``obs_var`` (scalar or [nlat]).  Built from the
        reductions and ONE write: means from ``reduced_sums``, P_oo and P_fo from ``covariance``, the gains on the host
        (``kalman_gains``: nlat^2 numbers leave the device, never a field), then ``update_columns`` moves every member on the
        device by G_f applied to its own innovation.  ``localize``: the half-width in x of the Gaspari-Cohn taper applied to
        both covariances by a Schur product (None: none) — possible because the update is in gain form, which a
        member-space transform could not do; ``inflation`` multiplies both covariances.
        ``method="denkf"`` (Sakov and Oke 2008, the deterministic filter): target = obs - mean_o / 2, scale = 1/2, no
        perturbation — the mean moves by the full gain, the anomalies by half of it.  ``method="perturbed"``: target = obs,
        scale = 1 and every member sees its own noisy copy of the observations, sqrt(obs_var) * randn drawn by torch on the
        device with ``generator``.
        With ``dist`` the sums and covariances are all-reduced, the gain is then the same on every rank, and each shard
        applies it to its own members: rank-local after the all-reduce, so a sharded update equals the unsharded one up to
        the cross-shard bound ``covariance`` states.
        Returns dict(gain_shape, observed (the number of observed cells), members, prior, posterior): ``prior`` and
        ``posterior`` hold bias, rmse and spread of ``obs_name`` against ``obs`` at the observed cells, from the ensemble sums
        before and after; ``posterior`` is None where ``obs_name`` is a diagnostic field, which the update leaves stale until
        the next diagnostic step.
        MIZ models: the update is linear algebra on Ei, Ew, h, D, phi and knows nothing of their meaning, so each field is
        bounded afterwards — by default Ei <= 0, Ew >= 0, h >= 0, 0 <= D <= Dmax, 0 <= phi <= 1 (``bounds``: dict name ->
        (lo, hi) replaces the default of that field).  Cross-field consistency — D = 0 where Ei = 0, the concentration that
        belongs to Ei and h, and so on — is restored only by the model's own step (src/miz.jl:109-117, 74-80), as after any
        ``set_field``.  Classic model (E, Tg): nothing to bound.
        ``solver="device"``: the gains are formed and solved on the device (``kalman_gains``) and handed to ``update_columns``
        as the tensor they are — an analysis step then moves O(nlat) numbers over the bus.  One shard only (ValueError with
        ``dist``)."""
        names = as_names(names)
        if method not in ("denkf", "perturbed"):
            raise ValueError(f"method = {method!r}: expected 'denkf' or 'perturbed'")
        y = np.asarray(obs, dtype=np.float64)
        k = self.kalman_gains(names, obs_name, y, obs_var, localize, inflation, dist, solver)
        J = k["observed"]
        prior = self._innovation_statistics(obs_name, y, J, dist)
        use = dict(self.default_update_bounds(names))
        use.update(bounds or {})
        use = {n: b for n, b in use.items() if n in names}
        if method == "denkf":
            self.update_columns(names, obs_name, k["gain"], y - 0.5 * k["mean_o"], 0.5, None, use)
        else:
            sd = np.where(J, np.sqrt(np.where(J, np.broadcast_to(np.asarray(obs_var, dtype=np.float64), y.shape), 0.0)), 0.0)
            self.update_columns(names, obs_name, k["gain"], y, 1.0, self.obs_noise(sd, generator), use)
        try:
            posterior = self._innovation_statistics(obs_name, y, J, dist)
        except StaleFieldError:
            posterior = None
        return {"gain_shape": tuple(k["gain"].shape), "observed": int(J.sum()), "members": k["members"], "prior": prior, "posterior": posterior}


class EnsembleRun(ColumnExchange, KalmanMixin):
    """``ncol`` independent columns of one model on one GPU (this rank's shard).

    ``init`` maps prognostic names to [ncol, nlat] arrays (or [nlat], broadcast to all
    columns); ``fcol`` is the per-column forcing offset; ``forcings`` a sequence of one Forcing
    per column, evaluated on the device at every step (hysteresis ensembles: every member its own
    ramp); ``member_params`` a sequence of one dict of parameter overrides over ``par`` per column
    (parameter sweeps: ``[{"D": d} for d in Ds]``, ebm_set_column_params) — member m gives the bits of a
    one-member run with ``par`` updated by ``member_params[m]``.  A sharded run passes ``member_params[mine]`` as it
    passes ``forcings[mine]``.

    A column's results do not depend on how many columns share its handle or on how the ensemble is sharded
    over GPUs: the launch geometry is a function of the latitude count and ``cells_per_thread`` only.

    ``noise``: per-member AR(1) forcing noise drawn on the device (ebm_set_column_noise), a dict with ``sigma`` (W m^-2,
    scalar or one per member), ``rho`` (lag-one-step autocorrelation) or ``tau`` (its e-folding time in years), and
    ``seed``.  Member m draws stream ``noise_streams[m]`` (default: m); a sharded run passes the global member indices
    of its shard, as it passes ``member_params[mine]``, and then gives the bits of the unsharded run."""

    has_noise = False

    def __init__(self, model, st, par, init, fcol=None, device=0, forcings=None, cells_per_thread=None,
                 member_params=None, noise=None, noise_streams=None):
        first = np.asarray(next(iter(init.values())))
        self.ncol = 1 if first.ndim == 1 else first.shape[0]
        if fcol is not None:
            self.ncol = len(fcol)
        if forcings is not None:
            self.ncol = len(forcings)
        rows = None
        if member_params is not None:
            rows = member_param_rows(member_params, par, init, fcol, forcings)
            self.ncol = rows.shape[0]
        noise_args = None
        if noise is not None:
            if not hasattr(noise, "items") or "sigma" not in noise or set(noise) - {"sigma", "rho", "tau", "seed"}:
                raise ValueError("noise: expected dict(sigma=..., rho=... or tau=..., seed=...)")
            noise_args = dict(sigma=noise["sigma"], rho=noise.get("rho"), tau=noise.get("tau"), seed=noise.get("seed", 0),
                              streams=None if noise_streams is None else np.asarray(noise_streams))
        elif noise_streams is not None:
            raise ValueError("noise_streams without noise")
        if noise_args is not None:
            check_noise_args(self.ncol, st.dt, **noise_args)     # before any device call
        self.st = st
        self.device = int(device)
        # cells_per_thread: launch option of ebm_create_ex (None = the library's default of 4).  Every rank of a
        # sharded run must pass the same value: the rounding of the solves depends on it and on nothing else
        self.engine = Engine(model, st.grid_kind, st.x, param_vector(par, default_parval), st.dt,
                             self.ncol, device, cells_per_thread=cells_per_thread)
        for k, v in init.items():
            a = np.asarray(v, dtype=np.float64)
            if a.ndim == 1:
                a = np.broadcast_to(a, (self.ncol, st.nx))
            self.engine.set_field(k, a)
        if fcol is not None:
            self.engine.set_column_forcing(fcol)
        self.engine.set_time_table(st.t)
        if forcings is not None:
            self.engine.set_column_schedules(forcings)
        if rows is not None:
            self.engine.set_column_params(rows)
        if noise_args is not None:
            self.engine.set_column_noise(**noise_args)
        self.has_schedules = forcings is not None
        self.has_noise = noise_args is not None
        self.step_index = 0

    def _forcing_table(self, forcing, first_step, nsteps):
        """The scalar forcing of global steps first_step .. first_step + nsteps - 1, evaluated at the middle of each step
        ([nsteps] float64; the bits of these times are part of the model time), or None without ``forcing``."""
        if forcing is None:
            return None
        T = (np.arange(first_step, first_step + nsteps) + 0.5) * self.st.dt
        return np.array([forcing(float(t)) for t in T])

    def _device_tensor(self, *shape):
        """An uninitialised float64 tensor of ``shape`` on this run's device."""
        import torch
        return torch.empty(shape, dtype=torch.float64, device=torch.device("cuda", self.device))

    def run(self, nsteps, forcing=None, diag_last=True, steps_per_launch=None):
        """Advance ``nsteps`` steps; ``forcing`` is a Forcing or None.  Nothing leaves the device between the
        steps of this call, so they are fused ``steps_per_launch`` to a launch (ebm_run_fused: the state stays in
        registers or LDS, bit-identical to one launch per step for every model and size); default 64, 1 = one
        launch per step (ebm_run)."""
        f = self._forcing_table(forcing, self.step_index, nsteps)
        self.engine.run(self.step_index, nsteps, f, diag_last, _steps_per_launch(steps_per_launch))
        self.step_index += nsteps

    def series(self, nsteps, every, names=("T", "phi"), forcing=None, steps_per_launch=None):
        """Advance ``nsteps`` steps like ``run`` (from ``step_index``, which advances; the scalar ``forcing`` evaluated as
        there) and return the time series of this shard's per-member hemispheric means (reference
        src/utilities.jl:397-403) of every field in ``names``, sampled on the device after every ``every`` steps
        (ebm_run_series): [len(names), nsteps // every, ncol].  Sample j is the state after ``every * (j + 1)`` steps of
        this call — a member's <T>(t) or ice area <phi>(t) at ``every * dt`` resolution, for crossing and residence times.
        Members are independent, so a sharded ensemble gives the bits of an unsharded one."""
        steps_per_launch = _steps_per_launch(steps_per_launch)
        self.engine.check_series_args(self.step_index, nsteps, every, names, None, steps_per_launch)    # before any device call
        f = self._forcing_table(forcing, self.step_index, nsteps)
        out = self.engine.run_series(self.step_index, nsteps, every, names, f, steps_per_launch)
        self.step_index += nsteps
        return out

    def first_passage(self, max_steps, every, name="T", level=0.0, direction="up", forcing=None, steps_per_launch=None):
        """Advance every member of this shard until the hemispheric mean of field ``name`` crosses the member's ``level``
        (ebm_run_until), tested on the device after every ``every`` steps, for at most ``max_steps`` steps (a multiple of
        ``every``).  ``direction``: "up" / +1 (mean >= level) or "down" / -1 (mean <= level); ``level`` and ``direction``
        are scalars or one entry per member; a NaN mean never crosses.  A member that has crossed takes no further step:
        its state is that of ``run`` over its own number of steps.  The scalar ``forcing`` is evaluated as in ``run``.
        Returns dict(step [ncol] int: the 0-based global step after which the member had crossed, -1 if it never did;
        time [ncol]: the model time of that step in years, NaN if never; crossed [ncol] bool; samples [ncol] int: the rounds
        taken; value [ncol]: the member's last mean).  Members are independent, so a sharded ensemble gives the results of
        an unsharded one; shards may stop at different rounds (no collective sits inside the call).  ``step_index``
        advances by the steps of this shard's slowest member; stepping on continues every member from its own state."""
        steps_per_launch = _steps_per_launch(steps_per_launch)
        if int(every) < 1:
            raise ValueError(f"every = {every}: the mean is tested every `every` >= 1 steps")
        if int(max_steps) < int(every) or int(max_steps) % int(every):
            raise ValueError(f"max_steps = {max_steps} is not a positive multiple of every = {every}")
        lev, d = passage_levels(self.ncol, level, direction)
        rounds = int(max_steps) // int(every)
        self.engine.check_until_args(self.step_index, rounds, every, name, lev, d, None, steps_per_launch)    # before any device call
        f = self._forcing_table(forcing, self.step_index, int(max_steps))
        first = self.step_index
        out = self.engine.run_until(first, rounds, every, name, lev, d, f, steps_per_launch)
        self.step_index += out["steps"]
        last = first + out["samples"] * int(every) - 1
        step = np.where(out["crossed"], last, -1)
        time = np.where(out["crossed"], (last + 0.5) * self.st.dt, np.nan)
        return dict(step=step, time=time, crossed=out["crossed"], samples=out["samples"], value=out["value"])

    def scalars(self, specs):
        """This shard's per-member column scalars (ebm_column_scalars), [len(specs), ncol]: band integrals and means and edge
        positions of the present state, reduced along each column on the device.  ``specs``: a sequence of ``scalar_spec``
        results.  Scalars are per member, so a sharded ensemble gives the bits of an unsharded one (no collective)."""
        return self.engine.column_scalars(specs)

    def ice_edge(self, level=0.15, name="phi"):
        """Each member's ice-edge position [ncol] in the grid's coordinate: walking poleward, where ``name`` first reaches
        ``level`` (linearly interpolated between the two cells); +Inf for a member without ice, x[0] for one that is covered
        to the equator."""
        return self.scalars([scalar_spec(self.st, "edge_ge", name, None, level)])[0]

    def scalar_series(self, nsteps, every, specs, forcing=None, steps_per_launch=None):
        """``series`` with the column scalars ``specs`` for a sample (ebm_run_series_scalars): [len(specs), nsteps // every,
        ncol], sample j what ``scalars`` would return after ``every * (j + 1)`` steps of this call.  ``step_index`` advances."""
        steps_per_launch = _steps_per_launch(steps_per_launch)
        self.engine.check_scalar_args(specs)                                                          # before any device call
        self.engine._check_sampling("scalar_series", self.step_index, nsteps, every, None, steps_per_launch)
        f = self._forcing_table(forcing, self.step_index, nsteps)
        out = self.engine.run_series_scalars(self.step_index, nsteps, every, specs, f, steps_per_launch)
        self.step_index += nsteps
        return out

    def first_passage_scalar(self, max_steps, every, spec, level, direction="up", forcing=None, steps_per_launch=None):
        """``first_passage`` on a column scalar (ebm_run_until_scalar): every member of this shard advances until its scalar
        ``spec`` (one ``scalar_spec``) crosses the member's ``level`` — its ice edge passes a latitude, its Arctic-band mean
        thickness reaches zero.  The +Inf of a member that has lost its ice crosses an upward test; a NaN never crosses.
        Arguments, result and ``step_index`` as ``first_passage``; ``value`` is the member's last scalar."""
        steps_per_launch = _steps_per_launch(steps_per_launch)
        if int(every) < 1:
            raise ValueError(f"every = {every}: the scalar is tested every `every` >= 1 steps")
        if int(max_steps) < int(every) or int(max_steps) % int(every):
            raise ValueError(f"max_steps = {max_steps} is not a positive multiple of every = {every}")
        lev, d = passage_levels(self.ncol, level, direction)
        rounds = int(max_steps) // int(every)
        self.engine.check_until_scalar_args(self.step_index, rounds, every, spec, lev, d, None, steps_per_launch)   # before any device call
        f = self._forcing_table(forcing, self.step_index, int(max_steps))
        first = self.step_index
        out = self.engine.run_until_scalar(first, rounds, every, spec, lev, d, f, steps_per_launch)
        self.step_index += out["steps"]
        last = first + out["samples"] * int(every) - 1
        step = np.where(out["crossed"], last, -1)
        time = np.where(out["crossed"], (last + 0.5) * self.st.dt, np.nan)
        return dict(step=step, time=time, crossed=out["crossed"], samples=out["samples"], value=out["value"])

    def resample(self, parents):
        """Selection step of a cloning / splitting / particle-filter algorithm, on the device (ebm_resample_columns):
        member c of this shard continues from a copy of member ``parents[c]``'s state — fields, warm start, noise state —
        and keeps its own forcing offset, schedule, parameter row and noise stream, so it draws its own noise from the
        next step on.  ``parents``: [ncol] integer indices WITHIN THIS SHARD (``selection_parents`` makes them from
        weights).  ``step_index`` is unchanged; no field becomes stale.  The call is rank-local: a parent on another
        rank's shard cannot be named here — ``resample_global`` selects across ranks, by the packed device export and
        import of whole columns (``export_tensor`` / ``import_tensor``: ebm_export_columns / ebm_import_columns) as the
        payload of an all-to-all between the shards."""
        self.engine.resample_columns(parents)

    def export_tensor(self, cols):
        """The state of the members ``cols`` of this shard (indices may repeat) as ``(records, mask)``: a float64 device
        tensor [len(cols), R], record i the packed state of member cols[i] (ebm_export_columns: every field in the natural
        layout, the warm start, N_c), and the mask of the fields that travel.  Nothing in the run changes.  The handle is
        synchronised before the tensor is returned: it is complete and any stream may read it."""
        c, _ = self.engine.check_exchange_args(cols, 16)
        R, _ = self.engine.column_record()
        out = self._device_tensor(len(c), R)
        mask = self.engine.export_columns(c, out.data_ptr() if len(c) else 0)
        self.engine.sync()
        return out, mask

    def import_tensor(self, cols, tensor, mask, records=None):
        """Member ``cols[i]`` of this shard (distinct) continues from record ``records[i]`` (default i) of ``tensor``, a
        float64 tensor [m, R] on this run's device as ``export_tensor`` of a run of the same model and shape returns it,
        with that export's ``mask`` (ebm_import_columns).  The member keeps its own settings and noise stream;
        ``step_index`` is unchanged.  torch's current stream is synchronised before the call (whatever filled the tensor has
        ended) and the handle after it (the tensor may be reused)."""
        import torch
        R, _ = self.engine.column_record()
        if not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float64 or tensor.dim() != 2 or tensor.shape[1] != R:
            raise ValueError(f"tensor: expected a float64 tensor [m, {R}], got {getattr(tensor, 'dtype', type(tensor).__name__)} "
                             f"{tuple(getattr(tensor, 'shape', ()))}")
        if tensor.device != torch.device("cuda", self.device) or not tensor.is_contiguous():
            raise ValueError(f"tensor: expected a contiguous tensor on cuda:{self.device}, got one on {tensor.device}")
        c, r = self.engine.check_exchange_args(cols, 16, records, mask, distinct=True)
        top = int(r.max()) + 1 if r is not None and len(r) else (len(c) if r is None else 0)
        if top > tensor.shape[0]:
            raise ValueError(f"tensor holds {tensor.shape[0]} records, but record {top - 1} is asked for")
        if len(c) == 0:
            return
        torch.cuda.current_stream(self.device).synchronize()
        self.engine.import_columns(c, tensor.data_ptr(), mask, r)
        self.engine.sync()

    def seasonal_means(self, years, names=("T", "phi"), forcing=None):
        """Integrate ``years`` whole years from the current state and return, per column, the
        hemispheric means (reference src/utilities.jl:397-403) of the winter snapshot, the summer
        snapshot and the annual mean of every variable in ``names`` for every year — reduced on the
        device (ebm_integrate_hemispheric): dict(winter, summer, avg), each [len(names), years, ncol].
        This is the data behind the reference's hysteresis plot (src/plot.jl:173-225: hemispheric_mean
        of seasonal.avg.T[year] against 2*pi*hemispheric_mean of seasonal.{avg,winter,summer}.phi[year])
        for every member, at O(members x years) bytes of I/O.  Model time — the scalar ``forcing`` and the
        per-column Forcing schedules — continues from the steps this run has already taken, so a ramp integrated
        in several calls (chunks of years) equals the same ramp integrated in one; the calls must start at a
        year boundary, as the reference's ``integrate`` does."""
        st = self.st
        if self.step_index % st.nt:
            raise ValueError(f"seasonal_means starts a year: {self.step_index} steps taken so far is not a multiple of nt = {st.nt}")
        f = self._forcing_table(forcing, self.step_index, st.nt * years)
        self.engine.set_step_clock(self.step_index)
        out = self.engine.integrate_hemispheric(st.nt, years, f, st.winter.inx, st.summer.inx, tuple(names))
        self.step_index += st.nt * years
        return out

    def equilibrate(self, max_years, tol=None, forcing=None, min_years=2):
        """Spin this shard's members up until each one's seasonal cycle repeats (ebm_equilibrate): whole years from the
        current state, member m stopping at the first year y >= max(2, min_years) whose year-end fields named in ``tol``
        (dict name -> absolute tolerance, default ``{"T": 1e-3}``) differ from the previous year's by at most the
        tolerance everywhere, or at ``max_years``.  ``forcing``: a constant Forcing (or None) added to every member's
        ``fcol``; ramps have no equilibrium and are refused, as are ensembles built with ``forcings=``.  Members are
        independent, so a sharded ensemble gives the bits of an unsharded one.  The call starts a year, like
        ``seasonal_means``; afterwards ``step_index`` is that of the slowest member.  Returns dict(years, converged,
        resid) as ``Engine.equilibrate``."""
        st = self.st
        if self.has_schedules:
            raise ValueError("equilibrate: this ensemble was built with forcings= (per-member ramps have no equilibrium)")
        if self.has_noise:
            raise ValueError("equilibrate: this ensemble was built with noise= (a noisy member has no repeating cycle)")
        if forcing is not None and not getattr(forcing, "constant", False):
            raise ValueError("equilibrate: needs a constant forcing (a Forcing{false} ramp has no equilibrium)")
        if self.step_index % st.nt:
            raise ValueError(f"equilibrate starts a year: {self.step_index} steps taken so far is not a multiple of nt = {st.nt}")
        tol = {"T": 1e-3} if tol is None else tol
        f = self._forcing_table(forcing, self.step_index, st.nt)
        self.engine.check_equilibrate_args(st.nt, max_years, tol, min_years, f)
        self.engine.set_step_clock(self.step_index)
        out = self.engine.equilibrate(st.nt, max_years, f, tol, min_years)
        self.step_index += st.nt * int(out["years"].max())
        return out

    def state(self, names=None):
        return self.engine.get_state(names)

    def hemispheric_mean_tensor(self, name):
        """Per-column hemispheric mean (reference src/utilities.jl:397-403) as a torch tensor ON THE
        DEVICE — reduced there by ebm_hemispheric_mean_device, never staged through the host — ready
        to be gathered over RCCL (gather_columns)."""
        out = self._device_tensor(self.ncol)
        self.engine.hemispheric_mean_device(name, out.data_ptr())
        return out

    def _reduced_tensor(self, names, nslots, device_call):
        """A float64 tensor [len(names), nslots, nlat] on this run's device, filled by ``device_call(its address)``."""
        out = self._device_tensor(len(as_names(names)), nslots, self.st.nx)
        device_call(out.data_ptr())
        return out

    def ensemble_sums(self, names, weights=None, center=None):
        """This shard's weighted sums across its members, per latitude (ebm_ensemble_sums): ndarray [len(names), 3, nlat] of
        S0, S1, S2, reduced on the device.  See ``Engine.ensemble_sums``; ``moments`` turns them into mean and variance."""
        return self.engine.ensemble_sums(names, weights, center)

    def ensemble_sums_tensor(self, names, weights=None, center=None):
        """The same sums as a float64 torch tensor [len(names), 3, nlat] ON THE DEVICE — written there by
        ebm_ensemble_sums_device, never staged through the host — ready to be all-reduced over RCCL (``reduced_sums``)."""
        return self._reduced_tensor(names, 3, lambda ptr: self.engine.ensemble_sums_device(names, ptr, weights, center))

    def ensemble_range(self, names, weights=None):
        """This shard's count, minimum and maximum across its members, per latitude (ebm_ensemble_range): ndarray
        [len(names), 3, nlat].  See ``Engine.ensemble_range``; ``range`` combines the shards."""
        return self.engine.ensemble_range(names, weights)

    def ensemble_range_tensor(self, names, weights=None):
        """The same as a float64 torch tensor ON THE DEVICE (ebm_ensemble_range_device), ready for RCCL."""
        return self._reduced_tensor(names, 3, lambda ptr: self.engine.ensemble_range_device(names, ptr, weights))

    def ensemble_histogram(self, names, lo, hi, nbins, weights=None):
        """This shard's weighted histogram across its members, per latitude (ebm_ensemble_histogram): ndarray [len(names),
        nbins + 2, nlat].  See ``Engine.ensemble_histogram``; ``histogram`` adds the shards, ``quantiles`` brackets with it."""
        return self.engine.ensemble_histogram(names, lo, hi, nbins, weights)

    def ensemble_histogram_tensor(self, names, lo, hi, nbins, weights=None):
        """The same as a float64 torch tensor ON THE DEVICE (ebm_ensemble_histogram_device), ready for RCCL."""
        return self._reduced_tensor(names, int(nbins) + 2, lambda ptr: self.engine.ensemble_histogram_device(names, lo, hi, nbins, ptr, weights))

    def ensemble_covariance(self, name_a, name_b=None, weights=None, center_a=None, center_b=None):
        """This shard's matrix of sums across its members for every pair of latitudes (ebm_ensemble_covariance): ndarray
        [nlat, nlat].  See ``Engine.ensemble_covariance``; ``covariance`` centres it on the ensemble means and ``eofs``
        diagonalises it."""
        return self.engine.ensemble_covariance(name_a, name_b, weights, center_a, center_b)

    def ensemble_covariance_tensor(self, name_a, name_b=None, weights=None, center_a=None, center_b=None):
        """The same as a float64 torch tensor [nlat, nlat] ON THE DEVICE (ebm_ensemble_covariance_device), ready to be
        all-reduced over RCCL."""
        out = self._device_tensor(self.st.nx, self.st.nx)
        self.engine.ensemble_covariance_device(name_a, name_b, weights, center_a, center_b, out.data_ptr())
        return out

    def misfits(self, names, targets, rweights=None):
        """This shard's per-member misfits to the target profiles (ebm_column_misfits): ndarray [ntargets, 2, ncol] of J and
        the number N of cells behind it, reduced along each member's column on the device.  See ``Engine.column_misfits``."""
        return self.engine.column_misfits(names, targets, rweights)

    def misfits_tensor(self, names, targets, rweights=None):
        """The same as a float64 torch tensor [ntargets, 2, ncol] ON THE DEVICE (ebm_column_misfits_device), ready to be
        all-gathered over RCCL."""
        y = np.asarray(targets, dtype=np.float64)
        out = self._device_tensor(1 if y.ndim == 2 else y.shape[0], 2, self.ncol)
        self.engine.column_misfits_device(names, targets, out.data_ptr(), rweights)
        return out

    def assimilate(self, names, obs, obs_var, rng, quad=None, ess_fraction=0.5, dist=None):
        """One observation step of a bootstrap particle filter.  ``obs`` [len(names), nlat]: the observed profiles, NaN where
        nothing was observed; ``obs_var``: the observation error variance, a scalar or [len(names), nlat], > 0; ``quad``: None
        or quadrature weights [nlat] / [len(names), nlat] >= 0 (0 masks a latitude out).  The misfit J_m = sum quad / obs_var *
        (x - obs)^2 of every member is reduced on the device (``misfits`` with rweights = quad / obs_var), the weights are
        ``assimilation_weights(J)`` over ALL members — with ``dist`` the O(members) values of J and N are all-gathered in rank
        order first — and when the effective sample size falls below ``ess_fraction`` * n the ensemble is resampled:
        ``selection_parents(weights, rng)``, then ``resample`` (``resample_global`` with ``dist``; every rank must pass a
        ``rng`` in the same state, so that all draw the same parents).  Returns dict(J [n], N [n], weights [n], ess,
        log_evidence, parents [n] or None if nothing was resampled), n the members of the whole ensemble."""
        obs_var = np.asarray(obs_var, dtype=np.float64)
        if not (np.isfinite(obs_var) & (obs_var > 0.0)).all():
            raise ValueError("obs_var: expected finite values > 0")
        if not 0.0 <= float(ess_fraction) <= 1.0:
            raise ValueError(f"ess_fraction = {ess_fraction}: expected a fraction between 0 and 1")
        shape = (len(as_names(names)), self.st.nx)
        rw = np.ascontiguousarray(np.broadcast_to((1.0 if quad is None else np.asarray(quad, dtype=np.float64)) / obs_var, shape))
        out = self.misfits(names, np.asarray(obs, dtype=np.float64).reshape(shape), rw)
        sharded = _sharded(dist)
        if sharded:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, out[0])
            out = np.concatenate(parts, axis=1)[None]
        J, N = out[0, 0], out[0, 1]
        res = assimilation_weights(J)
        parents = None
        if res["ess"] < float(ess_fraction) * J.shape[0]:
            parents = selection_parents(res["weights"], rng)
            if sharded:
                self.resample_global(parents, J.shape[0], dist)
            else:
                self.resample(parents)
        return dict(J=J, N=N, weights=res["weights"], ess=res["ess"], log_evidence=res["log_evidence"], parents=parents)

    def update_columns(self, names, obs_name, gain, target, scale=1.0, perturb=None, bounds=None):
        """Every member moved by ``gain`` applied to its own innovation, on the device (ebm_update_columns).  See
        ``Engine.update_columns``; ``enkf`` forms the gain."""
        self.engine.update_columns(names, obs_name, gain, target, scale, perturb, bounds)

    def kalman_gain_tensor(self, obs, obs_var, localize, factor, P_oo, P_fo):
        """The Kalman gains [len(P_fo), nlat, nlat] as a torch tensor ON THE DEVICE from covariances already there
        (ebm_kalman_gain_device).  See ``Engine.kalman_gain_tensor``; ``kalman_gains(solver="device")`` feeds it."""
        return self.engine.kalman_gain_tensor(obs, obs_var, localize, factor, P_oo, P_fo)

    def obs_noise(self, sd, generator=None):
        """[ncol, nlat] float64 on this run's device: sd[j] * randn, drawn by torch with ``generator`` (a torch.Generator of
        that device, or None for the default one)."""
        import torch
        dev = torch.device("cuda", self.device)
        e = torch.randn((self.ncol, self.st.nx), dtype=torch.float64, device=dev, generator=generator)
        return (e * torch.as_tensor(np.ascontiguousarray(sd, dtype=np.float64), device=dev)).contiguous()

    def default_update_bounds(self, names) -> dict:
        """MIZ: Ei <= 0, Ew >= 0, h >= 0, 0 <= D <= Dmax (of the parameters the run was created with), 0 <= phi <= 1."""
        if not self.engine.model.startswith("MIZ"):
            return {}
        dmax = float(self.engine.params[PARAM_ORDER.index("Dmax")])
        return {n: tuple(dmax if b == "Dmax" else b for b in MIZ_UPDATE_BOUNDS[n]) for n in names if n in MIZ_UPDATE_BOUNDS}

    def field_tensor(self, name):
        """A packed [ncol, nlat] device tensor copy of a field (device-to-device)."""
        out = self._device_tensor(self.ncol, self.st.nx)
        self.engine.get_field_device(name, out.data_ptr())
        return out

    def close(self):
        self.engine.close()


def broadcast_inputs(arrays: dict | None, dist=None, device=None, src: int = 0) -> dict:
    """Broadcast the run's small inputs — ``st.x``, the parameter vector, the per-step forcing
    table, the per-column forcing offsets — from rank ``src`` to every rank (I/O only, a few KB;
    SURVEY §8(e)).  ``arrays`` maps names to fp64 arrays on ``src`` and is ignored elsewhere;
    every rank returns the same dict.  With dist=None (single process) returns ``arrays``."""
    if not _sharded(dist):
        return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in (arrays or {}).items()}
    import torch
    rank = dist.get_rank()
    meta = [None]
    if rank == src:
        arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
        meta = [[(k, v.shape) for k, v in arrays.items()]]
    dist.broadcast_object_list(meta, src=src)                 # names and shapes (host side)
    total = sum(int(np.prod(shape)) for _, shape in meta[0])
    flat = np.concatenate([arrays[k].ravel() for k, _ in meta[0]]) if rank == src else np.empty(total)
    t = torch.from_numpy(flat)
    if device is not None:
        t = t.to(device)
    dist.broadcast(t, src=src)                                # one message for all payloads
    flat = t.cpu().numpy()
    out, pos = {}, 0
    for k, shape in meta[0]:
        n = int(np.prod(shape))
        out[k] = flat[pos:pos + n].reshape(shape).copy()
        pos += n
    return out


def gather_columns(local, ncol_total: int, dist=None, device=None, dst: int = 0):
    """Gather per-column data ([ncol_local, ...]) from all ranks to rank ``dst`` (I/O only).

    ``local`` is a NumPy array or a torch tensor.  With the "nccl" backend (= RCCL on ROCm) the
    payload stays on the device end to end: a device tensor (e.g. from
    ``EnsembleRun.hemispheric_mean_tensor`` / ``field_tensor``) is gathered with ``dist.gather`` —
    point-to-point sends to ``dst`` only, 1/world_size of an all-gather's traffic — and copied to the
    host once, on ``dst``.  With "gloo" (CPU tests) host tensors are gathered.  Returns the
    [ncol_total, ...] NumPy array on ``dst`` and None elsewhere.  With dist=None (single process)
    returns ``local`` as a NumPy array."""
    if not _sharded(dist):
        return local.cpu().numpy() if hasattr(local, "cpu") else local
    import torch
    ws, rank = dist.get_world_size(), dist.get_rank()
    t = local if isinstance(local, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(local, dtype=np.float64))
    if _backend(dist) == "nccl":
        if t.device.type == "cpu":
            t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    else:
        t = t.cpu()
    width = -(-ncol_total // ws)                      # block sizes differ by at most one column: pad
    if t.shape[0] < width:
        t = torch.cat([t, torch.zeros((width - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)])
    t = t.contiguous()
    outs = [torch.empty_like(t) for _ in range(ws)] if rank == dst else None
    dist.gather(t, outs, dst=dst)
    if rank != dst:
        return None
    parts = []
    for r in range(ws):
        sl = shard_columns(ncol_total, ws, r)
        parts.append(outs[r][: sl.stop - sl.start])
    return torch.cat(parts, dim=0).cpu().numpy()
