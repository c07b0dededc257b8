"""GPU tests (-m gpu) of the column scalars (include/ebm_hip.h: ebm_column_scalars, ebm_run_series_scalars,
ebm_run_until_scalar), bit for bit against the NumPy restatement tests/column_scalars_ref.py (checked on the CPU by
tests/test_host_column_scalars.py) and against identities with entry points the library already has.

Reduction cases: fields the test sets itself (so the reference reads the very arrays the device holds): the mid-year state
of support.midyear_state with, per column, a crafted phi — as it is, ice-free, ice-covered, and a first hit in lane 0, lane
63, the first cell of the second 64 and of the second 256-cell tile — and Ti / Tw with NaN sentinels.  nlat 2, 3, 65, 130,
kMeanTile + 2 = 514 (two tiles of the mean walk) and 4096 x 3 columns; both cells_per_thread where they exist; MIZ and
classic.  Twelve scalars in one call, a field repeated; bands from 0, to nlat-1, interior, of two cells, of one cell (edges).
Stepping cases: series on 70 columns under noise against fresh ebm_run_fused runs; first passage on an edge under a ramp with
per-member offsets against the series-derived answer (first_crossing, tests/test_host_until.py); ebm_run_series and
ebm_run_until unchanged by scalar calls before them."""
import numpy as np
import pytest

import column_scalars_ref as ref
from support import (assert_same_bits, assert_same_snapshot, assert_snapshot_by_column, forcing_of, is_miz, make_engine, midyear_state,
                     same_bits, snapshot)
from test_host_until import first_crossing

pytestmark = pytest.mark.gpu

MEAN_TILE = 512                                 # kMeanTile (csrc/ebm_internal.h)
ICE = 0.15


def bare(pkg, model, grid, nlat, ncol, cells):
    """A handle of any meridian length that is only read: no time table, no stepping."""
    st = pkg.SpaceTime(grid, nlat, 2000, 1)
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ" if is_miz(model) else "Classic"), pkg.default_parval)
    return pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, ncol, device=0, cells_per_thread=cells), st


def crafted_fields(model, st, ncol):
    """name -> [ncol, nlat], every field the specs below name."""
    nlat = len(st.x)
    rng = np.random.default_rng(nlat)
    base = midyear_state(model, st, ncol)
    k = np.arange(nlat)
    if not is_miz(model):
        out = {n: base[n].copy() for n in ("E", "Tg")}
        out["T"] = rng.normal(size=(ncol, nlat)) * 20.0
        out["h"] = np.where(k[None, :] >= nlat // 2 + (np.arange(ncol) % 3)[:, None], 1.5, 0.0) * rng.uniform(0.5, 1.0, (ncol, nlat))
        return out
    out = {n: base[n].copy() for n in ("Ei", "Ew", "h", "D", "phi")}
    phi = out["phi"]
    phi[1 % ncol] = 0.0                                                       # ice-free
    if ncol > 2:
        phi[2] = 1.0                                                          # ice-covered: the hit is at k0 of every band
    for c, first in zip(range(3, ncol), (0, 63, 64, 256, nlat - 1)):          # the first cell at ICE, to the bit
        first = min(first, nlat - 1)
        phi[c] = np.where(k >= first, np.minimum(1.0, ICE + 0.05 * (k - first)), 0.1 * ICE * rng.uniform(size=nlat))
    out["T"] = rng.normal(size=(ncol, nlat)) * 20.0
    for name in ("Ti", "Tw"):
        f = rng.normal(size=(ncol, nlat)) * 5.0
        f[0] = np.where(phi[0] > 0.0, f[0], np.nan) if name == "Ti" else np.where(phi[0] < 1.0, f[0], np.nan)
        f[ncol - 1, nlat // 2] = np.nan
        out[name] = f
    return out


def specs_for(model, nlat):
    """Twelve scalars, the fields repeated."""
    last, mid = nlat - 1, nlat // 2
    a, b = min(1, last), max(min(1, last), last - 1)                          # an interior band where there is one
    ice, temp, third = ("phi", "T", "Ti") if is_miz(model) else ("h", "T", "Tg")
    want = [("integral", temp, 0, last), ("mean", temp, 0, max(1, mid)), ("mean", temp, min(mid, last - 1), last),
            ("integral", temp, a, b) if a < b else ("integral", temp, 0, last), ("mean", ice, mid if mid < last else 0, min(mid + 1, last)),
            ("integral", third, 0, last), ("edge_ge", ice, 0, last, ICE), ("edge_ge", ice, a, b, ICE),
            ("edge_le", temp, 0, last, -10.0), ("edge_ge", ice, mid, mid, ICE), ("edge_le", ice, min(2, last), last, 0.5),
            ("edge_ge", third, 0, last, 1.0)]
    assert len(want) == 12
    return want


SHAPES = [("MIZ", "sin", n, c) for n in (2, 3, 65, 130, MEAN_TILE + 2) for c in (4, 2)] + \
         [("MIZ", "identity", 130, 4), ("MIZ", "sin", 4096, 4), ("Classic", "identity", 65, 4), ("Classic", "identity", MEAN_TILE + 2, 2)]


@pytest.mark.parametrize("model,grid,nlat,cells", SHAPES, ids=lambda v: str(v))
def test_scalars_are_the_restatement_bit_for_bit(pkg, model, grid, nlat, cells):
    import torch
    ncol = 3 if nlat == 4096 else 8
    eng, st = bare(pkg, model, grid, nlat, ncol, cells)
    fields = crafted_fields(model, st, ncol)
    for name, f in fields.items():
        eng.set_field(name, f)
    specs = specs_for(model, nlat)
    before = (eng.counters(), eng.field_step(specs[0][1]))
    got = eng.column_scalars(specs)
    want = ref.column_scalars(fields, st.x, specs)
    for s, one in enumerate(specs):
        assert same_bits(got[s], want[s]), (one, got[s], want[s])
    assert (eng.counters(), eng.field_step(specs[0][1])) == before
    # the anchor: the full-range integral IS ebm_hemispheric_mean
    assert same_bits(got[0], eng.hemispheric_mean(specs[0][1]))
    if is_miz(model):
        assert np.isnan(got[5]).any() and np.isinf(got[6][1]) and got[6][2] == st.x[0]      # NaN sentinel, ice-free, ice-covered
    # one scalar alone, and the device variant
    assert same_bits(eng.column_scalars(specs[6:7])[0], want[6])
    dev = torch.full((len(specs), ncol), -1.0, dtype=torch.float64, device="cuda:0")
    eng.column_scalars_device(specs, dev.data_ptr())
    assert same_bits(dev.cpu().numpy(), want)
    eng.close()


def test_stale_field_phi_derived_and_conversions(pkg):
    mk = lambda: make_engine(pkg, "MIZ", "sin", 65, 5, cells=4)[0]
    eng, st = make_engine(pkg, "MIZ", "sin", 65, 5, cells=4)
    twin = mk()
    eng.run(0, 3, forcing_of(0, 3), False, 1)                # state-only one-step launches: T is stale, phi underived
    twin.run(0, 3, forcing_of(0, 3), False, 1)
    before = (eng.counters(), eng.state_conversions(), {k: eng.field_step(k) for k in ("T", "phi")})
    with pytest.raises(pkg.StaleFieldError, match="field T is stale") as err:
        eng.column_scalars([("edge_ge", "phi", 0, 64, ICE), ("mean", "T", 0, 64)])
    assert err.value.status == -5
    assert (eng.counters(), eng.state_conversions(), {k: eng.field_step(k) for k in ("T", "phi")}) == before
    specs = [("edge_ge", "phi", 0, 64, ICE), ("integral", "phi", 0, 64), ("mean", "h", 40, 64)]
    got = eng.column_scalars(specs)
    mean = twin.hemispheric_mean("phi")
    assert eng.state_conversions() == twin.state_conversions()               # counted as ebm_hemispheric_mean counts
    assert eng.counters() == before[0] and eng.field_step("phi") == before[2]["phi"]
    assert same_bits(got[1], mean)
    fused = mk()
    fused.run(0, 3, forcing_of(0, 3), False, 3)              # the fused kernel stores phi
    want = ref.column_scalars({k: fused.get_field(k) for k in ("phi", "h")}, st.x, specs)
    assert_same_bits(got, want)
    for e in (eng, twin, fused):
        e.close()


SERIES_SPECS = [("edge_ge", "phi", 0, 64, ICE), ("mean", "T", 0, 64), ("integral", "phi", 30, 64), ("mean", "h", 40, 64),
                ("edge_le", "T", 0, 64, -5.0)]


def test_series_samples_and_state(pkg):
    ncol, every, ns, K = 70, 4, 3, 3
    mk = lambda: make_engine(pkg, "MIZ", "sin", 65, ncol, what=("noise",))[0]
    f = forcing_of(0, every * ns)
    eng = mk()
    got = eng.run_series_scalars(0, every * ns, every, SERIES_SPECS, f, K)
    assert got.shape == (len(SERIES_SPECS), ns, ncol)
    for j in range(ns):
        fresh = mk()
        fresh.run(0, (j + 1) * every, f[:(j + 1) * every], True, K)
        assert_same_bits(got[:, j, :], fresh.column_scalars(SERIES_SPECS), f"sample {j}")
        fresh.close()
    plain = mk()
    plain.run_series(0, every * ns, every, ("T", "phi"), f, K)
    assert_same_snapshot(snapshot(eng, "MIZ"), snapshot(plain, "MIZ"), "after the series")
    eng.close()
    plain.close()


def test_first_passage_on_the_ice_edge(pkg):
    ncol, every, ns, K = 70, 5, 6, 4
    spec = ("edge_ge", "phi", 0, 64, ICE)
    hot = np.arange(ncol - 4, ncol)                          # open water but for a little ice in the polar cell, under a strong
    ice = np.array([0.3, 0.8, 1.5, 3.0])                     # forcing: it melts on the way and the edge becomes +Inf

    def mk():
        eng, st = make_engine(pkg, "MIZ", "sin", 65, ncol, what=("sched",))
        state = midyear_state("MIZ", st, ncol)
        Lf = pkg.default_parameters("MIZ")["Lf"]
        for k in ("Ei", "h", "D", "phi"):
            state[k][hot] = 0.0
        state["Ei"][hot, -1], state["h"][hot, -1] = -ice, ice / Lf
        state["D"][hot, -1], state["phi"][hot, -1] = 10.0, 1.0
        eng.set_state(state)
        fcol = np.linspace(-1.5, 1.5, ncol)
        fcol[hot] = 400.0                                    # (the mid-year pole loses about 190 W m^-2: less would freeze)
        eng.set_column_forcing(fcol)
        return eng
    f = forcing_of(0, every * ns)
    ser = mk()
    m = ser.run_series_scalars(0, every * ns, every, [spec], f, K)[0]        # [ns, ncol]
    ser.close()
    # levels from the measured series: the running maximum up to a target sample (an equality at the bit), never, first
    level, direc = np.empty(ncol), np.ones(ncol, dtype=np.int64)
    for c in range(ncol):
        level[c] = np.max(m[:1 + c % ns, c])
    level[1], direc[1] = -np.inf, -1                         # never: no edge is <= -inf
    level[hot] = np.inf                                      # only "no edge in the band" crosses
    samples, crossed, value = first_crossing(m, level, direc)
    assert len(set(samples[crossed].tolist())) >= 3 and not crossed[1] and samples[1] == ns, "honesty: several rounds, one never"
    lost = np.isfinite(m[0, hot]) & crossed[hot] & np.isinf(value[hot]) & (samples[hot] > 1)
    assert lost.any(), ("honesty: a member has an edge at the first sample and has lost its ice at a later one", m[:, hot])
    eng = mk()
    out = eng.run_until_scalar(0, ns, every, spec, level, direc, f, K)
    assert np.array_equal(out["samples"], samples) and np.array_equal(out["crossed"], crossed)
    assert same_bits(out["value"], value)
    R = int(samples.max())
    c = eng.counters()
    assert c["steps"] == R * every
    assert c["launches"] == sum(-(-every // K) for j in range(1, R + 1) if (samples >= j).any())     # one chain at 65 cells
    eng.run(R * every, 1, None, True, 1)                     # a diagnostic step: every field readable
    got = snapshot(eng, "MIZ")
    for s in sorted(set(samples.tolist())):
        want_eng = mk()
        want_eng.run(0, s * every, f[:s * every], False, K)
        want_eng.run(R * every, 1, None, True, 1)
        want = snapshot(want_eng, "MIZ")
        cols = np.flatnonzero(samples == s)
        for k in want["fields"]:
            assert same_bits(got["fields"][k][cols], want["fields"][k][cols]), (s, k)
        assert same_bits(got["noise"][cols], want["noise"][cols])
        want_eng.close()
    eng.close()


def test_series_and_until_are_unchanged_by_scalar_calls(pkg):
    ncol, every, ns, K = 70, 4, 3, 3
    mk = lambda: make_engine(pkg, "MIZ", "sin", 65, ncol, what=("noise",))[0]
    f = forcing_of(0, 2 * every * ns)
    level, direc = np.linspace(-2.0, 6.0, ncol), np.where(np.arange(ncol) % 2, 1, -1)
    plain, mixed = mk(), mk()
    a = plain.run_series(0, every * ns, every, ("T", "phi"), f[:every * ns], K)
    mixed.column_scalars(SERIES_SPECS[:1])
    b = mixed.run_series(0, every * ns, every, ("T", "phi"), f[:every * ns], K)
    assert_same_bits(a, b)
    ua = plain.run_until(every * ns, ns, every, "T", level, direc, f[every * ns:], K)
    mixed.column_scalars(SERIES_SPECS)
    ub = mixed.run_until(every * ns, ns, every, "T", level, direc, f[every * ns:], K)
    assert np.array_equal(ua["samples"], ub["samples"]) and np.array_equal(ua["crossed"], ub["crossed"]) and same_bits(ua["value"], ub["value"])
    assert len(set(ua["samples"].tolist())) >= 2
    assert_snapshot_by_column(snapshot(mixed, "MIZ"), snapshot(plain, "MIZ"), "after series and until")
    plain.close()
    mixed.close()
