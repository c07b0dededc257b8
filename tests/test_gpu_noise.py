"""GPU tests (-m gpu) of the per-column forcing noise (ebm_set_column_noise; the definition is in include/ebm_hip.h).

The generator is pinned by ebm_noise_innovations against the host restatement (energybalancemodel.jl_amd/noise.py, whose
Philox words the CPU tests pin to the published answers).  The stepping is pinned bit for bit against the path that
exists without noise: a noise-free handle stepped one step at a time with ebm_set_column_forcing(N(n)), N(n) computed on
the host from the device's innovations with the exact recurrence — f + N is the same sum in both.
"""
import math

import numpy as np
import pytest

from conftest import load_golden
from support import (MIZ_PROG as PROG, all_fields as names, assert_same_values as assert_same, host_N, is_miz, noise_args,
                     noise_module as _noise)

pytestmark = pytest.mark.gpu

MIZ_ALL = names("MIZ")
NLAT, NT = 180, 2000
FIRST = 1000                     # global index of the first step: mid-year, a live T0 solve


def initial_state(st, model, ncol):
    """Interpolated field by field: not support.midyear_state, whose nearest-cell values are other numbers."""
    if is_miz(model):
        g = load_golden("miz_sin_180_2000.npz")
        return {k: np.tile(np.interp(st.x, g["x"], g[f"s1000_{k}"]), (ncol, 1)) for k in PROG + ("T0",)}
    g = load_golden("classic_identity_180_2000.npz")
    return {k: np.tile(np.interp(st.x, g["x"], g[f"s522_{k}"]), (ncol, 1)) for k in ("E", "Tg")}


def spacetime(pkg, model):
    return pkg.SpaceTime("sin" if is_miz(model) else "identity", NLAT, NT, 1)


def make(pkg, model, ncol, state=None, params=None, **opt):
    st = spacetime(pkg, model)
    par = pkg.default_parameters("Classic" if model == "Classic" else "MIZ")
    vec = pkg.engine.param_vector(par, pkg.default_parval) if params is None else params
    eng = pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, ncol, device=0, **opt)
    eng.set_state(initial_state(st, model, ncol) if state is None else state)
    eng.set_time_table(st.t)
    eng.set_step_clock(FIRST)
    return st, eng


def forcing(nsteps):
    return 0.5 * np.sin(np.arange(nsteps) * 0.37)


def reference(pkg, model, ncol, nsteps, f, N, **opt):
    """A noise-free handle stepped one step at a time with the column forcing N(n): the state after the last step."""
    st, ref = make(pkg, model, ncol, **opt)
    with ref:
        for i in range(nsteps):
            ref.set_column_forcing(N[:, i])
            ref.run(FIRST + i, 1, f[i:i + 1], diag_last=(i == nsteps - 1))
        return ref.get_state(names(model))


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---- generator ---------------------------------------------------------------------------------------------------------

def test_innovations_match_the_host_restatement(pkg):
    nz = _noise(pkg)
    ncol = 64
    streams = np.array([0, 1, 2, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345] + list(range(100, 100 + ncol - 6)), dtype=np.uint64)
    for seed, first in ((0, 0), (0xFFFF_FFFF_FFFF_FFFF, 2 ** 32 - 100), (123456789, 7)):
        st, eng = make(pkg, "MIZ", ncol)
        with eng:
            eng.set_column_noise(1.0, 0.0, seed=seed, streams=streams)
            got = eng.noise_innovations(first, 1000)
        want = nz.innovations(seed, streams, first, 1000)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - want)) <= 1e-14, (seed, first)


def test_innovation_statistics(pkg):
    ncol, n = 256, 4096
    st, eng = make(pkg, "Classic", ncol)
    with eng:
        eng.set_column_noise(1.0, 0.0, seed=20261016)
        x = eng.noise_innovations(0, n)
    N = x.size
    # bars: about 5 standard errors of each estimate for N = 2^20 samples (a false alarm is ~1e-6 per bar)
    assert abs(x.mean()) < 5.0 / math.sqrt(N)
    assert abs(x.var() - 1.0) < 5.0 * math.sqrt(2.0 / N)
    lag1 = np.mean(x[:, 1:] * x[:, :-1])
    assert abs(lag1) < 5.0 / math.sqrt(ncol * (n - 1))
    # neighbouring streams: each pair's correlation over n samples has a standard error of 1/64; 255 pairs -> bar 6 s.e.
    xc = (x - x.mean(axis=1, keepdims=True)) / x.std(axis=1, keepdims=True)
    cross = np.mean(xc[1:] * xc[:-1], axis=1)
    assert np.max(np.abs(cross)) < 6.0 / math.sqrt(n)
    assert abs(cross.mean()) < 5.0 / math.sqrt(n * (ncol - 1))
    # Kolmogorov-Smirnov distance against the normal CDF: sqrt(N) D < 1.95 (p = 0.001)
    s = np.sort(x.ravel()[:: 8])
    cdf = 0.5 * (1.0 + np.vectorize(math.erf)(s / math.sqrt(2.0)))
    m = s.size
    d = max(np.max(np.arange(1, m + 1) / m - cdf), np.max(cdf - np.arange(m) / m))
    assert math.sqrt(m) * d < 1.95


# ---- bit identity against the noise-free path ---------------------------------------------------------------------------

PATHS = ("step", "run", "graph", "fused_registers", "fused_lds", "chains2")


@pytest.mark.parametrize("model, cells", [("MIZ", 4), ("MIZ", 2), ("MIZ_IMEX", 4), ("Classic", 4), ("Classic", 2)])
def test_noisy_stepping_equals_single_steps_with_the_noise_as_column_forcing(pkg, model, cells):
    ncol, nsteps = 6, 130            # 130: two graph replays of 64 and two direct steps
    f = forcing(nsteps)
    args = noise_args(ncol)
    ref = None
    for path in PATHS:
        opt = dict(cells_per_thread=cells)
        if path == "graph":
            opt["use_graph"] = True
        elif path in ("run", "step"):
            opt["use_graph"] = False
        elif path == "fused_lds":
            opt["fused_state_in_lds"] = True
        elif path == "fused_registers":
            opt["fused_state_in_lds"] = False
        elif path == "chains2":
            opt["launch_chains"] = 2
        st, eng = make(pkg, model, ncol, **opt)
        with eng:
            eng.set_column_noise(**args)
            if ref is None:
                N = host_N(pkg, eng, args, FIRST, nsteps)
                ref = reference(pkg, model, ncol, nsteps, f, N, cells_per_thread=cells)
            if path == "step":
                for i in range(nsteps):
                    t = (FIRST + i) % st.nt
                    eng.step(eng.ttab[t], eng.ttab[(t + 1) % st.nt], f[i], write_diag=(i == nsteps - 1))
            else:
                spl = 64 if path.startswith("fused") or path == "chains2" else 1
                eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=spl)
            got = eng.get_state(names(model))
            assert np.array_equal(eng.noise_state(), N[:, -1]), (model, cells, path)
        assert_same(got, ref, (model, cells, path))


@pytest.mark.parametrize("model", ["MIZ", "MIZ_IMEX", "Classic"])
def test_integrate_with_noise(pkg, model):
    """ebm_integrate's final state equals the single-step reference's; its means and snapshots are the same bits with 64
    steps per launch and with one."""
    ncol = 4
    args = noise_args(ncol)
    out = {}
    for spl in (64, 1):
        st, eng = make(pkg, model, ncol, integrate_steps_per_launch=spl)
        with eng:
            eng.set_step_clock(0)
            eng.set_column_noise(**args)
            out[spl] = eng.integrate(st.nt, 1, None, True, st.winter.inx, st.summer.inx, ("T", PROG[0] if is_miz(model) else "E"),
                                     want_raw=False)
            out[spl]["state"] = eng.get_state(names(model))
            if spl == 64:
                N = host_N(pkg, eng, args, 0, st.nt)
    for k in ("winter", "summer", "avg"):
        assert np.array_equal(out[64][k], out[1][k], equal_nan=True), k
    assert_same(out[64]["state"], out[1]["state"], "spl")
    st, ref = make(pkg, model, ncol)
    with ref:
        for i in range(st.nt):
            ref.set_column_forcing(N[:, i])
            ref.run(i, 1, None, diag_last=(i == st.nt - 1))
        want = ref.get_state(names(model))
    assert_same(out[64]["state"], want, "integrate vs single steps")


# ---- invariance ----------------------------------------------------------------------------------------------------------

def test_member_alone_in_an_ensemble_and_in_shards(pkg):
    ncol, nsteps = 1000, 100
    f = forcing(nsteps)
    sigma, rho = np.full(ncol, 2.0), np.full(ncol, 0.9)
    st, eng = make(pkg, "MIZ", ncol)
    with eng:
        eng.set_column_noise(sigma, rho, seed=42)
        eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=64)
        whole = eng.get_state(MIZ_ALL)
        Nw = eng.noise_state()
    halves = []
    for lo, hi in ((0, 500), (500, 1000)):
        st, eng = make(pkg, "MIZ", hi - lo)
        with eng:
            eng.set_column_noise(sigma[lo:hi], rho[lo:hi], seed=42, streams=np.arange(lo, hi))
            eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=64)
            halves.append(eng.get_state(MIZ_ALL))
    for k in MIZ_ALL:
        assert np.array_equal(np.concatenate([h[k] for h in halves]), whole[k], equal_nan=True), k
    for j in (0, 317, 999):
        st, eng = make(pkg, "MIZ", 1)
        with eng:
            eng.set_column_noise(2.0, 0.9, seed=42, streams=[j])
            eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=64)
            alone = eng.get_state(MIZ_ALL)
            assert eng.noise_state()[0] == Nw[j]
        for k in MIZ_ALL:
            assert np.array_equal(alone[k][0], whole[k][j], equal_nan=True), (j, k)


@pytest.mark.parametrize("model", ["MIZ", "Classic"])
def test_chunked_calls_and_checkpoint_restart(pkg, model):
    ncol = 5
    f = forcing(400)
    args = noise_args(ncol)
    st, one = make(pkg, model, ncol)
    with one:
        one.set_column_noise(**args)
        one.run(FIRST, 400, f, diag_last=True, steps_per_launch=64)
        want = one.get_state(names(model))
        want_N = one.noise_state()
    st, four = make(pkg, model, ncol)
    with four:
        four.set_column_noise(**args)
        for c in range(4):
            four.run(FIRST + 100 * c, 100, f[100 * c:100 * (c + 1)], diag_last=True, steps_per_launch=64)
            if c == 1:                                   # checkpoint after 200 steps
                ckpt = four.get_state(PROG + ("T0",) if is_miz(model) else ("E", "Tg"))
                ckpt_N = four.noise_state()
        assert_same(four.get_state(names(model)), want, "four calls of 100")
        assert np.array_equal(four.noise_state(), want_N)
    st, fresh = make(pkg, model, ncol, state=ckpt)
    with fresh:
        fresh.set_column_noise(**args)
        fresh.set_noise_state(ckpt_N)
        fresh.set_step_clock(FIRST + 200)
        fresh.run(FIRST + 200, 200, f[200:], diag_last=True, steps_per_launch=64)
        assert_same(fresh.get_state(names(model)), want, "restart")
        assert np.array_equal(fresh.noise_state(), want_N)


# ---- neutrality ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["MIZ", "Classic"])
def test_zero_sigma_and_clearing_give_the_noise_free_bits(pkg, model):
    ncol, nsteps = 4, 100
    f = forcing(nsteps)
    runs = {}
    for how in ("none", "sigma0", "cleared"):
        st, eng = make(pkg, model, ncol)
        with eng:
            if how == "sigma0":
                eng.set_column_noise(0.0, rho=0.7, seed=9)
            elif how == "cleared":
                eng.set_column_noise(3.0, rho=0.5, seed=9)
                eng.set_column_noise(None)
                assert np.array_equal(eng.noise_state(), np.zeros(ncol))
            eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=1)
            eng.run(FIRST + nsteps, nsteps, f, diag_last=True, steps_per_launch=64)
            runs[how] = eng.get_state(names(model))
    assert_same(runs["sigma0"], runs["none"], "sigma = 0")
    assert_same(runs["cleared"], runs["none"], "cleared")


# ---- composition ---------------------------------------------------------------------------------------------------------

def test_noise_with_column_forcing_schedules_and_parameters(pkg):
    """Noise on top of fcol, per-column schedules and per-column parameter rows: equal, to rounding, to the noise-free
    path stepped with the per-step, per-column forcing fcol + schedule(T) + N folded into the column forcing."""
    model, ncol, nsteps = "MIZ", 4, 128
    f = forcing(nsteps)
    args = noise_args(ncol)
    fcol = np.linspace(-1.0, 1.0, ncol)
    Forcing = pkg.Forcing
    # one-year ramps up and down (the reference wants whole years): the steps taken sit on the first one
    forcings = [Forcing(base=0.1 * c, peak=0.1 * c + 2.0 + c, cool=0.1 * c, holdyrs=(0, 0), rates=(2.0 + c, -(2.0 + c)))
                for c in range(ncol)]
    base = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    rows = np.tile(base, (ncol, 1))
    rows[:, pkg.engine.PARAM_ORDER.index("D")] *= np.linspace(0.9, 1.1, ncol)
    st, eng = make(pkg, model, ncol)
    with eng:
        eng.set_column_forcing(fcol)
        eng.set_column_schedules(forcings)
        eng.set_column_params(rows)
        eng.set_column_noise(**args)
        eng.run(FIRST, nsteps, f, diag_last=True, steps_per_launch=64)
        got = eng.get_state(MIZ_ALL)
        N = host_N(pkg, eng, args, FIRST, nsteps)
    words = np.array([pkg.engine.schedule_words(fc) for fc in forcings])

    def sched(T):
        out = np.empty(ncol)
        for c, w in enumerate(words):
            base_, peak, cool, up, down, d1, d2, d3, d4 = w
            out[c] = (base_ if T < d1 else base_ + up * (T - d1) if T < d2 else peak if T < d3
                      else peak + down * (T - d3) if T < d4 else cool)
        return out
    st, ref = make(pkg, model, ncol)
    with ref:
        ref.set_column_params(rows)
        for i in range(nsteps):
            n = FIRST + i
            ref.set_column_forcing(fcol + sched((2 * n + 1) / (2.0 * st.nt)) + N[:, i])
            ref.run(n, 1, f[i:i + 1], diag_last=(i == nsteps - 1))
        want = ref.get_state(MIZ_ALL)
    for k in MIZ_ALL:
        a, b = got[k], want[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        ok = ~np.isnan(a)
        assert np.max(np.abs(a[ok] - b[ok]) / (1.0 + np.abs(b[ok]))) < 1e-10, k


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_equilibrate_refuses_noise_and_works_after_clearing(pkg):
    st, eng = make(pkg, "Classic", 2)
    with eng:
        eng.set_step_clock(0)
        eng.set_column_noise(1.0, 0.5, seed=1)
        with pytest.raises(pkg.EBMError) as e:
            eng.equilibrate(st.nt, 1)
        assert e.value.status == -3 and "noise" in str(e.value)
        with pytest.raises(ValueError):
            eng.set_column_noise(1.0, 1.0)          # rho = 1: refused before the device (the library: below)
        eng.set_column_noise(None)
        out = eng.equilibrate(st.nt, 1)
        assert list(out["years"]) == [1, 1]


def test_library_refuses_bad_noise_arguments(pkg):
    import ctypes
    import sys
    _lib = sys.modules[pkg.__name__ + "._lib"]
    st, eng = make(pkg, "MIZ", 2)
    with eng:
        lib = eng.lib
        ok = np.array([1.0, 1.0])
        for sig, rho in ((np.array([1.0, np.nan]), np.zeros(2)), (np.array([-1.0, 1.0]), np.zeros(2)),
                         (ok, np.array([0.0, 1.0])), (ok, np.array([-0.5, 0.0])), (ok, np.array([np.inf, 0.0]))):
            assert lib.ebm_set_column_noise(eng._h, _lib.dptr(sig), _lib.dptr(rho), None, ctypes.c_ulonglong(0)) == -1
        out = np.empty(2)
        assert lib.ebm_noise_innovations(eng._h, 0, 1, _lib.dptr(out)) == -1        # no noise installed
        assert lib.ebm_set_noise_state(eng._h, _lib.dptr(out)) == -1
        eng.set_column_noise(1.0, 0.0)
        assert lib.ebm_set_noise_state(eng._h, _lib.dptr(np.array([0.0, np.nan]))) == -1
