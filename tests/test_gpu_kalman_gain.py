"""ebm_spd_solve_device / ebm_kalman_gain_device on the GPU (include/ebm_hip.h has the definition; tests/kalman_gain_ref.py the
restatements; tests/test_host_kalman_gain.py shows on the CPU that the exact cases are exact)."""
import numpy as np
import pytest
import torch

from kalman_gain_ref import (assemble_ref, backward_errors, bidiagonal_case, diagonal_case, pad_system, random_spd, round_up)
from support import MIZ_PROG, forcing_of, make_engine, midyear_state, same_bits, snapshot, assert_same_snapshot, space_time
from test_gpu_ensemble_sums import blank_engine

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 128, 130, 200)
# eta_dev <= MARGIN * max(eta_lapack, 2^-53) per right-hand side: four times the largest ratio measured on one MI355X over
# error_cases() (profiles/r35_gain_errors.jsonl: 3.96) — another elimination order and explicit block inverses change the
# constant; an indexing error is off by orders of magnitude.  And eta_dev <= 64 m 2^-53 whatever was measured.
MARGIN = 4.0 * 3.96


def solve_on_device(eng, S, B):
    """(L, X, lower triangle and rows as left by ebm_spd_solve_device) of the padded system."""
    Sp, Bp = pad_system(S, B)
    St, Bt = torch.from_numpy(Sp).cuda(), torch.from_numpy(Bp).cuda()
    eng.spd_solve(St, Bt, S.shape[0])
    return St.cpu().numpy(), Bt.cpu().numpy()


@pytest.fixture(scope="module")
def eng(pkg):
    with blank_engine(pkg, "MIZ", 65, 3) as e:
        yield e


@pytest.mark.parametrize("m", SIZES)
def test_exact_factor(eng, m):
    S, L = bidiagonal_case(m)
    got, _ = solve_on_device(eng, S, np.zeros((1, m)))
    assert same_bits(np.tril(got)[:m, :m], L), "the lower triangle is L bit for bit"
    assert np.array_equal(np.tril(got)[m:, m:], np.eye(round_up(m) - m)) and not np.tril(got)[m:, :m].any(), "the padding stays the identity"


@pytest.mark.parametrize("nrhs", (1, 65, 130))
@pytest.mark.parametrize("m", SIZES)
def test_exact_solve(eng, m, nrhs):
    S, B, X = diagonal_case(m, nrhs, 100 * m + nrhs)
    _, got = solve_on_device(eng, S, B)
    assert same_bits(got[:, :m], X) and not got[:, m:].any()


@pytest.mark.parametrize("nvars", (1, 2, 5))
@pytest.mark.parametrize("nlat", (17, 65, 130, 180))
def test_exact_gain_and_scatter(pkg, nlat, nvars):
    """Every second cell unobserved, P_oo diagonal with 4^p - 1, obs_var 1: S = diag(4^p); integer P_fo: observed columns are
    P_fo / 4^p bit for bit, unobserved ones +0.0 by bits.  The same call again: the same bits."""
    rng = np.random.default_rng(nlat + nvars)
    s = 4.0 ** rng.integers(0, 6, nlat)
    P_fo = rng.integers(-2 ** 20, 2 ** 20, (nvars, nlat, nlat)).astype(np.float64)
    P_fo[0, 1, 2] = np.inf                                          # a non-finite entry counts as +0.0
    obs = np.where(np.arange(nlat) % 2 == 0, 1.0, np.nan)
    want = np.where(np.isnan(obs)[None, None, :], 0.0, np.where(np.isfinite(P_fo), P_fo, 0.0) / s)
    Po = torch.from_numpy(np.diag(s - 1.0)).cuda()
    Pf = [torch.from_numpy(p.copy()).cuda() for p in P_fo]
    with blank_engine(pkg, "MIZ", nlat, 3) as e:
        got = e.kalman_gain_tensor(obs, 1.0, None, 1.0, Po, Pf)
        assert same_bits(got.cpu().numpy(), want)
        assert same_bits(e.kalman_gain_tensor(obs, 1.0, None, 1.0, Po, Pf).cpu().numpy(), want)
        none = e.kalman_gain_tensor(np.full(nlat, np.nan), 1.0, None, 1.0, Po, Pf)
        assert same_bits(none.cpu().numpy(), np.zeros((nvars, nlat, nlat))), "nothing observed: a gain of +0.0"


@pytest.mark.parametrize("nlat", (65, 180))
def test_taper_bit_for_bit(pkg, nlat):
    """P_oo = 0 and obs_var = 1 make S the identity, so the gain is B = rho itself: gaspari_cohn, bit for bit."""
    st, _ = space_time(pkg, "sin", nlat)
    x = np.asarray(st.x, dtype=np.float64)
    ones = torch.ones((nlat, nlat), dtype=torch.float64).cuda()
    zero = torch.zeros((nlat, nlat), dtype=torch.float64).cuda()
    with blank_engine(pkg, "MIZ", nlat, 3) as e:
        for half in (0.05, 0.3, 2.0):
            got = e.kalman_gain_tensor(np.zeros(nlat), 1.0, half, 1.0, zero, [ones]).cpu().numpy()[0]
            want = pkg.gaspari_cohn(np.abs(x[:, None] - x[None, :]) / half)
            assert same_bits(got, want), half
            assert (want == 0.0).any() or half == 2.0
        assert same_bits(e.kalman_gain_tensor(np.zeros(nlat), 1.0, None, 1.0, zero, [ones]).cpu().numpy()[0], np.ones((nlat, nlat)))


def ensemble_run(pkg, st, ncol):
    init = {k: v for k, v in midyear_state("MIZ", st, ncol).items() if k in MIZ_PROG}
    return pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), init, fcol=np.linspace(-1.5, 1.5, ncol), device=0)


def stepped(pkg, nlat, ncol, cells=4, state_only=False):
    eng, st = make_engine(pkg, "MIZ", "sin", nlat, ncol, cells, ("noise",))
    first = st.nt // 2
    eng.run(first, 3, forcing_of(first, 3), not state_only, 1)
    return eng, st


def device_covariances(eng, names, obs_name, ncol):
    """P_oo and P_fo of a handle as device tensors: the sums of ebm_ensemble_covariance_device about the means, over ncol."""
    s = eng.ensemble_sums(tuple(names) + (obs_name,))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(s[:, 0] > 0, s[:, 1] / s[:, 0], 0.0)
    out = []
    for i, n in enumerate(tuple(names) + (obs_name,)):
        t = torch.empty((eng.nlat, eng.nlat), dtype=torch.float64, device="cuda")
        eng.ensemble_covariance_device(n, obs_name, None, mean[i], mean[-1], t.data_ptr())
        out.append(t / ncol)
    return out[-1], out[:-1]


def real_case(pkg, nlat, ncol, localize, inflation, every, names=("Ei", "h", "Ew")):
    """(S, B, X of the device, J, the device gain, its inputs) after real steps of a small MIZ ensemble."""
    eng, st = stepped(pkg, nlat, ncol)
    with eng:
        P_oo, P_fo = device_covariances(eng, names, "T", ncol)
        obs = np.zeros(nlat)
        obs[::every] = np.nan if every > 1 else 0.0
        R = np.linspace(0.2, 0.4, nlat)
        factor = inflation * ncol / (ncol - 1.0)
        gain = eng.kalman_gain_tensor(obs, R, localize, factor, P_oo, P_fo).cpu().numpy()
    J, S, B = assemble_ref(st.x, obs, R, localize, factor, P_oo.cpu().numpy(), [p.cpu().numpy() for p in P_fo], pkg.gaspari_cohn)
    m = J.size
    unobserved = np.setdiff1d(np.arange(nlat), J)
    assert same_bits(gain[:, :, unobserved], np.zeros((len(names), nlat, unobserved.size)))
    return S[:m, :m], B[:, :m], gain[:, :, J].reshape(len(names) * nlat, m)


def error_cases(pkg):
    """(label, S, B, X_device): dense random SPD systems with condition numbers over eleven decades through
    ebm_spd_solve_device, and gains from real steps through ebm_kalman_gain_device."""
    with blank_engine(pkg, "MIZ", 65, 3) as e:
        for m, decades, nrhs in ((63, 1.0, 65), (65, 4.0, 130), (130, 8.0, 65), (200, 11.0, 65), (2, 3.0, 1), (128, 6.0, 1)):
            S = random_spd(m, decades, 7 * m)
            B = np.random.default_rng(m).normal(size=(nrhs, m))
            yield f"random m={m} cond=1e{decades:g} nrhs={nrhs}", S, B, solve_on_device(e, S, B)[1][:, :m]
    for nlat, localize, inflation, every in ((65, None, 1.0, 1), (180, 0.3, 1.1, 1), (180, None, 1.05, 3), (65, 0.1, 1.2, 4)):
        S, B, X = real_case(pkg, nlat, 40, localize, inflation, every)
        seen = "every cell observed" if every == 1 else f"one cell in {every} unobserved"
        yield f"real nlat={nlat} localize={localize} inflation={inflation} {seen}", S, B, X


def error_ratios(S, B, X):
    """(eta of the device, eta of numpy.linalg.solve, the largest per-row ratio eta_dev / max(eta_lapack, 2^-53))"""
    eta = backward_errors(S, X, B)
    eta_np = backward_errors(S, np.linalg.solve(S, B.T).T, B)
    return eta, eta_np, float(np.max(eta / np.maximum(eta_np, 2.0 ** -53)))


def test_backward_error_against_lapack(pkg):
    for label, S, B, X in error_cases(pkg):
        eta, eta_np, ratio = error_ratios(S, B, X)
        print(label, "eta_dev", eta.max(), "eta_lapack", eta_np.max(), "ratio", ratio)
        assert np.isfinite(X).all() and np.abs(X).max() > 0.0, label
        assert (eta <= MARGIN * np.maximum(eta_np, 2.0 ** -53)).all(), (label, ratio)
        assert (eta <= 64.0 * S.shape[0] * 2.0 ** -53).all(), (label, eta.max())


def test_real_gain_is_todays_host_gain(pkg):
    """EnsembleRun.kalman_gains: solver="device" against solver="host" from one state — localisation, inflation, a subset
    observed.  Both solve the same system to a backward error of a few 2^-53, so they differ by at most cond(S) times that:
    cond <= (||P||inf * inflation + Rmax) / Rmin."""
    nlat, ncol = 65, 40
    st, _ = space_time(pkg, "sin", nlat)
    run = ensemble_run(pkg, st, ncol)
    try:
        run.run(4)
        obs = np.zeros(nlat)
        obs[::5] = np.nan
        for localize, inflation in ((None, 1.0), (0.25, 1.2)):
            host = run.kalman_gains(("Ei", "T"), "T", obs, 0.3, localize, inflation)
            dev = run.kalman_gains(("Ei", "T"), "T", obs, 0.3, localize, inflation, solver="device")
            g = dev["gain"].cpu().numpy()
            assert g.shape == host["gain"].shape and same_bits(g[:, :, ::5], np.zeros_like(g[:, :, ::5]))
            assert same_bits(dev["mean_o"], host["mean_o"]) and np.array_equal(dev["observed"], host["observed"]) and dev["members"] == ncol
            assert np.allclose(dev["var_o"], host["var_o"], rtol=1e-14, atol=0.0)
            cond = (np.abs(host["var_o"]).max() * nlat * inflation + 0.3) / 0.3
            scale = np.max(np.abs(host["gain"]), axis=2, keepdims=True)
            assert np.abs(host["gain"]).max() > 0.0
            assert (np.abs(g - host["gain"]) <= 64.0 * nlat * 2.0 ** -53 * cond * scale).all(), (localize, float(np.max(np.abs(g - host["gain"]))))
    finally:
        run.close()


def test_same_bits_for_every_geometry_and_layout(pkg):
    """cells_per_thread 4 and 2, rows pair-split (after state-only one-launch steps) and natural (loaded by set_field): each
    handle forms its OWN covariances from the same state with ebm_ensemble_covariance_device and its own gain from them —
    the same bits all the way, and the same call twice the same bits."""
    nlat, ncol = 180, 33
    names = ("Ei", "h", "Ew")
    obs = np.zeros(nlat)
    obs[3::4] = np.nan

    def gain_of(e):
        P_oo, P_fo = device_covariances(e, names, "T", ncol)
        first = e.kalman_gain_tensor(obs, 0.5, 0.4, 1.1 * ncol / (ncol - 1.0), P_oo, P_fo).cpu().numpy()
        assert same_bits(e.kalman_gain_tensor(obs, 0.5, 0.4, 1.1 * ncol / (ncol - 1.0), P_oo, P_fo).cpu().numpy(), first), "twice"
        return first
    eng, _ = stepped(pkg, nlat, ncol)
    with eng:
        assert eng.launch_info()["cells_per_thread"] == 4
        conv = eng.state_conversions()
        want = gain_of(eng)                                          # the rows where they lie: pair-split
        assert eng.state_conversions() == conv, "no field was converted for the covariances or the gain"
        entry = {n: eng.get_field(n) for n in MIZ_PROG + ("T",)}
        assert eng.state_conversions() == conv + 1, "honesty: the state lay pair-split"
    assert np.abs(want).max() > 0.0
    for cells in (4, 2):
        with blank_engine(pkg, "MIZ", nlat, ncol, cells) as other:
            assert other.launch_info()["cells_per_thread"] == cells
            for n in MIZ_PROG + ("T",):                              # prognostic first: T stays current
                other.set_field(n, entry[n])
            assert same_bits(gain_of(other), want), (cells, "natural rows give the bits of the pair-split ones")


def test_not_positive_definite_is_an_ordinary_refusal(pkg):
    nlat, ncol = 65, 7
    eng, st = stepped(pkg, nlat, ncol)
    twin, _ = stepped(pkg, nlat, ncol)
    first = st.nt // 2 + 3
    with eng, twin:
        before = snapshot(eng, "MIZ")
        Sp, Bp = pad_system(np.array([[1.0, 2.0], [2.0, 1.0]]), np.ones((1, 2)))
        with pytest.raises(pkg.EBMError, match=r"ebm_spd_solve_device.*pivot 2 ") as err:
            eng.spd_solve(torch.from_numpy(Sp).cuda(), torch.from_numpy(Bp).cuda(), 2)
        assert err.value.info == 2 and err.value.status == -1
        P = np.eye(nlat)
        P[40, 40] = np.nan
        Pt = torch.from_numpy(P).cuda()
        obs = np.zeros(nlat)
        obs[:10] = np.nan                                            # latitude 40 is observed cell 30: pivot 31
        with pytest.raises(pkg.EBMError, match=r"ebm_kalman_gain_device.*pivot 31 .*observed latitude 40 ") as err:
            eng.kalman_gain_tensor(obs, 1.0, None, 1.0, Pt, [Pt])
        assert err.value.info == 31 and err.value.status == -1
        for bad, what in ((dict(obs=np.where(np.arange(nlat) == 3, np.inf, 0.0)), "infinite"), (dict(obs_var=0.0), "obs_var"),
                          (dict(factor=0.0), "factor"), (dict(factor=np.inf), "factor")):
            kw = dict(obs=obs, obs_var=1.0, localize=None, factor=1.0, P_oo=Pt, P_fo=[Pt]) | bad
            with pytest.raises(pkg.EBMError, match=what):
                eng.kalman_gain_tensor(**kw)
        with pytest.raises(ValueError):
            eng.kalman_gain_tensor(obs, 1.0, None, 1.0, Pt, [Pt] * 6)
        assert_same_snapshot(snapshot(eng, "MIZ"), before, "the refusals left the handle as it was")
        good = torch.from_numpy(np.eye(nlat)).cuda()
        eng.kalman_gain_tensor(obs, 1.0, None, 1.0, good, [good])    # and a good call after them
        assert_same_snapshot(snapshot(eng, "MIZ"), before, "neither does a good call touch a field, the clock or a counter")
        for e_ in (eng, twin):
            e_.run(first, 2, forcing_of(first, 2), True, 1)
        assert_same_snapshot(snapshot(eng, "MIZ"), snapshot(twin, "MIZ"), "steps on with the bits of a handle that never made the calls")


def test_enkf_device_against_host(pkg):
    """enkf(solver="device") and enkf(solver="host") from identical states.  The posterior differs by the update applied to
    the gain difference: |sum_j dG[k][j] d[c][j]| <= nobs * max|dG row| * max|d|, dG within the bound of
    test_real_gain_is_todays_host_gain, plus the update's own rounding on both sides."""
    nlat, ncol = 65, 40
    st, _ = space_time(pkg, "sin", nlat)
    names = ("Ei", "Ew", "h")
    obs = np.full(nlat, np.nan)
    out, post, book = {}, {}, {}
    for solver in ("host", "device"):
        run = ensemble_run(pkg, st, ncol)
        try:
            run.run(4)
            if solver == "host":
                T = run.state(("T",))["T"]
                obs[::2] = T.mean(axis=0)[::2] + 0.3
                gains = run.kalman_gains(names, "T", obs, 0.3, 0.3, 1.1)
                innov = np.abs(obs[None, ::2] - 0.5 * gains["mean_o"][None, ::2] - 0.5 * T[:, ::2]).max()
            conv, counters = run.engine.state_conversions(), run.engine.counters()
            out[solver] = run.enkf(names, "T", obs, 0.3, localize=0.3, inflation=1.1, solver=solver)
            assert run.engine.counters() == counters
            book[solver] = (run.engine.state_conversions() - conv, {n: run.engine.field_step(n) for n in MIZ_PROG + ("T", "T0")})
            post[solver] = run.state(names)
        finally:
            run.close()
    assert book["device"] == book["host"], "the same conversions, the same fields current and stale"
    assert out["device"]["observed"] == out["host"]["observed"] == 33 and out["device"]["gain_shape"] == out["host"]["gain_shape"]
    cond = (np.abs(gains["var_o"]).max() * nlat * 1.1 + 0.3) / 0.3
    moved = 0
    for v, n in enumerate(names):
        grow = np.max(np.abs(gains["gain"][v]), axis=1)              # per state cell
        bound = 33 * innov * (64.0 * nlat * 2.0 ** -53 * cond * grow) + 2.0 ** -50 * (np.abs(post["host"][n]) + 33 * innov * grow[None, :])
        assert (np.abs(post["device"][n] - post["host"][n]) <= bound).all(), n
        moved += int(grow.max() > 0.0)
    assert moved >= 2, "honesty: the fields co-vary with T"
    assert out["device"]["posterior"] is None and out["host"]["posterior"] is None, "T is diagnostic: stale after either update"
    for q in ("bias", "rmse", "spread"):
        assert np.isclose(out["device"]["prior"][q], out["host"]["prior"][q], rtol=1e-9, atol=1e-12), q
