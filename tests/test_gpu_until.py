"""GPU tests (-m gpu) of ebm_run_until (include/ebm_hip.h): step each column until the hemispheric mean of one field crosses
the column's level, and keep the column's state at its crossing.

No oracle: the definition is an identity with entry points the library already has.  Per case, on handles of their own
from the same start (computed once, shared by the tests):
  1. ebm_run_series over max_samples * every steps gives the means m[j][c];
  2. first_crossing (tests/test_host_until.py, NumPy, checked there on hand-made series) gives the expected samples, crossed
     and value;
  3. for every distinct expected samples value s, ebm_run_fused of s * every steps from the start gives the expected state
     of the columns that stop there.
Everything is compared on the bit patterns: the fields, the noise state, the outputs, the validity bookkeeping (which holds
the step clock's last step) and counters[0]; counters[3] is computed from the expected samples alone — per round
ceil(every / K') launches times the chains of that round's list that have a column (tests/test_gpu_equilibrate_lists.py).

Levels are built FROM THE MEASURED SERIES (levels_from): +-inf for "first sample" and "never", which fixes those members
whatever the numbers are, and for the others the running maximum (direction up) or minimum (down) of the member's means up
to a chosen sample — so the crossing is an equality at the bit, and a build with `>` for `>=` stops nobody there.  Every
case first asserts from the reference alone (honesty) that its pattern holds what it claims: at least three distinct
stopping rounds, a member that never stops, a member that stops at round 1, a frozen member whose state would have moved on.

Shapes: nlat 180 (MIZ on both grids, classic, the implicit extension), 1025 (two 512-term tiles of the mean), 65 for the
long lists; lists of 3 (the tail of two launch chains: the list shrinks to one entry, the first chain empty), 65, 1025 and
2100 columns (more than one 1024-entry round of the compaction: an empty wave, waves whose only survivor is lane 0 / lane
63, an empty round); every in {1, 7, 64, 100} with 1 and 64 steps per launch (launch counts that do not divide `every`), and
128 under noise (capped at 64).
"""
import ctypes
import functools

import numpy as np
import pytest

from support import (MIZ_PROG as PROG, all_fields, assert_same_snapshot, bits, forcing_of, is_diagnostic, make_engine, midyear_state,
                     prognostic, same_bits, snapshot)
from test_host_until import first_crossing

pytestmark = pytest.mark.gpu

FIRST, NEVER = 0, -1                           # targets: stop at the first sample / never; t >= 1: the measured sample t


# ---- targets and levels ----------------------------------------------------------------------------------------------------

def targets(ncol, ns):
    """target[c]: FIRST, NEVER or the measured sample 1 .. ns whose running extremum becomes the column's level.  Drawn at
    random, then the places the list code depends on are set (the first compaction sees the identity list, so wave w of it
    is columns 64 w .. 64 w + 63)."""
    t = np.random.default_rng(1000 + ncol).integers(-1, ns + 1, ncol)
    mid = max(2, ns // 2)
    if ncol == 3:                         # two chains: the list goes [0, 1, 2] -> [1, 2] -> [2], one entry, first chain empty
        return np.array([FIRST, mid, NEVER])
    if ncol == 8:
        return np.array([FIRST, NEVER, 3, 5, 2, 4, 6, 1])
    t[0], t[1], t[2] = FIRST, NEVER, mid
    if ncol >= 65:                        # wave 0 keeps every lane but 63; column 64 is the single lane of the second wave
        w = t[:64]
        w[(w == FIRST) | (w == 1)] = mid
        t[63], t[64] = FIRST, ns - 1
    if ncol >= 1025:
        t[0:64] = FIRST                   # an empty wave
        t[64:128] = FIRST                 # only lane 0 survives
        t[64] = NEVER
        t[128:192] = FIRST                # only lane 63 survives
        t[191] = mid
        w = t[192:256]                    # every lane but 63 survives
        w[(w == FIRST) | (w == 1)] = NEVER
        t[255] = FIRST
        t[320:384] = FIRST                # another empty wave, between live ones
        t[1023], t[1024] = NEVER, ns - 1  # the last entry of round 0 and the first of round 1 both survive (1025 columns)
    if ncol >= 2100:
        t[1024:2048] = FIRST              # an empty round between live ones
        t[2048], t[2099] = mid, NEVER
    return t


def levels_from(m, target):
    """(level, direction) [ncol] from the measured means m[ns][ncol].  FIRST / NEVER: +-inf, the direction alternating with
    the column.  A measured target t: the running maximum of m[:t] going up or the running minimum going down — whichever
    is first met later (at t itself where the means are monotone), so the crossing is an equality at the bit."""
    ns, ncol = m.shape
    level, direc = np.empty(ncol), np.empty(ncol, dtype=np.int64)
    for c in range(ncol):
        up, t = c % 2 == 0, int(target[c])
        if t == NEVER:
            level[c], direc[c] = (np.inf, 1) if up else (-np.inf, -1)
        elif t == FIRST:
            level[c], direc[c] = (-np.inf, 1) if up else (np.inf, -3)
        else:
            assert np.isfinite(m[:, c]).all(), f"column {c}: a measured level needs finite means"
            hi, lo = m[:t, c].max(), m[:t, c].min()
            first_hi, first_lo = int(np.argmax(m[:, c] >= hi)), int(np.argmax(m[:, c] <= lo))
            if first_hi > first_lo or (first_hi == first_lo and up):
                level[c], direc[c] = hi, 2
            else:
                level[c], direc[c] = lo, -1
    return level, direc


def launches_expected(samples, every, K, chains):
    """counters[3] from the expected samples alone: per round ceil(every / K) launches for each chain that has a column."""
    total = 0
    for j in range(1, int(samples.max()) + 1):
        n = int((samples >= j).sum())
        nchains = ((n // 2 > 0) + (n - n // 2 > 0)) if chains == 2 else 1
        total += -(-every // K) * nchains
    return total


# ---- one case: reference, honesty, the call -------------------------------------------------------------------------------

def case(model="MIZ", grid="sin", nlat=180, ncol=65, cells=4, every=7, K=64, ns=6, name="Ew", what=(), **opt):
    return (model, grid, nlat, ncol, cells, every, K, ns, name, tuple(what), tuple(sorted(opt.items())))


def reference(pkg, c, level_of=None):
    """Steps 1 to 3 of the module docstring.  level_of(m) -> (level, direction) replaces targets + levels_from."""
    model, grid, nlat, ncol, cells, every, K, ns, name, what, opt = c
    opt = dict(opt)
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells, what, **opt)
    first = st.nt // 2
    f = forcing_of(first, ns * every)
    with eng:
        m = eng.run_series(first, ns * every, every, (name,), f, K)[0]
    level, direc = level_of(m) if level_of else levels_from(m, targets(ncol, ns))
    samples, crossed, value = first_crossing(m, level, direc)
    diag = is_diagnostic(model, name)
    snaps = {}
    for s in sorted(set(samples.tolist())):
        ref, _ = make_engine(pkg, model, grid, nlat, ncol, cells, what, **opt)
        with ref:
            ref.run(first, s * every, f[:s * every], diag, K)
            snaps[s] = snapshot(ref, model)
    return dict(m=m, level=level, direc=direc, samples=samples, crossed=crossed, value=value, snaps=snaps, first=first, f=f,
                diag=diag)


def honesty(c, r, never=True):
    """From the reference alone: the pattern holds what the case claims."""
    model, ncol, ns = c[0], c[3], c[7]
    samples, crossed, snaps = r["samples"], r["crossed"], r["snaps"]
    report = f"{c}: samples {np.unique(samples, return_counts=True)}, crossed {int(crossed.sum())} of {ncol}"
    assert len(set(samples.tolist())) >= 3, f"fewer than three distinct stopping rounds\n{report}"
    assert (crossed & (samples == 1)).any(), f"no member stops at round 1\n{report}"
    if never:
        assert (~crossed).any() and (samples[~crossed] == ns).all(), f"no member runs to the end uncrossed\n{report}"
    R = int(samples.max())
    for s, snap in snaps.items():
        for k in prognostic(model):
            assert np.isfinite(snap["fields"][k]).all(), f"{k} is not finite after {s} rounds: the comparison would be of NaNs"
    early = int(samples.min())
    cols = samples == early
    assert early < R and any(not same_bits(snaps[early]["fields"][k][cols], snaps[R]["fields"][k][cols]) for k in prognostic(model)), \
        f"the members frozen at round {early} would not have moved on: a build that keeps stepping them would pass\n{report}"
    # a crossing at a measured level is an equality at the bit: `>` for `>=` would stop the member later or never
    measured = crossed & np.isfinite(r["level"])
    assert not measured.any() or same_bits(r["value"][measured], r["level"][measured]), report


def expected_after(c, r):
    """The snapshot the call must leave: column by column the reference of the column's own stopping round; bookkeeping and
    counters[0] of the longest; counters[3] by the formula; counters[1], [2] summed over the column-steps taken are not
    predicted here."""
    every, K, what, opt = c[5], c[6], c[9], dict(c[10])
    samples, snaps = r["samples"], r["snaps"]
    R = int(samples.max())
    last = snaps[R]
    fields = {k: v.copy() for k, v in last["fields"].items()}
    noise = last["noise"].copy()
    for s, snap in snaps.items():
        cols = samples == s
        noise[cols] = snap["noise"][cols]
        for k in fields:
            fields[k][cols] = snap["fields"][k][cols]
    Kp = min(K, 64) if "noise" in what else K
    return dict(field_step=last["field_step"], fields=fields, noise=noise, steps=R * every,
                launches=launches_expected(samples, every, Kp, opt.get("launch_chains", 1)))


def assert_call_matches(got, after, want, r, what):
    assert np.array_equal(got["samples"], r["samples"]), (what, got["samples"], r["samples"])
    assert np.array_equal(got["crossed"], r["crossed"]), what
    assert same_bits(got["value"], r["value"]), what
    assert got["steps"] == want["steps"], what
    assert after["field_step"] == want["field_step"], (what, after["field_step"], want["field_step"])
    assert after["counters"]["steps"] == want["steps"], (what, after["counters"])
    assert after["counters"]["launches"] == want["launches"], (what, after["counters"], want["launches"])
    assert same_bits(after["noise"], want["noise"]), what
    assert after["fields"].keys() == want["fields"].keys(), (what, sorted(after["fields"]), sorted(want["fields"]))
    for k in want["fields"]:
        bad = np.flatnonzero((bits(after["fields"][k]) != bits(want["fields"][k])).any(axis=1))
        assert bad.size == 0, f"{what}: field {k} differs in columns {bad[:10]} (stopping rounds {r['samples'][bad[:10]]})"


@functools.lru_cache(maxsize=None)
def run_case(pkg, c, claims=None):
    """Reference, honesty (and the case's own claims(r, ncol) about the reference), then ONE ebm_run_until on a fresh handle:
    computed once per case."""
    model, grid, nlat, ncol, cells, every, K, ns, name, what, opt = c
    r = reference(pkg, c)
    honesty(c, r)
    if claims is not None:
        claims(r, ncol)
    eng, _ = make_engine(pkg, model, grid, nlat, ncol, cells, what, **dict(opt))
    with eng:
        got = eng.run_until(r["first"], ns, every, name, r["level"], r["direc"], r["f"], K)
        after = snapshot(eng, model)
    return r, got, after


def check_case(pkg, c, claims=None):
    r, got, after = run_case(pkg, c, claims)
    want = expected_after(c, r)
    print(f"{c}: rounds {np.unique(r['samples'], return_counts=True)}, launches {after['counters']['launches']} "
          f"(reference {want['launches']})")
    assert_call_matches(got, after, want, r, c)
    return r, got, after


# ---- 1: every x steps per launch -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 64])
@pytest.mark.parametrize("every", [1, 7, 64, 100])
def test_miz_sin_180_every_and_steps_per_launch(pkg, every, K):
    """A prognostic field where every is odd, a diagnostic one (T: diagnostics and T0 of a frozen column are those of its own
    last step) where it is even; 100 steps at 64 to a launch is two launches, of 64 and 36 steps."""
    name = "T" if every % 2 == 0 else "Ew"
    r, got, after = check_case(pkg, case(every=every, K=K, name=name))
    if name == "T":
        assert set(after["fields"]) == set(all_fields("MIZ")), "a diagnostic field: every field is current afterwards"
    else:
        assert set(after["fields"]) == set(PROG)


# ---- 2: the other models and shapes ------------------------------------------------------------------------------------------

def test_miz_identity_two_cells_two_chains_three_columns(pkg):
    """The list shrinks to one entry under two launch chains: its first chain is empty (half = 0)."""
    c = case(grid="identity", ncol=3, cells=2, name="T", launch_chains=2, use_graph=False)
    r, got, after = check_case(pkg, c)
    assert r["samples"][0] == 1 and 1 < r["samples"][1] < c[7] and not r["crossed"][2]


def test_miz_identity_180(pkg):
    check_case(pkg, case(grid="identity", every=64, K=64, name="phi"))


def test_classic_180(pkg):
    check_case(pkg, case(model="Classic", grid="identity", name="T"))


def test_classic_prognostic_one_step_per_launch(pkg):
    check_case(pkg, case(model="Classic", grid="identity", ncol=3, every=7, K=1, name="E"))


def test_miz_imex_180(pkg):
    check_case(pkg, case(model="MIZ_IMEX", every=64, K=64, name="T"))


def test_miz_1025_cells_two_tiles(pkg):
    """1024 terms: the mean takes two full 512-term tiles."""
    check_case(pkg, case(nlat=1025, ncol=3, every=100, K=64, ns=4, name="T"))


# ---- 3: lists past one wave and one compaction round -----------------------------------------------------------------------

def wave_claims(r, ncol):
    """From the reference alone: what survives the first compaction in the waves targets() sets."""
    alive = r["samples"] > 1
    assert not alive[0:64].any() and not alive[320:384].any(), "an empty wave"
    assert alive[64] and not alive[65:128].any(), "a wave whose only survivor is lane 0"
    assert alive[191] and not alive[128:191].any(), "a wave whose only survivor is lane 63"
    assert alive[192:255].all() and not alive[255], "a wave where every lane but 63 survives"
    assert alive[1023], "the last entry of round 0 survives"
    if ncol == 1025:
        assert alive[1024], "the one entry of round 1 survives"
    if ncol >= 2100:
        assert not alive[1024:2048].any() and alive[2048] and alive[2099], "an empty round between live ones"


@pytest.mark.parametrize("ncol", [1025, 2100])
def test_long_lists_miz_sin(pkg, ncol):
    c = case(nlat=65, ncol=ncol, every=7, K=64, name="Ew")
    check_case(pkg, c, wave_claims)


@pytest.mark.parametrize("ncol", [1025, 2100])
def test_long_lists_miz_identity_two_chains(pkg, ncol):
    c = case(grid="identity", nlat=65, ncol=ncol, cells=2, every=7, K=64, name="T", launch_chains=2, use_graph=False)
    check_case(pkg, c, wave_claims)


# ---- 4: the new ground — an active list with noise, schedules and parameter rows installed -----------------------------------

@pytest.mark.parametrize("what, every, K", [(("noise",), 100, 128), (("noise",), 7, 1), (("sched",), 7, 64), (("params",), 64, 64),
                                            (("noise", "sched", "params"), 100, 64)],
                         ids=["noise_capped", "noise_one_step", "schedules", "param_rows", "all_three"])
def test_per_member_settings(pkg, what, every, K):
    """Each N_c must be that of the plain run of the member's own length (expected_after takes it from that run); under
    noise a launch takes at most 64 steps, so 100 steps at K = 128 are two launches."""
    c = case(ncol=8, every=every, K=K, name="T", what=what)
    r, got, after = check_case(pkg, c)
    if "noise" in what:
        stopped = r["samples"] < r["samples"].max()
        R = int(r["samples"].max())
        assert (bits(after["noise"][stopped]) != bits(r["snaps"][R]["noise"][stopped])).all(), \
            "the noise state of a frozen member must not have advanced with the others"
        assert len(np.unique(after["noise"])) == 8


def test_two_calls_compose(pkg):
    """Two calls of max_samples / 2 rounds against one of max_samples.  The second call tests EVERY member anew from its own
    state: a member that crossed in the first call is stepped one more round at least (and stops there if its mean still
    satisfies the comparison), so its state is not that of the single call.  What composes, as the definition implies, is
    the members that had not crossed in the first call — their rounds add up, their flags, values and states are those of
    the single call — and the union of the crossings."""
    c = case(ncol=8, every=7, K=64, ns=6, name="Ew", what=("noise", "sched"))
    model, grid, nlat, ncol, cells, every, K, ns, name, what, opt = c
    r, single, single_after = check_case(pkg, c)
    assert (single["crossed"] & (single["samples"] > ns // 2)).any(), "honesty: a member crosses in the second call"
    half = ns // 2
    eng, _ = make_engine(pkg, model, grid, nlat, ncol, cells, what)
    with eng:
        a = eng.run_until(r["first"], half, every, name, r["level"], r["direc"], r["f"][:half * every], K)
        assert a["steps"] == half * every, "a member runs through the first call: the clock is at first + half * every"
        b = eng.run_until(r["first"] + half * every, half, every, name, r["level"], r["direc"], r["f"][half * every:], K)
        after = snapshot(eng, model)
    want_a = first_crossing(r["m"][:half], r["level"], r["direc"])
    assert np.array_equal(a["samples"], want_a[0]) and np.array_equal(a["crossed"], want_a[1]) and same_bits(a["value"], want_a[2])
    open_ = ~a["crossed"]
    assert open_.sum() >= 2 and a["crossed"].any(), "honesty: both kinds of member"
    assert np.array_equal(a["samples"][open_] + b["samples"][open_], single["samples"][open_])
    assert np.array_equal(b["crossed"][open_], single["crossed"][open_])
    assert same_bits(b["value"][open_], single["value"][open_])
    assert np.array_equal(a["crossed"] | b["crossed"], single["crossed"])
    for k in single_after["fields"]:
        assert same_bits(after["fields"][k][open_], single_after["fields"][k][open_]), k
    assert same_bits(after["noise"][open_], single_after["noise"][open_])
    always = a["crossed"] & np.isinf(r["level"])          # FIRST members: their comparison holds for any finite mean
    assert always.any() and (b["samples"][always] == 1).all() and b["crossed"][always].all()
    assert after["counters"]["steps"] == (half + int(b["samples"].max())) * every
    assert after["field_step"]["Ew"]["state_step"] == r["first"] + after["counters"]["steps"] - 1


# ---- 5: NaN means ----------------------------------------------------------------------------------------------------------

def test_nan_mean_never_crosses(pkg):
    """Ti holds a NaN sentinel in every ice-free cell: its mean is NaN in a column that has one, and no level is crossed —
    not even -inf going up or +inf going down."""
    c = case(ncol=4, every=7, K=64, ns=3, name="Ti")
    model, grid, nlat, ncol, cells, every, K, ns, name, what, opt = c
    level = np.array([-np.inf, np.inf, 0.0, 0.0])
    direc = np.array([1, -1, 1, -1])
    r = reference(pkg, c, level_of=lambda m: (level, direc))
    assert np.isnan(r["m"]).all(), "honesty: every column has an ice-free cell"
    assert (r["samples"] == ns).all() and not r["crossed"].any() and np.isnan(r["value"]).all()
    eng, _ = make_engine(pkg, model, grid, nlat, ncol, cells)
    with eng:
        got = eng.run_until(r["first"], ns, every, name, level, direc, r["f"], K)
        after = snapshot(eng, model)
    assert_call_matches(got, after, expected_after(c, r), r, c)


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    model = "MIZ"
    eng, st = make_engine(pkg, model, "sin", 180, 3, 4, ("noise",))
    lib, F, dptr = eng.lib, pkg.engine.FIELD, pkg.engine.dptr
    ip = ctypes.POINTER(ctypes.c_int)
    first = st.nt // 2
    good = dict(first=first, ns=4, every=2, K=4, field=F["T"], level=np.array([0.0, 1.0, np.inf]),
                direc=np.array([1, -1, 1], dtype=np.int32), samples=np.full(3, 7, dtype=np.int32),
                crossed=np.full(3, 7, dtype=np.int32), value=np.full(3, 7.0))

    def call(h=None, **kw):
        a = dict(good)
        a.update(kw)
        iptr = lambda x: None if x is None else x.ctypes.data_as(ip)
        return lib.ebm_run_until(eng._h if h is None else h, a["first"], a["ns"], a["every"], None, a["K"], a["field"],
                                 dptr(a["level"]), iptr(a["direc"]), iptr(a["samples"]), iptr(a["crossed"]), dptr(a["value"]))
    with eng:
        eng.run(first, 4, None, True, 2)
        before = snapshot(eng, model)
        bad = [dict(every=0), dict(every=-1), dict(ns=0), dict(ns=-2), dict(K=0), dict(first=-1), dict(field=F["Tg"]),
               dict(field=F["T0"]), dict(field=99), dict(field=-1), dict(level=np.array([0.0, np.nan, 1.0])),
               dict(direc=np.array([1, 0, -1], dtype=np.int32)), dict(level=None), dict(direc=None), dict(samples=None),
               dict(crossed=None)]
        for kw in bad:
            assert call(**kw) == -1, kw
            assert b"ebm_run_until" in lib.ebm_last_error(), kw
            assert_same_snapshot(snapshot(eng, model), before, kw)
        assert np.all(good["samples"] == 7) and np.all(good["crossed"] == 7) and np.all(good["value"] == 7.0)
        assert call(first=first + 4, value=None) == 0                  # the call itself is fine, value may be NULL
        assert eng.counters()["steps"] == before["counters"]["steps"] + 8      # (column 2 never crosses: 4 rounds of 2)
        assert good["samples"][2] == 4 and good["crossed"][2] == 0
    # a handle without a time table
    vec = pkg.engine.param_vector(pkg.default_parameters("MIZ"), pkg.default_parval)
    with pkg.Engine(model, st.grid_kind, st.x, vec, st.dt, 3, device=0) as bare:
        assert call(h=bare._h, first=0) == -1
        assert b"ebm_set_time_table" in lib.ebm_last_error()
        assert bare.counters()["steps"] == 0 and bare.field_step("phi")["state_step"] == -1


# ---- 7: EnsembleRun.first_passage ----------------------------------------------------------------------------------------

def test_ensemble_first_passage_is_independent_of_sharding(pkg):
    """One handle of 8 members against two of 4.  The levels come from a series of the same ensemble; the second shard's
    members all cross by round 2, so the shards stop at different rounds and their step_index differs."""
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    par = pkg.default_parameters("MIZ")
    members, every, ns = 8, 20, 5
    init = {k: v for k, v in midyear_state("MIZ", st, members).items() if k != "T0"}
    fcol = np.linspace(-2.0, 2.0, members)
    noise = dict(sigma=1.5, tau=0.01, seed=5)
    forcing = pkg.Forcing(0.75)

    def ensemble(cols):
        run = pkg.EnsembleRun("MIZ", st, par, {k: v[cols] for k, v in init.items()}, fcol=fcol[cols], noise=noise,
                              noise_streams=np.arange(members)[cols])
        run.run(10, forcing)
        return run
    run = ensemble(slice(0, members))
    m = run.series(ns * every, every, names=("T",), forcing=forcing)[0]
    run.close()
    level, direc = levels_from(m, np.array([FIRST, 3, NEVER, 4, 2, FIRST, 1, 2]))
    samples, crossed, value = first_crossing(m, level, direc)
    assert len(set(samples.tolist())) >= 3 and (~crossed[:4]).any() and samples[4:].max() < samples[:4].max(), "honesty"
    words = np.where(direc > 0, "up", "down").tolist()

    def shard(cols, direction):
        run = ensemble(cols)
        out = run.first_passage(ns * every, every, "T", level=level[cols], direction=direction, forcing=forcing)
        state, steps, N = run.state(PROG + ("T",)), run.step_index, run.engine.noise_state()
        run.close()
        return out, state, steps, N
    whole, state, steps, N = shard(slice(0, members), direc)
    assert np.array_equal(whole["samples"], samples) and np.array_equal(whole["crossed"], crossed) and same_bits(whole["value"], value)
    assert steps == 10 + int(samples.max()) * every
    last = 10 + samples * every - 1
    assert np.array_equal(whole["step"], np.where(crossed, last, -1))
    assert same_bits(whole["time"], np.where(crossed, (last + 0.5) * st.dt, np.nan))
    parts = [shard(slice(0, 4), words[:4]), shard(slice(4, members), words[4:])]     # "up" / "down" as well as +-1
    assert parts[0][2] == steps and parts[1][2] == 10 + int(samples[4:].max()) * every < steps
    for k in ("step", "crossed", "samples"):
        assert np.array_equal(np.concatenate([p[0][k] for p in parts]), whole[k]), k
    for k in ("time", "value"):
        assert same_bits(np.concatenate([p[0][k] for p in parts]), whole[k]), k
    for k in state:
        assert same_bits(np.concatenate([p[1][k] for p in parts]), state[k]), k
    assert same_bits(np.concatenate([p[3] for p in parts]), N)
