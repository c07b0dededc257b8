"""GPU tests (-m gpu) of ebm_resample_columns (include/ebm_hip.h): for every column c at once, the new state of c is the old
state of parent[c]; the member's settings stay with the slot.

No oracle: the definition is an identity with entry points the library already has.  Everything is compared on the bit
patterns (bits / same_bits of tests/support.py): a download before the call, gathered in NumPy, against a download
after it; and the stepping after a resample against a handle that was loaded through set_state / set_field("T0") /
set_noise_state with the gathered download and keeps every column's own settings.

Start: the golden mid-year state of tests/support.py, the columns made different by their forcing offsets (and by
noise and parameter rows where installed) over a few steps.

Shapes, the smallest at which the copy can go wrong: nlat 2 (pitch 128: the row is nearly all padding), 180 at 2 and at 4
cells per thread (128 / 64 threads: active-set rows of 256 / 128 bytes, natural / pair-split layout), 1025 (pitch 2048: a
lane makes four accesses); 1, 3, 65 and 2100 columns; MIZ on both grids, the implicit extension, classic (no active set).

Maps, each first asserted in NumPy alone to be what it claims (map_claims): the identity; a swap; the full shift, ONE
cycle through every column, which an in-place copy in either column order corrupts; a chain without a cycle; the fan-out
of the last column to all; a random map with fixed points, a chain and cycles.
"""
import ctypes

import numpy as np
import pytest

from support import (MIZ_PROG as PROG, all_fields, assert_snapshot_by_column as assert_snapshot, bits, forcing_of, is_miz, make_engine, make_maps,
                     map_claims, midyear_state, prognostic, same_bits, snapshot, step_by)

pytestmark = pytest.mark.gpu

def gathered(snap, p):
    """The snapshot the definition promises: every row that may be read taken from the parent's; the rest unchanged."""
    return dict(field_step=snap["field_step"], counters=snap["counters"], noise=snap["noise"][p],
                fields={k: v[p] for k, v in snap["fields"].items()})


def columns_differ(snap, model, ncol):
    """Honesty: the columns of the snapshot are pairwise different in their prognostic state (else a wrong row passes)."""
    state = np.concatenate([bits(snap["fields"][k]) for k in prognostic(model)], axis=1)
    return len({state[c].tobytes() for c in range(ncol)}) == ncol


# ---- 1: the gather ------------------------------------------------------------------------------------------------------------

GATHER = [("MIZ", "sin", 180, 4, 65), ("MIZ", "sin", 180, 2, 65), ("MIZ", "identity", 180, 4, 3), ("MIZ", "identity", 180, 2, 2100),
          ("MIZ", "sin", 2, 4, 3), ("MIZ", "sin", 2, 4, 2100), ("MIZ", "sin", 1025, 4, 3), ("MIZ", "sin", 180, 4, 1),
          ("MIZ_IMEX", "sin", 180, 4, 65), ("Classic", "identity", 180, 4, 65), ("Classic", "identity", 180, 4, 1)]


@pytest.mark.parametrize("model, grid, nlat, cells, ncol", GATHER, ids=lambda v: str(v))
def test_gather(pkg, model, grid, nlat, cells, ncol):
    """Every map in turn on one handle, a diagnostic step before each so that every field (T0 and the diagnostics
    included) is current and the columns have parted again after the map before; noise installed, so N_c moves too."""
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells, ("noise",))
    first = st.nt // 2
    with eng:
        eng.run(first, 3, forcing_of(first, 3), True, 1)
        step = first + 3
        for name, p in make_maps(ncol).items():
            map_claims(name, p)
            eng.run(step, 2, forcing_of(step, 2), True, 1)
            step += 2
            before = snapshot(eng, model)
            assert set(before["fields"]) == set(all_fields(model)), "honesty: every field is current"
            assert columns_differ(before, model, ncol) and len(np.unique(before["noise"])) == ncol, "honesty: distinct columns"
            conv = eng.state_conversions()
            eng.resample_columns(p)
            assert eng.state_conversions() == conv, name
            assert_snapshot(snapshot(eng, model), gathered(before, p), (name, model, grid, nlat, cells, ncol))


def test_gather_through_the_diffusion_scratch(pkg):
    """A handle that has called ebm_diffusion owns three fields of scratch, which the resample borrows as its staging rows
    and hands back zeroed: the gather is the same and the operator gives the bits it gave before."""
    model, ncol = "MIZ", 65
    eng, st = make_engine(pkg, model, "sin", 180, ncol, 4, ("noise",))
    first = st.nt // 2
    temp = np.random.default_rng(5).normal(0.0, 10.0, (ncol, 180))
    with eng:
        eng.run(first, 3, None, True, 1)
        want = eng.diffusion(temp)
        before = snapshot(eng, model)
        p = make_maps(ncol)["random"]
        eng.resample_columns(p)
        assert_snapshot(snapshot(eng, model), gathered(before, p), "random map through the scratch")
        assert same_bits(eng.diffusion(temp), want), "the scratch came back with its padding zero"


SPLIT = [("MIZ", "sin", 180, 4, 65), ("MIZ", "identity", 180, 4, 3), ("MIZ", "sin", 180, 2, 65), ("MIZ", "sin", 1025, 4, 3),
         ("MIZ_IMEX", "sin", 180, 4, 65), ("Classic", "identity", 180, 4, 65)]


@pytest.mark.parametrize("mapname", ["shift", "random"])
@pytest.mark.parametrize("model, grid, nlat, cells, ncol", SPLIT, ids=lambda v: str(v))
def test_gather_in_the_layout_the_steps_leave(pkg, model, grid, nlat, cells, ncol, mapname):
    """test_gather downloads before it resamples, and a download takes every field to the natural layout.  Here nothing
    reads the handle between its last one-step launch and the resample: at four cells per thread the prognostic AND the
    diagnostic fields are pair-split when their rows are copied.  The expected rows come from a twin handle that took the
    same steps.  Then one ebm_step, which takes its step index from the handle's clock: the clock is where the run left it."""
    p = make_maps(ncol)[mapname]
    map_claims(mapname, p)

    def start():
        eng, st = make_engine(pkg, model, grid, nlat, ncol, cells, ("noise",))
        first = st.nt // 2
        eng.run(first, 5, forcing_of(first, 5), True, 1)
        return eng, first
    twin, first = start()
    with twin:
        before = snapshot(twin, model)
    assert set(before["fields"]) == set(all_fields(model)) and columns_differ(before, model, ncol), "honesty"
    eng, _ = start()
    with eng:
        conv = eng.state_conversions()
        eng.resample_columns(p)
        assert eng.state_conversions() == conv
        after = snapshot(eng, model)
        if is_miz(model) and cells == 4:
            assert eng.state_conversions() == conv + 1, "honesty: the state was pair-split until the download after the resample"
        assert_snapshot(after, gathered(before, p), (mapname, model, grid, nlat, cells, ncol))
        name = prognostic(model)[0]
        assert after["field_step"][name]["state_step"] == first + 4
        ti = (first + 5) % eng.nt
        eng.step(eng.ttab[ti], eng.ttab[(ti + 1) % eng.nt], 0.0, True)
        assert eng.field_step(name)["state_step"] == first + 5, "ebm_step took the step the clock pointed at before the resample"


# ---- 2: continuation ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["run_1", "fused_7", "series"])
@pytest.mark.parametrize("model, grid, cells, what", [("MIZ", "sin", 4, ("noise", "params")), ("MIZ", "identity", 2, ("noise", "params")),
                                                      ("MIZ_IMEX", "sin", 4, ("noise",)), ("Classic", "identity", 4, ("noise",))],
                         ids=["miz_sin_4", "miz_identity_2", "imex", "classic"])
def test_continuation(pkg, model, grid, cells, what, path):
    """Column c after the resample and n more steps = column c of a handle with the same per-column settings, loaded
    through set_state, set_field("T0") and set_noise_state with parent[c]'s downloaded state, after the same global steps."""
    ncol, nlat, n = 9, 180, 7
    p = make_maps(ncol)["random"]
    p[7], p[8] = 5, 5                                  # two clones of one parent, besides the fixed point, cycle and chain
    map_claims("random", p)
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells, what)
    first = st.nt // 2
    f = forcing_of(first, 5 + n)
    with eng:
        eng.run(first, 5, f[:5], True, 1)                # one-step launches: the pair-split layout at four cells per thread
        start = snapshot(eng, model)
        eng.resample_columns(p)
        step_by(eng, path, first + 5, n, f[5:])
        got = snapshot(eng, model)
    assert columns_differ(start, model, ncol), "honesty: distinct parents"
    ref, _ = make_engine(pkg, model, grid, nlat, ncol, cells, what)
    with ref:
        ref.set_state({k: start["fields"][k][p] for k in prognostic(model)})
        if is_miz(model):
            ref.set_field("T0", start["fields"]["T0"][p])
        ref.set_noise_state(start["noise"][p])
        step_by(ref, path, first + 5, n, f[5:])
        want = snapshot(ref, model)
    assert set(got["fields"]) == set(all_fields(model))
    for k in all_fields(model):
        bad = np.flatnonzero((bits(got["fields"][k]) != bits(want["fields"][k])).any(axis=1))
        assert bad.size == 0, f"{path}: field {k} differs in columns {bad} (parents {p[bad]})"
    assert same_bits(got["noise"], want["noise"])
    for k in prognostic(model):
        assert np.isfinite(got["fields"][k]).all(), "the comparison would be of NaNs"
    moved = np.flatnonzero(p != np.arange(ncol))
    k = prognostic(model)[1]
    assert all(not same_bits(got["fields"][k][c], start["fields"][k][p[c]]) for c in moved), "honesty: the steps moved the state"


@pytest.mark.parametrize("noisy", [True, False], ids=["own_streams", "no_noise"])
def test_clones_part_only_through_their_noise(pkg, noisy):
    """Every setting equal but the stream id: the clones of one parent differ after the next steps; without noise they
    stay identical."""
    ncol, model = 5, "MIZ"
    eng, st = make_engine(pkg, model, "sin", 180, ncol)
    first = st.nt // 2
    with eng:
        eng.run(first, 3, None, True, 1)
        eng.set_column_forcing(None)
        if noisy:
            eng.set_column_noise(np.full(ncol, 1.0), rho=np.full(ncol, 0.9), seed=3, streams=np.arange(ncol, dtype=np.uint64) + 50)
        eng.resample_columns(make_maps(ncol)["fanout"])
        clones = eng.get_state(PROG)
        assert all(same_bits(clones[k], np.tile(clones[k][ncol - 1], (ncol, 1))) for k in PROG)
        eng.run(first + 3, 4, None, True, 7)
        after = eng.get_state(PROG)
    distinct = len({bits(after["Ew"][c]).tobytes() for c in range(ncol)})
    assert distinct == (ncol if noisy else 1)
    assert not same_bits(after["Ew"][0], clones["Ew"][0]), "honesty: the steps moved the state"


# ---- 3: layout ----------------------------------------------------------------------------------------------------------------

def test_no_layout_conversion_and_the_host_route_agrees(pkg):
    """ebm_run, resample, ebm_run, ... at four cells per thread: the prognostic fields stay pair-split throughout — as many
    conversions as the loop without the resample, one — and the final state is that of the loop which gathers through the
    host (get_state, NumPy, set_state, T0 and the noise state)."""
    model, ncol, rounds, n = "MIZ", 65, 3, 4
    p = make_maps(ncol)["shift"]

    def loop(select):
        eng, st = make_engine(pkg, model, "sin", 180, ncol, 4, ("noise",))
        first = st.nt // 2
        with eng:
            for r in range(rounds):
                eng.run(first + r * n, n, forcing_of(first + r * n, n), True, 1)
                select(eng)
            eng.run(first + rounds * n, n, None, True, 1)
            conv = eng.state_conversions()
            return conv, snapshot(eng, model)

    def host_route(eng):
        state, N = eng.get_state(PROG + ("T0",)), eng.noise_state()
        eng.set_state({k: v[p] for k, v in state.items()})          # (T0 last: it rebuilds the active set)
        eng.set_noise_state(N[p])
    plain_conv, plain = loop(lambda eng: None)
    dev_conv, dev = loop(lambda eng: eng.resample_columns(p))
    host_conv, host = loop(host_route)
    assert plain_conv == 1, "a steady ebm_run loop converts once"
    assert dev_conv == plain_conv, (dev_conv, plain_conv)
    assert host_conv > dev_conv, "honesty: the host route pays conversions"
    for k in all_fields(model):
        assert same_bits(dev["fields"][k], host["fields"][k]), k
    assert same_bits(dev["noise"], host["noise"])
    assert not same_bits(dev["fields"]["Ew"], plain["fields"]["Ew"]), "honesty: the selection changed the outcome"


# ---- 4: staleness -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model, grid", [("MIZ", "sin"), ("Classic", "identity")])
def test_stale_fields_stay_stale_and_are_not_copied(pkg, model, grid):
    ncol = 65
    eng, st = make_engine(pkg, model, grid, 180, ncol, 4, ("noise",))
    first = st.nt // 2
    p = make_maps(ncol)["random"]
    stale = [k for k in all_fields(model) if k not in prognostic(model)]

    def refusals():
        out = {}
        for k in stale:
            with pytest.raises(pkg.StaleFieldError) as err:
                eng.get_field(k)
            out[k] = str(err.value)
        return out
    with eng:
        eng.run(first, 2, None, True, 1)
        eng.run(first + 2, 3, None, False, 1)            # the diagnostics are of step first + 1, the state of first + 4
        before = snapshot(eng, model)
        assert set(before["fields"]) == set(prognostic(model))
        messages = refusals()
        assert all(f"step {first + 1}" in m and f"step {first + 4}" in m for m in messages.values()), messages
        held = {k: eng.get_field_as_of(k, first + 1) for k in stale}
        eng.resample_columns(p)
        assert refusals() == messages
        assert_snapshot(snapshot(eng, model), gathered(before, p), "prognostic rows under stale diagnostics")
        for k in stale:                                  # not copied: the rows hold what step first + 1 wrote, and say so
            assert same_bits(eng.get_field_as_of(k, first + 1), held[k]), k
        eng.run(first + 5, 1, None, True, 1)             # and the handle steps on, every field current again
        assert set(snapshot(eng, model)["fields"]) == set(all_fields(model))


# ---- 5: two launch chains -----------------------------------------------------------------------------------------------------

def test_two_launch_chains_are_joined_first(pkg):
    """Directly after an ebm_run on two chains (nothing synchronised), rows move across the boundary between the chains'
    halves; then more steps: the bits of the one-chain handle."""
    model, ncol = "MIZ", 65
    p = make_maps(ncol)["shift"]
    p[3], p[60] = 60, 3                                # ... and a swap across the halves, whatever the boundary is
    assert ((p < 32) & (np.arange(ncol) >= 33)).any() and ((p >= 33) & (np.arange(ncol) < 32)).any()

    def run(**opt):
        eng, st = make_engine(pkg, model, "sin", 180, ncol, 4, ("noise",), **opt)
        first = st.nt // 2
        with eng:
            eng.run(first, 6, forcing_of(first, 6), True, 1)
            eng.resample_columns(p)
            eng.run(first + 6, 5, None, True, 1)
            eng.resample_columns(p)
            eng.run(first + 11, 5, None, True, 7)
            return snapshot(eng, model), eng.counters()["launches"]
    one, launches_one = run(use_graph=False)
    two, launches_two = run(launch_chains=2, use_graph=False)
    assert launches_two == 2 * launches_one, "honesty: the second handle ran two chains"
    for k in all_fields(model):
        assert same_bits(one["fields"][k], two["fields"][k]), k
    assert same_bits(one["noise"], two["noise"])


# ---- 6: refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    model, ncol = "MIZ", 5
    eng, st = make_engine(pkg, model, "sin", 180, ncol, 4, ("noise",))
    lib = eng.lib
    ip = ctypes.POINTER(ctypes.c_int)
    first = st.nt // 2
    with eng:
        eng.run(first, 3, None, True, 1)
        before = snapshot(eng, model)
        for bad, col in (([0, 1, -1, 3, 4], 2), ([0, 1, 2, 3, ncol], 4), ([4, 9, 2, -3, 4], 1)):
            a = np.array(bad, dtype=np.int32)
            assert lib.ebm_resample_columns(eng._h, a.ctypes.data_as(ip)) == -1, bad
            msg = lib.ebm_last_error()
            assert b"ebm_resample_columns" in msg and f"parent[{col}]".encode() in msg, msg
            assert_snapshot(snapshot(eng, model), before, bad)
        assert lib.ebm_resample_columns(eng._h, None) == -1
        assert b"ebm_resample_columns" in lib.ebm_last_error() and b"null" in lib.ebm_last_error()
        assert_snapshot(snapshot(eng, model), before, "NULL parent")
        with pytest.raises(ValueError):
            eng.resample_columns([0, 1, 2, 3, 5])
        assert_snapshot(snapshot(eng, model), before, "refused by the binding")


# ---- 7: EnsembleRun.resample --------------------------------------------------------------------------------------------------

def test_ensemble_resample_end_to_end(pkg):
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    members = 16
    init = {k: v for k, v in midyear_state("MIZ", st, members).items() if k != "T0"}
    run = pkg.EnsembleRun("MIZ", st, pkg.default_parameters("MIZ"), init, fcol=np.linspace(-2.0, 2.0, members),
                          noise=dict(sigma=1.5, tau=0.01, seed=5))
    names = PROG + ("T0", "T")
    try:
        T = run.series(40, 20, names=("T",))[0]
        w = np.exp(-0.5 * (T.sum(axis=0) - T.sum(axis=0).mean()))
        parents = pkg.selection_parents(w, np.random.default_rng(1))
        assert (parents != np.arange(members)).any() and (parents == np.arange(members)).any(), "honesty: some move, some stay"
        before, N = run.state(names), run.engine.noise_state()
        run.resample(parents)
        assert run.step_index == 40
        after, N_after = run.state(names), run.engine.noise_state()
        for k in names:
            assert same_bits(after[k], before[k][parents]), k
        assert same_bits(N_after, N[parents])
        run.run(10)
        assert run.step_index == 50 and np.isfinite(run.state(("T",))["T"]).all()
    finally:
        run.close()
