"""GPU tests (-m gpu) of ebm_export_columns / ebm_import_columns (include/ebm_hip.h) — whole columns into a packed device buffer
of records and back — and of the selection across shards built on them (resample_plan, EnsembleRun.resample_export /
resample_import).

No oracle: every claim is an identity with entry points the library already has, compared on the bit patterns (bits /
same_bits of tests/support.py):
  1. export + import on ONE handle through one buffer, the parents of the moved columns into the moved columns, is
     ebm_resample_columns with the same map (a twin handle);
  2. across two handles that hold different layouts, the destination column reads back as the source column did;
  3. after an import a column steps like a one-column handle with the slot's settings, loaded through the host;
  4. shards that select through the plan equal the unsharded ensemble that calls resample;
  5. every refusal, by return code and message, leaves the handle as it was.

Shapes, the smallest at which the kernel can go wrong: nlat 2 (rowlen 16 of pitch 128), 180 at 2 and at 4 cells per thread
(rowlen 192 of pitch 256; natural and pair-split rows; active-set rows of 256 and 128 bytes), 1025 (rowlen 1040 of pitch 2048:
the last unit is half padding, a lane makes several accesses); 1, 3, 65 and 2100 columns; MIZ on both grids, the implicit
extension, classic (no active set).  The buffers start as NaN, so a slot that is read without having been written shows.
"""
import ctypes

import numpy as np
import pytest
import torch

from support import (all_fields, assert_snapshot_by_column as assert_snapshot, bits, forcing_of, is_miz, make_engine, make_maps, map_claims,
                     member_installer, midyear_state, prognostic, same_bits, snapshot, step_by)

pytestmark = pytest.mark.gpu

IP = ctypes.POINTER(ctypes.c_int)


def nan_buffer(eng, n):
    """n records (at least one, so that the address is real) of NaN on the device, complete before anybody reads them."""
    R, _ = eng.column_record()
    buf = torch.full((max(int(n), 1), R), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return buf


def full_mask(pkg, model, names):
    return sum(1 << pkg.engine.FIELD[k] for k in names)


def exchange_as_resample(eng, p):
    """The map p as one export and one import through one buffer: the distinct parents of the moved columns out, the moved
    columns in, records given.  Nothing is synchronised between the two."""
    moved = np.flatnonzero(p != np.arange(len(p)))
    distinct = np.unique(p[moved])
    buf = nan_buffer(eng, len(distinct))
    mask = eng.export_columns(distinct, buf.data_ptr())
    eng.import_columns(moved, buf.data_ptr(), mask, np.searchsorted(distinct, p[moved]))
    eng.sync()
    return mask


# ---- 1: the same handle ---------------------------------------------------------------------------------------------------------

SAME = [("MIZ", "sin", 180, 4, 65, ("noise",)), ("MIZ", "sin", 180, 2, 65, ("noise",)), ("MIZ", "identity", 180, 4, 3, ("noise", "params")),
        ("MIZ", "identity", 180, 2, 2100, ("noise",)), ("MIZ", "sin", 2, 4, 3, ("noise",)), ("MIZ", "sin", 2, 4, 2100, ()),
        ("MIZ", "sin", 1025, 4, 3, ("noise", "params")), ("MIZ", "sin", 180, 4, 1, ("noise",)), ("MIZ_IMEX", "sin", 180, 4, 65, ("noise",)),
        ("Classic", "identity", 180, 4, 65, ("noise",)), ("Classic", "identity", 180, 4, 1, ())]


@pytest.mark.parametrize("spl", [1, 7], ids=["one_step", "fused"])
@pytest.mark.parametrize("model, grid, nlat, cells, ncol, what", SAME, ids=lambda v: str(v))
def test_same_handle_is_resample(pkg, model, grid, nlat, cells, ncol, what, spl):
    """Every map of make_maps in turn on a handle and its twin, steps before each (one launch per step: at four cells per
    thread the rows are pair-split and, all fields being current, the diagnostics too; fused: natural).  The handle exports
    and imports, the twin resamples: the same snapshot — fields, noise state, field_step, counters."""
    eng, st = make_engine(pkg, model, grid, nlat, ncol, cells, what)
    twin, _ = make_engine(pkg, model, grid, nlat, ncol, cells, what)
    step = st.nt // 2
    with eng, twin:
        for name, p in make_maps(ncol).items():
            map_claims(name, p)
            for e in (eng, twin):
                e.run(step, 3, forcing_of(step, 3), True, spl)
            step += 3
            conv = eng.state_conversions()
            mask = exchange_as_resample(eng, p)
            assert eng.state_conversions() == conv, name
            if (p != np.arange(ncol)).any():
                assert mask == full_mask(pkg, model, all_fields(model)), (name, hex(mask))
            twin.resample_columns(p)
            want = snapshot(twin, model)
            assert set(want["fields"]) == set(all_fields(model)), "honesty: every field is current"
            k = prognostic(model)[1]
            assert len({bits(row).tobytes() for row in want["fields"][k]}) == len(np.unique(p)), "honesty: distinct parents differ"
            assert_snapshot(snapshot(eng, model), want, (name, model, grid, nlat, cells, ncol, spl))


@pytest.mark.parametrize("model, grid, cells", [("MIZ", "sin", 4), ("MIZ", "identity", 2), ("Classic", "identity", 4)])
def test_same_handle_with_stale_diagnostics(pkg, model, grid, cells):
    """The diagnostics are a step older than the state: the mask lacks their bits, the prognostic rows move as under
    resample, and the fields fail with EBM_ERR_STALE afterwards, with the same message; their rows are not written."""
    ncol = 65
    stale = [k for k in all_fields(model) if k not in prognostic(model)]
    p = make_maps(ncol)["random"]

    def start():
        eng, st = make_engine(pkg, model, grid, 180, ncol, cells, ("noise",))
        first = st.nt // 2
        eng.run(first, 2, None, True, 1)
        eng.run(first + 2, 3, None, False, 1)            # the diagnostics are of step first + 1, the state of first + 4
        return eng, first

    def refusals(eng):
        out = {}
        for k in stale:
            with pytest.raises(pkg.StaleFieldError) as err:
                eng.get_field(k)
            out[k] = str(err.value)
        return out
    eng, first = start()
    twin, _ = start()
    with eng, twin:
        messages = refusals(eng)
        assert all(f"step {first + 1}" in m and f"step {first + 4}" in m for m in messages.values()), messages
        assert eng.column_record()[1] == full_mask(pkg, model, prognostic(model))
        held = {k: eng.get_field_as_of(k, first + 1) for k in stale}
        mask = exchange_as_resample(eng, p)
        assert mask == full_mask(pkg, model, prognostic(model)), hex(mask)
        assert refusals(eng) == messages
        twin.resample_columns(p)
        want = snapshot(twin, model)
        assert set(want["fields"]) == set(prognostic(model))
        k = prognostic(model)[1]
        assert len({bits(row).tobytes() for row in want["fields"][k]}) == len(np.unique(p)), "honesty: distinct parents differ"
        assert_snapshot(snapshot(eng, model), want, "prognostic rows under stale diagnostics")
        for k in stale:
            assert same_bits(eng.get_field_as_of(k, first + 1), held[k]), k


# ---- 2: across handles and layouts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("diag", [False, True], ids=["state_only", "all_fields"])
def test_across_handles_and_layouts(pkg, diag):
    """A has just stepped one launch per step (MIZ, four cells: pair-split; state-only steps: phi not stored), B with fused
    launches (natural).  Columns go A -> B and B -> A through two buffers; what reads back from a destination column is what
    read back from the source column of an untouched twin; nobody converts."""
    model, nlat = "MIZ", 180
    nA, nB = 5, 3

    def make_A():
        eng, st = make_engine(pkg, model, "sin", nlat, nA, 4, ("noise",))
        first = st.nt // 2
        eng.run(first, 5, forcing_of(first, 5), diag, 1)
        return eng

    def make_B():
        eng, st = make_engine(pkg, model, "sin", nlat, nB, 4, ("noise", "params"))
        first = st.nt // 2
        eng.run(first, 5, forcing_of(first, 5) + 0.25, diag, 7)
        return eng
    with make_A() as A2, make_B() as B2:
        wantA, wantB = snapshot(A2, model), snapshot(B2, model)
    names = all_fields(model) if diag else prognostic(model)
    assert set(wantA["fields"]) == set(wantB["fields"]) == set(names)
    with make_A() as A, make_B() as B:
        convA, convB = A.state_conversions(), B.state_conversions()
        assert (convA, convB) == (1, 0), "honesty: A holds the pair-split layout, B the natural one"
        a2b, b2a = nan_buffer(A, 2), nan_buffer(B, 1)
        maskA = A.export_columns([4, 1], a2b.data_ptr())
        maskB = B.export_columns([1], b2a.data_ptr())
        assert maskA == maskB == full_mask(pkg, model, names)
        A.sync(), B.sync()
        B.import_columns([0, 2], a2b.data_ptr(), maskA)
        A.import_columns([3], b2a.data_ptr(), maskB)
        A.sync(), B.sync()
        assert (A.state_conversions(), B.state_conversions()) == (convA, convB)
        gotA, gotB = snapshot(A, model), snapshot(B, model)
    assert gotA["field_step"] == wantA["field_step"] and gotB["field_step"] == wantB["field_step"]
    assert gotA["counters"] == wantA["counters"] and gotB["counters"] == wantB["counters"]
    srcA = {0: 0, 1: 1, 2: 2, 4: 4}                                   # untouched columns of A
    for k in names:
        assert same_bits(gotB["fields"][k][0], wantA["fields"][k][4]) and same_bits(gotB["fields"][k][2], wantA["fields"][k][1]), k
        assert same_bits(gotB["fields"][k][1], wantB["fields"][k][1]), k
        assert same_bits(gotA["fields"][k][3], wantB["fields"][k][1]), k
        assert all(same_bits(gotA["fields"][k][c], wantA["fields"][k][c]) for c in srcA), k
    assert same_bits(gotB["noise"], [wantA["noise"][4], wantB["noise"][1], wantA["noise"][1]])
    assert same_bits(gotA["noise"], [wantA["noise"][c] for c in (0, 1, 2)] + [wantB["noise"][1], wantA["noise"][4]])
    for src, dst in ((wantA, wantB), (wantB, wantA)):              # honesty: what arrived differs from what it replaced
        pairs = ((4, 0), (1, 2)) if src is wantA else ((1, 3),)
        for a, b in pairs:
            assert not same_bits(src["noise"][a], dst["noise"][b]) and not same_bits(src["fields"]["Ew"][a], dst["fields"]["Ew"][b])


@pytest.mark.parametrize("model, grid, cells", [("MIZ", "sin", 4), ("Classic", "identity", 4)])
def test_a_slot_whose_field_is_stale_in_the_destination_is_ignored(pkg, model, grid, cells):
    """The source has every field current, the destination's diagnostics are a step older than its state: the prognostic
    rows, the noise state arrive; the diagnostic rows hold what their step wrote and fail as before, with the same message."""
    ncol = 4
    stale = [k for k in all_fields(model) if k not in prognostic(model)]
    S, st = make_engine(pkg, model, grid, 180, ncol, cells, ("noise",))
    D, _ = make_engine(pkg, model, grid, 180, ncol, cells, ("noise",))
    first = st.nt // 2

    def refusals():
        out = {}
        for k in stale:
            with pytest.raises(pkg.StaleFieldError) as err:
                D.get_field(k)
            out[k] = str(err.value)
        return out
    with S, D:
        S.run(first, 5, forcing_of(first, 5) + 0.5, True, 1)
        D.run(first, 2, None, True, 1)
        D.run(first + 2, 3, None, False, 1)
        messages = refusals()
        held = {k: D.get_field_as_of(k, first + 1) for k in stale}
        src = snapshot(S, model)
        buf = nan_buffer(S, 1)
        mask = S.export_columns([1], buf.data_ptr())
        assert mask == full_mask(pkg, model, all_fields(model))
        S.sync()
        steps = {k: D.field_step(k) for k in all_fields(model)}
        D.import_columns([2], buf.data_ptr(), mask)
        D.sync()
        assert {k: D.field_step(k) for k in all_fields(model)} == steps
        assert refusals() == messages
        for k in stale:
            assert same_bits(D.get_field_as_of(k, first + 1), held[k]), k
        after = snapshot(D, model)
        for k in prognostic(model):
            assert same_bits(after["fields"][k][2], src["fields"][k][1]), k
        k = prognostic(model)[1]
        assert not same_bits(after["fields"][k][2], after["fields"][k][1]), "honesty: the columns differ"
        assert same_bits(after["noise"][2], src["noise"][1])


# ---- 3: continuation ------------------------------------------------------------------------------------------------------------

CONT = [("MIZ", "sin", 180, 4, ("noise", "params")), ("MIZ", "identity", 180, 2, ("noise", "params")), ("MIZ", "sin", 2, 4, ("noise",)),
        ("MIZ", "sin", 1025, 4, ("noise", "params")), ("MIZ_IMEX", "sin", 180, 4, ("noise",)), ("Classic", "identity", 180, 4, ("noise",))]


@pytest.mark.parametrize("path", ["run_1", "fused_7", "until"])
@pytest.mark.parametrize("model, grid, nlat, cells, what", CONT, ids=lambda v: str(v))
def test_continues_like_a_loaded_member(pkg, model, grid, nlat, cells, what, path):
    """Column 1 of a source handle (fused steps: natural rows) into column 2 of a destination handle with other settings
    (one launch per step: pair-split rows at four cells).  Then n more steps: column 2 equals a ONE-column handle created
    with slot 2's settings and loaded through the host with the source's state, T0, noise state and clock — so nothing in
    the cells between nlat and rowlen, or beyond, matters."""
    nS, nD, n = 3, 4, 6

    def make_S():
        eng, st = make_engine(pkg, model, grid, nlat, nS, cells, ("noise",))
        first = st.nt // 2
        eng.run(first, 5, forcing_of(first, 5) - 0.5, True, 7)
        return eng, first
    with make_S()[0] as S2:
        src = snapshot(S2, model)
    assert set(src["fields"]) == set(all_fields(model))
    S, first = make_S()
    D, _ = make_engine(pkg, model, grid, nlat, nD, cells, what)
    f = forcing_of(first + 5, n)
    with S, D:
        D.run(first, 5, forcing_of(first, 5), True, 1)
        buf = nan_buffer(S, 3)
        mask = S.export_columns([0, 1, 2], buf.data_ptr())
        S.sync()
        D.import_columns([2], buf.data_ptr(), mask, [1])
        step_by(D, path, first + 5, n, f)
        got = snapshot(D, model)
    ref, _ = make_engine(pkg, model, grid, nlat, 1, cells)
    with ref:
        ref.set_column_forcing(np.linspace(-1.5, 1.5, nD)[2:3])
        if what:
            member_installer(pkg, nD, what)(ref, slice(2, 3))
        ref.set_state({k: src["fields"][k][1:2] for k in prognostic(model)})
        if is_miz(model):
            ref.set_field("T0", src["fields"]["T0"][1:2])
        ref.set_noise_state(src["noise"][1:2])
        step_by(ref, path, first + 5, n, f)
        want = snapshot(ref, model)
    assert set(got["fields"]) == set(want["fields"]) == set(all_fields(model))
    for k in all_fields(model):
        assert same_bits(got["fields"][k][2], want["fields"][k][0]), (path, k)
    assert same_bits(got["noise"][2], want["noise"][0])
    for k in prognostic(model):
        assert np.isfinite(got["fields"][k]).all(), "the comparison would be of NaNs"
    k = prognostic(model)[1]
    assert not same_bits(got["fields"][k][2], src["fields"][k][1]), "honesty: the steps moved the state"


# ---- 4: sharded selection equals unsharded ----------------------------------------------------------------------------------------

def selection_maps(pkg, N, W):
    c = np.arange(N)
    w = np.array([0.0, 1.0]) if N == 2 else np.random.default_rng(N).random(N) ** 4
    maps = {"shift": (c - 1) % N, "fanout": np.full(N, N - 1), "selection": pkg.selection_parents(w, np.random.default_rng(3))}
    starts = np.array([pkg.shard_columns(N, W, r).start for r in range(W)] + [N])
    owner = np.searchsorted(starts, c, side="right") - 1
    for name, p in maps.items():
        assert (owner[p] != owner).any(), f"honesty: {name} names a parent on another shard"
    return maps


@pytest.mark.parametrize("mapname", ["shift", "fanout", "selection"])
@pytest.mark.parametrize("N, W, spl", [(7, 2, 1), (7, 3, 64), (130, 2, 64), (130, 3, 1), (2, 3, 1)], ids=lambda v: str(v))
def test_sharded_selection_equals_unsharded(pkg, N, W, spl, mapname):
    """One EnsembleRun of N members against W shards of the same ensemble in this process, on this device: steps, the
    selection — resample(parents) on the one, the plan's export on ALL shards, the hand-over by slicing, then the import on
    all shards on the others — more steps with diag_last.  Every field and the noise state agree, bit for bit.  N = 2 with
    W = 3 has an empty shard, which owns no run."""
    parents = selection_maps(pkg, N, W)[mapname]
    st = pkg.SpaceTime("sin", 180, 2000, 1)
    par = pkg.default_parameters("MIZ")
    init = {k: v for k, v in midyear_state("MIZ", st, N).items() if k != "T0"}
    fcol = np.linspace(-2.0, 2.0, N)
    rows = [{"D": float(d)} for d in pkg.default_parval["D"] * np.linspace(0.9, 1.1, N)]
    noise = dict(sigma=1.5, tau=0.01, seed=5)
    names = all_fields("MIZ")

    def ensemble(cols):
        run = pkg.EnsembleRun("MIZ", st, par, {k: v[cols] for k, v in init.items()}, fcol=fcol[cols], noise=noise,
                              noise_streams=np.arange(N)[cols], member_params=rows[cols])
        run.run(6, steps_per_launch=spl)
        return run
    whole = ensemble(slice(0, N))
    try:
        whole.resample(parents)
        whole.run(5, diag_last=True, steps_per_launch=spl)
        want, wantN = whole.state(names), whole.engine.noise_state()
    finally:
        whole.close()
    shards = [pkg.shard_columns(N, W, r) for r in range(W)]
    plans = pkg.resample_plan(parents, N, W)
    runs = [ensemble(s) if s.stop > s.start else None for s in shards]
    try:
        sent = [run.resample_export(plans[r]) if run else None for r, run in enumerate(runs)]      # all exports first
        masks = {m for m in (s[1] for s in sent if s)}
        assert len(masks) == 1
        for r, run in enumerate(runs):
            if run is None:
                assert plans[r].ncol == 0 and not len(plans[r].recv_cols)
                continue
            parts = []
            for q in range(W):
                if plans[r].recv_counts[q]:
                    a = int(plans[q].send_counts[:r].sum())
                    parts.append(sent[q][0][a:a + int(plans[q].send_counts[r])])
            received = torch.cat(parts) if parts else sent[r][0][:0]
            run.resample_import(plans[r], received.contiguous(), masks.copy().pop())
        got, gotN = {k: [] for k in names}, []
        for run in runs:
            if run is None:
                continue
            run.run(5, diag_last=True, steps_per_launch=spl)
            state = run.state(names)
            for k in names:
                got[k].append(state[k])
            gotN.append(run.engine.noise_state())
    finally:
        for run in runs:
            if run:
                run.close()
    for k in names:
        assert same_bits(np.concatenate(got[k]), want[k]), k
    assert same_bits(np.concatenate(gotN), wantN)
    assert len({bits(want["Ew"][c]).tobytes() for c in range(N)}) == N, "honesty: the members parted (noise, fcol)"


# ---- 5: refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_alone(pkg):
    model, ncol = "MIZ", 5
    eng, st = make_engine(pkg, model, "sin", 180, ncol, 4, ("noise",))
    lib = eng.lib
    first = st.nt // 2

    def ints(v):
        return None if v is None else np.array(v, dtype=np.int32)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(IP)
    with eng:
        eng.run(first, 3, None, True, 1)
        before = snapshot(eng, model)
        buf = nan_buffer(eng, ncol)
        good = full_mask(pkg, model, all_fields(model))
        prog = full_mask(pkg, model, prognostic(model))
        m = ctypes.c_uint()

        def export(n, cols, addr, h=eng._h):
            c = ints(cols)
            return lib.ebm_export_columns(h, n, ptr(c), ctypes.c_void_p(addr), ctypes.byref(m))

        def imprt(n, cols, recs, addr, mask, h=eng._h):
            c, r = ints(cols), ints(recs)
            return lib.ebm_import_columns(h, n, ptr(c), ptr(r), ctypes.c_void_p(addr), mask)
        d = buf.data_ptr()
        cases = [
            ("export null handle", lambda: export(1, [0], d, h=None), -1, (b"ebm_export_columns", b"null handle")),
            ("import null handle", lambda: imprt(1, [0], None, d, good, h=None), -1, (b"ebm_import_columns", b"null handle")),
            ("record null handle", lambda: lib.ebm_column_record(None, None, None), -1, (b"ebm_column_record", b"null handle")),
            ("export n < 0", lambda: export(-1, [0], d), -1, (b"ebm_export_columns", b"n = -1")),
            ("import n < 0", lambda: imprt(-2, [0], None, d, good), -1, (b"ebm_import_columns", b"n = -2")),
            ("export null cols", lambda: export(2, None, d), -1, (b"ebm_export_columns", b"cols is null")),
            ("import null cols", lambda: imprt(2, None, None, d, good), -1, (b"ebm_import_columns", b"cols is null")),
            ("export null buffer", lambda: export(1, [0], None), -1, (b"ebm_export_columns", b"dev_buf is null")),
            ("import null buffer", lambda: imprt(1, [0], None, None, good), -1, (b"ebm_import_columns", b"dev_buf is null")),
            ("export unaligned", lambda: export(1, [0], d + 8), -1, (b"ebm_export_columns", b"16-byte aligned")),
            ("import unaligned", lambda: imprt(1, [0], None, d + 8, good), -1, (b"ebm_import_columns", b"16-byte aligned")),
            ("export column -1", lambda: export(3, [0, -1, 9], d), -1, (b"ebm_export_columns", b"cols[1] = -1")),
            ("export column ncol", lambda: export(3, [0, 1, ncol], d), -1, (b"ebm_export_columns", b"cols[2] = 5")),
            ("import column ncol", lambda: imprt(3, [4, ncol, -1], None, d, good), -1, (b"ebm_import_columns", b"cols[1] = 5")),
            ("import repeated", lambda: imprt(4, [1, 2, 3, 2], None, d, good), -1, (b"ebm_import_columns", b"cols[3] = 2", b"repeated")),
            ("import record < 0", lambda: imprt(3, [1, 2, 3], [0, -4, -1], d, good), -1, (b"ebm_import_columns", b"records[1] = -4")),
            ("import mask lacks h", lambda: imprt(1, [0], None, d, good & ~(1 << 2)), -1, (b"ebm_import_columns", b"prognostic", b" h")),
            ("import mask has Tg", lambda: imprt(1, [0], None, d, good | (1 << 11)), -1, (b"ebm_import_columns", b"field 11")),
            ("import stale", lambda: imprt(1, [0], None, d, prog), -5, (b"ebm_import_columns", b"field T0", b"current")),
        ]
        for what, call, code, words in cases:
            assert call() == code, what
            msg = lib.ebm_last_error()
            assert all(w in msg for w in words), (what, msg)
            assert_snapshot(snapshot(eng, model), before, what)
        # n == 0 launches nothing and needs nothing
        assert export(0, None, None) == 0 and m.value == good
        assert imprt(0, None, None, None, good) == 0
        assert_snapshot(snapshot(eng, model), before, "n == 0")
        # the binding refuses before any device call
        for bad in (lambda: eng.export_columns([0, ncol], d), lambda: eng.export_columns([0], d + 8),
                    lambda: eng.import_columns([1, 1], d, good), lambda: eng.import_columns([1], d, good, [-1]),
                    lambda: eng.import_columns([1.5], d, good), lambda: eng.import_columns([1], d, -1)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(pkg.StaleFieldError):
            eng.import_columns([1], d, prog)
        assert_snapshot(snapshot(eng, model), before, "refused by the binding")
        # repeated SOURCE columns are legal: two records of one column
        assert export(2, [3, 3], d) == 0
        eng.sync()
        rows = buf[:2].cpu().numpy()
        assert same_bits(rows[0], rows[1]) and not np.isnan(rows[0][:180]).any()
