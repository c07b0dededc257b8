"""GPU tests (-m gpu) of the prognostic fields' second storage layout.

At four cells per thread the one-launch-per-step MIZ kernel keeps Ei, Ew, h, D, phi pair-split in device memory between
its launches (csrc/ebm_miz_step.h; FieldBook::state_split), every other user of those fields sees the natural layout, and
the runtime converts in place between the two.  Every case here runs one sequence of calls twice: as written, so that
consecutive steps leave the state in the private layout, and with every field read back after every single step, which
forces the round trip through the natural layout each time (that path is what the parity tests hold against the oracle).
The two must agree bit for bit, in every field.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROG = ("Ei", "Ew", "h", "D", "phi")
DIAG = ("Tw", "Ti", "n", "E", "T")
ALL = PROG + ("T0",) + DIAG
# nlat -> workgroup size at four cells per thread: 5 is almost all padding; 255 / 256 / 257 straddle 64 -> 128 threads;
# 1025 is 320 threads; 4096 is 1024 threads, the pitch exactly 4 T
THREADS = {5: 64, 255: 64, 256: 64, 257: 128, 1025: 320, 4096: 1024}


def steps_per_year(model, nlat):
    """The explicit step of the reference is stable for dt ~ dx^2; the extension at the reference test's 2000."""
    return 2000 if model == "MIZ_IMEX" else max(2000, nlat * nlat // 16)


@functools.lru_cache(maxsize=None)
def space(pkg, model, grid, nlat):
    return pkg.SpaceTime(grid, nlat, steps_per_year(model, nlat), 1)


@functools.lru_cache(maxsize=None)
def start_state(pkg, grid, nlat, ncol):
    """Ice poleward of x = 0.55, open water elsewhere: every prognostic field differs from cell to cell and from column
    to column, so a pair that lands in the wrong place shows."""
    par = pkg.default_parameters("MIZ")
    x = space(pkg, "MIZ", grid, nlat).x[None, :]
    c = (1.0 + 0.01 * np.arange(ncol) / max(1, ncol))[:, None]
    phi = np.clip((x - 0.55) * 2.0, 0.0, 0.95) * c / 1.01
    ice = phi > 0
    h = np.where(ice, (par["hmin"] + 1.5 * x) * c, 0.0)
    D = np.where(ice, (par["Dmin"] + 40.0 * x) * c, 0.0)
    Ei = -par["Lf"] * h * phi
    Ew = par["cw"] * (1.0 - phi) * (12.0 * (1.0 - x) + 0.25) * c
    state = dict(Ei=Ei, Ew=Ew, h=h, D=D, phi=phi)
    return {k: np.ascontiguousarray(np.broadcast_to(v, (ncol, nlat)), dtype=np.float64) for k, v in state.items()}


def open_engine(pkg, model, grid, nlat, ncol, **opt):
    st = space(pkg, model, grid, nlat)
    par = pkg.default_parameters("MIZ")
    opt.setdefault("cells_per_thread", 4)
    eng = pkg.Engine(model, st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol, device=0, **opt)
    assert eng.launch_info()["threads"] == THREADS[nlat] and eng.launch_info()["cells_per_thread"] == 4
    eng.set_column_forcing(np.linspace(-1.0, 1.0, ncol))
    eng.set_time_table(st.t)
    eng.set_state(start_state(pkg, grid, nlat, ncol))
    return eng


def same(a, b, what=""):
    for k in a:
        if a[k] is None or b[k] is None:                             # an output that was not asked for
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def stepped(eng, nsteps, diag, natural):
    """nsteps single steps through ebm_step from the handle's clock; natural: every field read back after every step."""
    first = eng.field_step("Ei")["state_step"] + 1
    for i in range(first, first + nsteps):
        eng.step(float(eng.ttab[i % eng.nt]), float(eng.ttab[(i + 1) % eng.nt]), 0.0, diag)
        if natural:
            eng.get_state(ALL if diag else PROG)


SHAPES = [(5, 3), (255, 3), (256, 257), (257, 1), (1025, 3), (4096, 1)]


@pytest.mark.parametrize("nlat,ncol", SHAPES)
@pytest.mark.parametrize("model,grid", [("MIZ", "sin"), ("MIZ", "identity"), ("MIZ_IMEX", "sin"), ("MIZ_IMEX", "identity")])
def test_steps_in_the_private_layout_equal_steps_through_the_natural_one(pkg, model, grid, nlat, ncol):
    """OUT_STATE and OUT_DIAG launches, both grids, the reference's step and the extension, at every workgroup-size
    boundary: six state-only steps and three diagnostic ones, left alone or read back after every step."""
    got = {}
    for natural in (False, True):
        with open_engine(pkg, model, grid, nlat, ncol, use_graph=False) as eng:
            before = eng.state_conversions()
            stepped(eng, 6, False, natural)
            stepped(eng, 3, True, natural)
            n = eng.state_conversions() - before
            got[natural] = eng.get_state(ALL)
            assert n == (2 * 9 if natural else 1), n                 # read back: split and un-split again around every step
            assert eng.state_conversions() - before == (n if natural else 2)
    same(got[False], got[True])
    start = start_state(pkg, grid, nlat, ncol)
    assert not np.array_equal(got[False]["Ew"], start["Ew"])         # (the steps did something)
    assert not got[False]["Ew"][:, nlat:].any()


@pytest.mark.parametrize("nlat,ncol", [(5, 3), (257, 3), (1025, 1)])
@pytest.mark.parametrize("model,grid", [("MIZ", "sin"), ("MIZ_IMEX", "identity")])
def test_integrate_one_launch_per_step(pkg, model, grid, nlat, ncol):
    """OUT_SAVE launches (ebm_integrate with integrate_steps_per_launch = 1): seasonal snapshots — which read the
    prognostic fields in the natural layout in the middle of the year — and annual means of two 12-step years, against
    the same years with the plain stretches fused (the state resident on the chip, natural layout in memory throughout)."""
    names = ("Ei", "phi", "h", "T", "D", "Ew")
    out = {}
    for spl in (1, 5):
        with open_engine(pkg, model, grid, nlat, ncol, integrate_steps_per_launch=spl) as eng:
            st = space(pkg, model, grid, nlat)
            eng.set_time_table(st.t[:12])
            res = eng.integrate(12, 2, None, False, 3, 9, names, want_raw=False)
            out[spl] = dict(res, **{"state_" + k: v for k, v in eng.get_state(PROG).items()})
    same(out[1], out[5])


def test_layout_transitions_on_one_handle(pkg):
    """step, get_field, step, set_field of ONE field, step; step, ebm_run_fused K = 4, step; step, hemispheric mean,
    step; a series sampled every step — each against the same calls with every field read back after every step."""
    nlat, ncol = 257, 3
    marker = np.arange(ncol * nlat, dtype=np.float64).reshape(ncol, nlat) * 1e-3

    def sequence(eng, natural):
        seen = []
        stepped(eng, 2, False, natural)
        seen.append(eng.get_field("h"))
        stepped(eng, 2, False, natural)
        eng.set_field("D", start_state(pkg, "sin", nlat, ncol)["D"] + marker)      # the other four keep their values
        stepped(eng, 2, True, natural)
        eng.run(6, 8, None, False, steps_per_launch=4)
        stepped(eng, 2, False, natural)
        seen.append(eng.hemispheric_mean("phi"))
        seen.append(eng.hemispheric_mean("Ew"))
        stepped(eng, 2, True, natural)
        seen.append(eng.run_series(18, 3, 1, ("Ew", "T", "phi"), None, 1))
        stepped(eng, 1, True, natural)
        return seen, eng.get_state(ALL)

    with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=False) as eng:
        seen_a, a = sequence(eng, False)
    with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=False) as eng:
        seen_b, b = sequence(eng, True)
    same(a, b)
    for i, (u, v) in enumerate(zip(seen_a, seen_b)):
        assert np.array_equal(u, v, equal_nan=True), i


@pytest.mark.parametrize("chains,graph", [(2, False), (1, True), (1, False)])
def test_launch_chains_and_graph_replay(pkg, chains, graph):
    """Two launch chains (each half of the columns on its own stream; a conversion joins them first) and graph replay (the
    conversion is never captured): 130 steps through ebm_run, a read, 130 more — against single steps read back one by
    one."""
    nlat, ncol = 255, 5
    with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=graph, launch_chains=chains) as eng:
        eng.run(0, 130, None, False)
        mid = eng.get_state(PROG)
        eng.run(130, 130, None, True)
        got = eng.get_state(ALL)
        assert eng.state_conversions() == 4                        # split, natural, split, natural
    with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=False) as eng:
        stepped(eng, 130, False, True)
        same(mid, eng.get_state(PROG), "after 130 steps")
        stepped(eng, 129, False, True)
        stepped(eng, 1, True, True)
        same(got, eng.get_state(ALL), "after 260 steps")


@pytest.mark.parametrize("threads", sorted(set(THREADS.values())))
def test_split_then_unsplit_is_the_identity(pkg, threads):
    """The two in-place conversions on a field whose value is its own cell index (ebm_selftest_permute): split puts pair j
    of thread t (cells 4t + 2j, 4t + 2j + 1) at j*2T + 2t, unsplit brings every cell home — at every workgroup size above."""
    from energybalancemodel_jl_amd import _lib
    ncol, T = 3, threads
    cells = np.arange(ncol * 4 * T, dtype=np.float64).reshape(ncol, 4 * T) + 1.0
    split, back = np.empty_like(cells), np.empty_like(cells)
    _lib.check(_lib.load().ebm_selftest_permute(0, T, ncol, _lib.dptr(cells), _lib.dptr(split), _lib.dptr(back)),
               "ebm_selftest_permute")
    assert np.array_equal(back, cells)
    t, j, q = np.meshgrid(np.arange(T), np.arange(2), np.arange(2), indexing="ij")
    want = np.empty_like(cells)
    want[:, (j * 2 * T + 2 * t + q).ravel()] = cells[:, (4 * t + 2 * j + q).ravel()]
    assert np.array_equal(split, want)


@pytest.mark.parametrize("nlat", sorted(THREADS))
def test_the_private_layout_is_the_documented_one(pkg, nlat):
    """What a step leaves in device memory, seen through a zero-copy view taken before it, is the pair-split permutation
    of what the next reader gets — all five prognostic fields, distinct values in every cell."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    ncol, T = 2, THREADS[nlat]
    t, j, q = np.meshgrid(np.arange(T), np.arange(2), np.arange(2), indexing="ij")
    with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=False) as eng:
        views = {k: eng.field_device_ptr(k) for k in PROG}
        stepped(eng, 1, False, False)
        eng.sync()
        raw = {}
        for k, (ptr, pitch) in views.items():
            assert pitch == 4 * T
            raw[k] = np.empty((ncol, pitch))
            assert hip.hipMemcpy(raw[k].ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(raw[k].nbytes), 2) == 0
        back = eng.get_state(PROG)
    for k in PROG:
        natural = np.zeros((ncol, 4 * T))
        natural[:, :nlat] = back[k]
        want = np.empty_like(natural)
        want[:, (j * 2 * T + 2 * t + q).ravel()] = natural[:, (4 * t + 2 * j + q).ravel()]
        assert np.array_equal(raw[k], want, equal_nan=True), k


def test_a_steady_run_converts_once(pkg):
    """50 steps of ebm_run, then 50 of ebm_step: one conversion, at the start."""
    with open_engine(pkg, "MIZ", "sin", 257, 3, use_graph=False) as eng:
        assert eng.state_conversions() == 0
        eng.run(0, 50, None, False)
        assert eng.state_conversions() == 1
        stepped(eng, 50, False, False)
        eng.sync()
        assert eng.state_conversions() == 1
    st = space(pkg, "MIZ", "sin", 255)
    par = pkg.default_parameters("MIZ")
    with pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, 3, device=0,
                    cells_per_thread=2) as eng:
        eng.set_time_table(st.t)
        eng.run(0, 50, None, False)
        eng.get_field("Ei")
        assert eng.state_conversions() == 0                        # two cells per thread: the pair is the chunk


# The alphabet of tests/host_fieldbook_main.cpp (the CPU walk of csrc/ebm_fieldbook.h), as calls of the engine
WALK_EVENTS = ("step_state step_diag step_save graph fused fused_diag fused_active get_prog get_diag get_T0 set_prog set_diag "
               "view_prog mean resample export import params sums_phi sums_other").split()


@pytest.fixture(scope="module")
def fieldbook_prog(tmp_path_factory):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path_factory.mktemp("host_fieldbook") / "host_fieldbook")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", out, os.path.join(root, "tests", "host_fieldbook_main.cpp")], check=True)
    return out


def play_event(pkg, eng, ev, buf):
    """One event of the walk on a MIZ engine whose time table has three entries; what the call returned (None: nothing, or
    the call was refused because the field is stale)."""
    nlat, ncol = eng.nlat, eng.ncol
    first = eng.field_step("Ei")["state_step"] + 1
    tab = lambda i: float(eng.ttab[i % eng.nt])
    marker = np.arange(ncol * nlat, dtype=np.float64).reshape(ncol, nlat) * 1e-3
    par = pkg.default_parameters("MIZ")
    try:
        if ev in ("step_state", "step_diag"):
            return eng.step(tab(first), tab(first + 1), 0.0, ev == "step_diag")
        if ev == "step_save":       # one year of three OUT_SAVE launches, the annual mean only
            return eng.integrate(3, 1, None, False, 0, 0, ("Ew",), want_raw=False, want_seasonal=False)["avg"]
        if ev == "graph":           # (use_graph = False: the same 128 steps, launched one by one)
            return eng.run(first, 128, None, False)
        if ev in ("fused", "fused_diag"):
            return eng.run(first, 8, None, ev == "fused_diag", steps_per_launch=4)
        if ev == "fused_active":    # one round of ebm_run_until that no column ends
            return eng.run_until(first, 1, 8, "T", np.full(ncol, 1e30), np.ones(ncol, dtype=np.int64), steps_per_launch=4)["value"]
        if ev in ("get_prog", "get_diag", "get_T0"):
            return eng.get_field({"get_prog": "phi", "get_diag": "T", "get_T0": "T0"}[ev])
        if ev == "set_prog":
            return eng.set_field("h", start_state(pkg, "sin", nlat, ncol)["h"] + 0.5 + marker)
        if ev == "set_diag":
            return eng.set_field("T", marker)
        if ev == "view_prog":
            eng.field_device_ptr("phi")
            return None
        if ev == "mean":
            return eng.hemispheric_mean("phi")
        if ev == "resample":
            return eng.resample_columns(np.array([1, 2, 0]))
        if ev in ("export", "import"):
            buf.fill_(float("nan"))
            mask = eng.export_columns([0, 1, 2], buf.data_ptr())
            if ev == "import":
                eng.import_columns([0, 1, 2], buf.data_ptr(), mask, [1, 2, 0])
            eng.sync()
            return np.append(buf.cpu().numpy().ravel(), float(mask))
        if ev == "params":
            rows = [{"Lf": par["Lf"] * (1.0 + 0.01 * c)} for c in range(ncol)]
            return eng.set_column_params(pkg.engine.param_matrix(rows, par, pkg.default_parval))
        if ev in ("sums_phi", "sums_other"):
            return eng.ensemble_sums(("phi",) if ev == "sums_phi" else ("T",))
    except pkg.StaleFieldError:
        return None
    raise AssertionError(ev)


@pytest.mark.parametrize("seed", range(8))
def test_random_call_sequences_convert_as_the_cpu_walk_says(pkg, fieldbook_prog, seed):
    """Twelve calls drawn from the alphabet of the field book's CPU walk (tests/test_host_fieldbook.py), on MIZ, sin grid,
    nlat = 257 (128 threads: the pitch exceeds nlat), 3 columns, four cells per thread: as written, and with every current
    field read back after every call.  What the calls return and every field at the end agree bit for bit, and the
    as-written run converts the state exactly as often as the stand-alone program says for the same sequence: the model the
    CPU walk checks the book against is the executor that runs here."""
    import subprocess
    import torch
    nlat, ncol = 257, 3
    seq = [WALK_EVENTS[i] for i in np.random.default_rng(1700 + seed).integers(0, len(WALK_EVENTS), 12)]
    seen, final, conversions = {}, {}, {}
    for natural in (False, True):
        with open_engine(pkg, "MIZ", "sin", nlat, ncol, use_graph=False, integrate_steps_per_launch=1) as eng:
            eng.set_time_table(space(pkg, "MIZ", "sin", nlat).t[:3])
            buf = torch.full((ncol, eng.column_record()[0]), float("nan"), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            before = eng.state_conversions()
            seen[natural] = []
            for ev in seq:
                seen[natural].append(play_event(pkg, eng, ev, buf))
                if natural:
                    eng.get_state([k for k in ALL if eng.field_step(k)["current"]])
            conversions[natural] = eng.state_conversions() - before
            final[natural] = {k: eng.get_field(k) if eng.field_step(k)["current"] else None for k in ALL}
    same(final[False], final[True], seq)
    assert all(final[False][k] is not None for k in PROG)
    for i, (u, v) in enumerate(zip(seen[False], seen[True])):
        assert (u is None) == (v is None), (seq, i)
        assert u is None or np.array_equal(u, v, equal_nan=True), (seq, i)
    # (open_engine sets the five prognostic fields first: the replay starts from a caller's state too)
    r = subprocess.run([fieldbook_prog, "replay", "miz4_derive", "set_prog", *seq], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(seq, conversions, r.stdout.splitlines()[-1])
    assert r.stdout.splitlines()[-1] == f"n_conversions {conversions[False]}", (seq, r.stdout)
