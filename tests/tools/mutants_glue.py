"""Mutation check of the Python glue between the host mirror and the C ABI, on the GPU box (no build needed):
python tests/tools/mutants.py run glue  — patches one line of energybalancemodel.jl_amd/*.py at a time in a temporary copy of
the tree and runs the -m gpu suite with -x inside the copy.  One line per mutant: KILLED by <first failing test> or SURVIVED."""
KIND = "tree"
TESTS = ("tests", "-m", "gpu", "-x")
LIMIT = 600
MUTANTS = [
    ("parameter_vector_swaps_A_and_B", 'PARAM_ORDER = ("D", "A", "B",', 'PARAM_ORDER = ("D", "B", "A",', "_lib.py"),
    ("field_ids_swap_Tw_and_Ti", '"T0": 5, "Tw": 6, "Ti": 7,', '"T0": 5, "Tw": 7, "Ti": 6,', "_lib.py"),
    ("time_table_half_a_step_late", "tab = np.array([cos2pit(float(t)) for t in t_in_year], dtype=np.float64)",
     "tab = np.array([cos2pit(float(t) + 0.5 / len(t_in_year)) for t in t_in_year], dtype=np.float64)", "engine.py"),
    ("column_forcing_negated", "a = None if fcol is None else as_f64(fcol, (self.ncol,))", "a = None if fcol is None else -as_f64(fcol, (self.ncol,))",
     "engine.py"),
    ("run_inverts_diag_last", 'check(self.lib.ebm_run(self._h, int(first_step), int(nsteps), dptr(a), int(diag_last)),',
     'check(self.lib.ebm_run(self._h, int(first_step), int(nsteps), dptr(a), int(not diag_last)),', "engine.py"),
    ("integrate_inverts_lastonly", "check(self.lib.ebm_integrate(self._h, nt, dur, dptr(f), int(lastonly), int(winter_inx),",
     "check(self.lib.ebm_integrate(self._h, nt, dur, dptr(f), int(not lastonly), int(winter_inx),", "engine.py"),
    ("solutions_winter_filled_with_summer", 'sols.seasonal.winter[v] = out["winter"][vi, :, 0, :]', 'sols.seasonal.winter[v] = out["summer"][vi, :, 0, :]',
     "infrastructure.py"),
]
