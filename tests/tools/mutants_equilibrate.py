"""Broken builds of ebm_equilibrate's two kernels (equilibrium_check_kernel and compact_active_kernel, csrc/ebm_launch.hip) for
the mutation check of tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.  Every mutant
computes a wrong number at a right address: each changed index stays inside the buffer the unbroken kernel addresses, no
barrier is removed and no loop loses its bound (a list that compacts to fewer columns than it should ends the call sooner).

    python tests/tools/mutants.py check equilibrate  (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build equilibrate  (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run equilibrate    (GPU box: the two test files against each build)

What tests/test_gpu_equilibrate.py and tests/test_gpu_equilibrate_lists.py do with each: profiles/r37_mutants_equilibrate.txt.
  check_forgets_the_fourth_wave        the distance of rows 192 .. 255 (mod 256) never reaches the verdict
  check_walks_every_second_stride      rows 256 .. 511 are neither compared nor snapshotted
  snapshot_never_refreshed             every year is compared with the first
  nan_distance_is_dropped              a NaN difference loses against any number: a column with a NaN field converges
  verdict_of_the_last_field_only       the tolerances of all fields but the last are ignored
  residuals_all_in_the_first_row       every field's residual is written to row 0 of resid
  freezes_before_min_years             a column that repeats in year 2 freezes whatever min_years says
  compaction_forgets_earlier_rounds    of a list of more than 1024 columns only the last round's survivors are counted
  compaction_scan_stops_a_wave_early   the round's total is the count of its sixteenth wave alone
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_equilibrate.py", "tests/test_gpu_equilibrate_lists.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("check_forgets_the_fourth_wave", "max_nan(part[2], part[3])", "max_nan(part[2], part[2])", "ebm_launch.hip"),
    ("check_walks_every_second_stride", "for (int k = t; k < e.nlat; k += 256) {", "for (int k = t; k < e.nlat; k += 512) {", "ebm_launch.hip"),
    ("snapshot_never_refreshed", "            prev[k] = c;\n", "", "ebm_launch.hip"),
    ("nan_distance_is_dropped", "double max_nan(double x, double y) { return (x != x || x > y) ? x : y; }",
     "double max_nan(double x, double y) { return x > y ? x : y; }", "ebm_launch.hip"),
    ("verdict_of_the_last_field_only", "ok = ok && d <= e.tol[v];", "ok = d <= e.tol[v];", "ebm_launch.hip"),
    ("residuals_all_in_the_first_row", "e.resid[(size_t)v * (size_t)e.ncol + col] = d;", "e.resid[col] = d;", "ebm_launch.hip"),
    ("freezes_before_min_years", "e.frozen[col] = (e.may_freeze && ok) ? 1 : 0;", "e.frozen[col] = ok ? 1 : 0;", "ebm_launch.hip"),
    ("compaction_forgets_earlier_rounds", "        total += wave_base[16];", "        total = wave_base[16];", "ebm_launch.hip"),
    ("compaction_scan_stops_a_wave_early", "for (int w = 1; w <= 16; ++w) wave_base[w] += wave_base[w - 1];",
     "for (int w = 1; w <= 15; ++w) wave_base[w] += wave_base[w - 1];", "ebm_launch.hip"),
]
