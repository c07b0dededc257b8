"""Broken builds of the series of hemispheric means (ebm_run_series: hemispheric_means_kernel and its launcher in
csrc/ebm_launch.hip, series_driver in csrc/ebm_drive.hip) for the mutation check of tests/tools/mutants.py, whose list, anchor
rule and build this file uses unchanged.  Every mutant computes a wrong number at a right address: each changed index stays
inside the buffer the unbroken code addresses, and no barrier or loop bound is touched.

    python tests/tools/mutants.py check series       (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build series       (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run series         (GPU box: tests/test_gpu_series.py against each build)

What tests/test_gpu_series.py does with each: profiles/r37_mutants_series.txt.
  means_all_land_in_the_first_field    every lane writes row 0 of the sample (the rows of the other fields keep what they had)
  means_of_the_first_field_for_all     every lane sums the terms of field 0
  tile_sum_restarts_per_tile           the running sum starts from 0.0 in every tile of 512 terms: the mean of the last tile.
                                       The line is hemispheric_means_of_column's, the ONE sum of the library, so this build
                                       also breaks ebm_run_until's passage check and the integral column scalars; this list
                                       asks the series' tests alone
  series_forcing_restarts_per_sample   every sample is stepped with the forcing of the first
  series_sample_clock_restarts         the fused launches of every sample carry the model time of the first: schedules and
                                       noise counters repeat, and the handle's clock ends `every` steps after first_step
One that no test can kill, kept as a control ("survives"):
  long_meridian_rule_off_by_a_tile     the LDS row of a field is min(nlat - 1, 512) terms without the `| 1`.  Every term index
                                       is below that length either way, so the same terms are summed in the same order: the
                                       odd row only starts the fields' rows on different banks
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_series.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("means_all_land_in_the_first_field", "s.out[(size_t)lane * (size_t)s.var_stride + col] = acc;", "s.out[col] = acc;", "ebm_launch.hip"),
    ("means_of_the_first_field_for_all", "return column + (size_t)s.slot[v] * (size_t)s.fstride; }, s.x,",
     "return column + (size_t)s.slot[0] * (size_t)s.fstride; }, s.x,", "ebm_launch.hip"),
    ("long_meridian_rule_off_by_a_tile", "b.row = (s.nlat - 1 < kMeanTile ? s.nlat - 1 : kMeanTile) | 1;",
     "b.row = (s.nlat - 1 < kMeanTile ? s.nlat - 1 : kMeanTile);", "ebm_launch.hip", "survives"),
    ("tile_sum_restarts_per_tile", "    for (int k0 = 0; k0 < nterms; k0 += kMeanTile) {\n",
     "    for (int k0 = 0; k0 < nterms; k0 += kMeanTile) {\n        acc = 0.0;\n", "ebm_launch.hip"),
    ("series_forcing_restarts_per_sample", "const double *f = f_steps ? f_steps + (size_t)j * every : nullptr;", "const double *f = f_steps;",
     "ebm_drive.hip"),
    ("series_sample_clock_restarts", ": fused_range(h, first, first, every, f, diag, steps_per_launch, nullptr);",
     ": fused_range(h, first, first_step, every, f, diag, steps_per_launch, nullptr);", "ebm_drive.hip"),
]
