"""Broken builds of the ensemble Kalman update (ebm_update_columns, csrc/ebm_update.hip) for the mutation check of
tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.  Every mutant computes a wrong number at a
right address: each changed index stays below the bound the unbroken kernel checks.

    python tests/tools/mutants.py check update        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build update        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run update          (GPU box: tests/test_gpu_update_columns.py against each build)

What tests/test_gpu_update_columns.py does with each: profiles/r32_update_mutants.txt.
  tail_group_dropped        a group of fewer than four observation cells at the end of the j axis is not issued
  nan_obs_is_data           d is not replaced by +0.0 where the cell of obs_field is NaN: a sentinel poisons its member
  clamp_not_strict          the lower clamp is written x <= lo: a new value +0.0 under lo = -0.0 becomes -0.0 (the only
                            place where strictness shows: equal values that differ in bits)
  clamp_catches_nan         the lower clamp is written !(x >= lo): a NaN cell becomes lo
  scale_on_the_target       d = scale * (t - xo) instead of t - scale * xo
  store_at_natural_index    the new value goes to the natural cell of its row, not the stored one: right in natural rows,
                            wrong in pair-split ones (k < nlat <= pitch: inside the row)
"d taken from the post-update row" has no one-line form here: the product kernel never reads obs_field, it reads the staged
innovations, which the first kernel has written for ALL columns before the second starts.  What guards that design is
test_obs_field_among_the_updated_fields; staging per field instead would be a rewrite, not a transcription error.
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_update_columns.py", "-m", "gpu")
LIMIT = 400
MUTANTS = [
    ("tail_group_dropped", "(a.nlat - j0 + 3) / 4", "(a.nlat - j0) / 4"),
    ("nan_obs_is_data", "return (in && y == y && xo == xo) ? d : 0.0;", "return (in && y == y) ? d : 0.0;"),
    ("clamp_not_strict", "x = x < lo ? lo : x;", "x = x <= lo ? lo : x;"),
    ("clamp_catches_nan", "x = x < lo ? lo : x;", "x = !(x >= lo) ? lo : x;"),
    ("scale_on_the_target", "const double d = t - s;", "const double d = scale * (t - xo);"),
    ("store_at_natural_index", "double *const cell = a.row[v] + (long long)c * a.pitch + s;",
     "double *const cell = a.row[v] + (long long)c * a.pitch + k;"),
]
