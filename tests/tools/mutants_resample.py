"""Broken builds of ebm_resample_columns for the mutation check of tests/tools/mutants.py, whose anchor rule and build this
file uses unchanged, restricted to the mutants below.

    python tests/tools/mutants.py check resample        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build resample        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run resample          (GPU box: tests/test_gpu_resample.py against each build)

What tests/test_gpu_resample.py does with each is recorded in profiles/r14_resample_mutants.txt."""
KIND = "csrc"
TESTS = ("tests/test_gpu_resample.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    # the scatter pass reads the parent's row of the array itself: an in-place gather, no staging
    ("resample_scatters_in_place", "STAGE ? r.rows + (long long)e.y * r.row_stride : stage;",
     "r.rows + (long long)e.y * r.row_stride;"),
    ("resample_leaves_the_active_set", "a.row_stride = a.units = h->amask ? h->cfg.threads / 8 : 0;", "a.row_stride = a.units = 0;"),
    ("resample_leaves_the_noise_state", "        a.nstate = h->noise.state.get();\n", "        a.nstate = nullptr;\n"),
    # (the fields that travel are the book's current_mask)
    ("resample_copies_stale_fields", "            if (has(f) && is_current(f)) m |= 1u << f;", "            if (has(f)) m |= 1u << f;", "ebm_fieldbook.h"),
    ("resample_marks_the_state_changed", "    if (borrowed) HIPCHK(hipMemsetAsync(h->scratch.get(), 0, sizeof(double) * moved * (size_t)h->pitch, s));\n",
     "    if (borrowed) HIPCHK(hipMemsetAsync(h->scratch.get(), 0, sizeof(double) * moved * (size_t)h->pitch, s));\n    h->book.field_set(EBM_F_Ew);\n"),
    ("resample_keeps_the_scratch_dirty", "    if (borrowed) HIPCHK(hipMemsetAsync(h->scratch.get(), 0, sizeof(double) * moved * (size_t)h->pitch, s));\n", ""),
]
