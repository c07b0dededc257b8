"""Broken builds of ebm_column_misfits (csrc/ebm_misfit.hip), for the mutation check of tests/tools/mutants.py, whose anchor
rule and build this file uses unchanged: the same commands, restricted to the mutants below.  Each changes arithmetic, a
condition or the order of in-bounds reads only — no bound, no launch shape — so a mutant computes wrong numbers and cannot
fault.

    python tests/tools/mutants.py check misfits        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build misfits        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run misfits          (GPU box: tests/test_gpu_column_misfits.py must fail against each build)

What each does (profiles/r23_misfit_mutants.txt has the verdicts):
  misfit_term_contracted_to_fma           J + (r d) d becomes fma(r d, d, J): one rounding less per term
  misfit_tree_ascending                   the cross-lane tree runs s = 1, 2, ..., 32: the same 64 values, another association
  misfit_variables_descending             the chains walk the variables from the last to the first.  (Swapping the operands of
                                          the parity add, chain(l, 1) + chain(l, 0), is an equivalent mutant — IEEE addition
                                          commutes — so the order that can show is the one across v.)
  misfit_nan_target_counts                `y == y` is dropped: a cell without an observation counts and makes J NaN
  misfit_odd_tail_padding_cell_read       the second cell of the last unit of an odd nlat, a padding cell, enters chain (l, 1)
  misfit_split_row_read_as_natural        the split flag is ignored: a pair-split row is walked in stored order"""
KIND = "csrc"
TESTS = ("tests/test_gpu_column_misfits.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("misfit_term_contracted_to_fma", "J = in ? J + t2 : J;", "J = in ? fma(t1, d, J) : J;", "ebm_misfit.hip"),
    ("misfit_tree_ascending", "for (int s = 32; s >= 1; s >>= 1) {", "for (int s = 1; s <= 32; s <<= 1) {", "ebm_misfit.hip"),
    ("misfit_variables_descending", "for (int v = 0; v < a.nvars; ++v) {", "for (int v = a.nvars - 1; v >= 0; --v) {", "ebm_misfit.hip"),
    ("misfit_nan_target_counts", "const bool in = live && r != 0.0 && y == y && x == x;", "const bool in = live && r != 0.0 && x == x;",
     "ebm_misfit.hip"),
    ("misfit_odd_tail_padding_cell_read", "live1 = k + 1 < a.nlat;", "live1 = k < a.nlat;", "ebm_misfit.hip"),
    ("misfit_split_row_read_as_natural", "const bool split = (a.split_mask >> v) & 1u;", "const bool split = false;", "ebm_misfit.hip"),
]
