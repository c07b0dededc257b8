"""Broken builds of the ensemble covariance (ebm_ensemble_covariance, csrc/ebm_covariance.hip) for the mutation check of
tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.

    python tests/tools/mutants.py check covariance        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build covariance        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run covariance          (GPU box: tests/test_gpu_ensemble_cov.py against each build)

What tests/test_gpu_ensemble_cov.py does with each: profiles/r31_covariance_mutants.txt, profiles/r36_dense_tile_mutants.txt.
  tail_group_dropped              a group of fewer than four members at the end of a block is not issued
  b_side_keeps_nan                the NaN cleaning of the B side is skipped: a sentinel of the column field poisons its column
  mirror_wrong_triangle           the finish computes j <= i from partials that rule 6 never wrote, and mirrors those
  weight_zero_contributes         a member of weight 0.0 is staged like any other: 0 * Inf is NaN, and b = y - center stays
  last_cell_is_padding            the latitude bound of the last tile is off by one: where the last pair of a row is half padding
                                  (odd nlat), its cell nlat - 1 is staged as padding too
  blocks_descending               the finish adds partial_0, then the blocks from the last down to the second.  NOT KILLABLE, and
                                  marked so: the definition leaves the bits of a matrix instruction to the hardware, so the
                                  only oracle for real-valued data is the derived bound, which holds for every order of the
                                  block partials; the bit-for-bit tests compare the library with itself (layouts, geometries,
                                  runs), where both sides add in the same wrong order; and on integer data every order is
                                  exact.  It is kept as a control, not counted as a kill.
One mutant of the shared tile (csrc/ebm_mfma_tile.h), which breaks the update and the gain as well; it is listed here only:
  d_map_rows_packed               register g of an accumulator is taken for row g of its 16, not row 4 g: three of every four
                                  results go to a wrong cell of the workgroup's own tile
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_ensemble_cov.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("tail_group_dropped", "(ncols - m0 + 3) / 4", "(ncols - m0) / 4"),
    ("b_side_keeps_nan", "return (in && w != 0.0 && x == x) ? t : 0.0;", "return (in && w != 0.0 && (x == x || !WEIGHTED)) ? t : 0.0;"),
    ("mirror_wrong_triangle", "if (j >= a.nlat || (a.symmetric && j < i)) return;", "if (j >= a.nlat || (a.symmetric && j > i)) return;"),
    ("weight_zero_contributes", "return (in && w != 0.0 && x == x) ? t : 0.0;", "return (in && x == x) ? t : 0.0;"),
    ("last_cell_is_padding", "s.in0 = 2 * u < a.nlat;", "s.in0 = 2 * u < a.nlat - 1;"),
    ("blocks_descending", "for (int b = 1; b < a.nblocks; ++b) r = r + part[b * stride];",
     "for (int b = 1; b < a.nblocks; ++b) r = r + part[(a.nblocks - b) * stride];", None, "survives"),
    ("d_map_rows_packed", "return {l.r0 + 16 * s + 4 * g + l.lk, l.q0 + 16 * t + l.lc};",
     "return {l.r0 + 16 * s + g + l.lk, l.q0 + 16 * t + l.lc};", "ebm_mfma_tile.h"),
]
