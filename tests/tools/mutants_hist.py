"""Broken builds of ebm_ensemble_range and ebm_ensemble_histogram (csrc/ebm_ensemble.hip), for the mutation check of
tests/tools/mutants.py, whose anchor rule and build this file uses unchanged: the same commands, restricted to the mutants
below.  Each changes arithmetic, a comparison or the order of in-bounds reads only — no bound, no launch shape — so a mutant
computes wrong numbers and cannot fault.

    python tests/tools/mutants.py check hist        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build hist        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run hist          (GPU box: tests/test_gpu_ensemble_hist.py must fail against each build)

What each does (profiles/r22_hist_mutants.txt has the verdicts; the range's `w != 0.0 && x == x` is named `counts`, the sums'
`in`, so that each anchor occurs once):
  hist_value_equal_to_hi_stays_inside     `x >= hi` becomes `x > hi`: a value equal to hi has t == nbins and is clamped into
                                          the last bin instead of going above
  hist_clamp_dropped                      min((int)t, nbins - 1) becomes min((int)t, nbins): nextafter(hi, -Inf) with t == nbins
                                          goes to slot nbins + 1 ("above", an allocated slot) instead of the last bin
  range_counts_zero_weights               the range's `w != 0.0` is dropped: members of weight zero count and give extremes.
                                          (The same change in the histogram is an equivalent mutant — adding a weight of 0.0 to
                                          a slot, which is never -0.0, changes no bit — and is not in the list.)
  hist_blocks_added_in_descending_order   the finish kernel's tail loop (the one finish of all three reductions) adds the block
                                          partials from the last to the first: rounding differs with weights over two blocks
                                          and more
  range_later_equal_extreme_wins          strict `x < mn` becomes `x <= mn`: of +0.0 and -0.0 the last, not the first, gives
                                          the bits of the minimum"""
KIND = "csrc"
TESTS = ("tests/test_gpu_ensemble_hist.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("hist_value_equal_to_hi_stays_inside", "const bool below = x < lo, above = x >= hi;", "const bool below = x < lo, above = x > hi;",
     "ebm_ensemble.hip"),
    ("hist_clamp_dropped", "1 + min(i, nbins - 1);", "1 + min(i, nbins);", "ebm_ensemble.hip"),
    ("range_counts_zero_weights", "const bool counts = w != 0.0 && x == x;", "const bool counts = x == x;", "ebm_ensemble.hip"),
    ("hist_blocks_added_in_descending_order", "for (; b < a.nblocks; ++b) r = Combine::of(r, part[b * stride], q);",
     "for (; b < a.nblocks; ++b) r = Combine::of(r, part[(a.nblocks - 1 - b) * stride], q);", "ebm_ensemble.hip"),
    ("range_later_equal_extreme_wins", "mn = (counts && x < mn) ? x : mn;", "mn = (counts && x <= mn) ? x : mn;", "ebm_ensemble.hip"),
]
