"""Broken builds of the Kalman gain on the device (ebm_spd_solve_device, ebm_kalman_gain_device, csrc/ebm_gain.hip) for the
mutation check of tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.  Every mutant computes a
wrong number at a right address: each changed index stays inside the buffer the unbroken kernel addresses.

    python tests/tools/mutants.py check gain        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build gain        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run gain          (GPU box: tests/test_gpu_kalman_gain.py against each build)

What tests/test_gpu_kalman_gain.py does with each: profiles/r35_gain_mutants.txt.
  panel_inv_untransposed    the panel tiles are multiplied by inv(L_kk), not by its transpose
  backward_walk_ascending   the backward solve walks the block columns ascending: it subtracts columns that are not solved yet
  padding_diagonal_zero     the padding of S is zeros, not the identity: the first padded pivot is 0
  scatter_at_compact_index  the gain of observed cell j is taken from column min(j, mp - 1) of X, not from column pos[j]
  taper_dropped_from_B      rho is applied to S only
  forward_skips_earlier     the forward solve subtracts nothing of the block columns before k
Two that no test can kill, kept as controls ("survives"):
  trailing_upper_tiles      the trailing update also runs over the tiles above the diagonal.  They are stale from then on, but
                            nothing ever reads them — the factor, the panel and both solves address tiles i >= j only — and
                            the definition leaves the strict upper triangle of S unspecified on return
  flag_ignored_by_solves    the two solve launches do not look at the bad-pivot flag.  They then run on a factor full of NaN,
                            inside the same buffers; the call still returns EBM_ERR_ARG with info, and the definition leaves B
                            and dev_gain unspecified after a bad pivot, so there is nothing for a test to hold
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_kalman_gain.py", "-m", "gpu")
LIMIT = 400
MUTANTS = [
    ("panel_inv_untransposed", "tile_product<false>(acc, sx, sy, tile, a.lds, kGainBlock, a.inv +",
     "tile_product<true>(acc, sx, sy, tile, a.lds, kGainBlock, a.inv +"),
    ("backward_walk_ascending", "const int k = BACKWARD ? T - 1 - step : step, k0 = k * kGainBlock;",
     "const int k = step, k0 = k * kGainBlock;"),
    ("padding_diagonal_zero", "double v = a == b ? 1.0 : 0.0;                                   // the padding: the identity",
     "double v = 0.0;"),
    ("scatter_at_compact_index", "const int a = g.pos[j];", "const int a = g.pos[j] < 0 ? -1 : (j < g.mp ? j : g.mp - 1);"),
    ("taper_dropped_from_B", "v = (g.factor * taper(g.x[k], g.x[ja], g.localize)) *", "v = (g.factor * 1.0) *"),
    ("forward_skips_earlier", "tile_product<false>(acc, sx, sy, rows, a.ldb, xrows, a.S + (long long)k0 * a.lds, a.lds, k0);",
     "tile_product<false>(acc, sx, sy, rows, a.ldb, xrows, a.S + (long long)k0 * a.lds, a.lds, 0);"),
    ("trailing_upper_tiles", "if (j > i || *a.flag) return;                                    // the lower triangle only",
     "if (*a.flag) return;", None, "survives"),
    ("flag_ignored_by_solves", "    if (*a.flag) return;\n    const long long row0", "    const long long row0", None, "survives"),
]
