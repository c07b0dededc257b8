"""Broken builds of the halo exchanges of the one-step kernels' first Newton pass (csrc/ebm_miz_step.h, csrc/ebm_solve.h:
halo_exchange_two, publish_then_vote), for the mutation check of tests/tools/mutants.py, whose anchor rule and build this file
uses unchanged.  Wrong-value mutants only — a word taken for another, a value kept too long; none removes a wait or a barrier
(those orders are played on the host: tests/test_host_step_lds.py).

    python tests/tools/mutants.py check step_halos        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build step_halos        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run step_halos          (GPU box: tests/test_gpu_step_halos.py against each build)

Each must fail tests/test_gpu_step_halos.py (profiles/r34_step_halos_mutants.txt):
  g_halo_from_unmasked_phi        g's halo words are the neighbour's phi, whatever its active set
  r_and_g_words_swapped           the merged read takes g's first value for r's right halo and r's first for g's
  tbar_halo_kept_after_again      the Tbar halo published under a vote that said "again" is what phase D uses
  tbar_halo_both_from_first_word  the left Tbar halo is the neighbour's first value, not its last"""
KIND = "csrc"
TESTS = ("tests/test_gpu_step_halos.py", "-m", "gpu")
LIMIT = 500
MUTANTS = [
    ("g_halo_from_unmasked_phi", "halo_exchange_two(P0, P1, t, T, r[0], r[C - 1], g[0], g[C - 1], rl, rr, gl, gr);",
     "halo_exchange_two(P0, P1, t, T, r[0], r[C - 1], ph[0], ph[C - 1], rl, rr, gl, gr);"),
    ("r_and_g_words_swapped", "const double al = P0[T + tl], ar = P0[tr], bl = P1[tl], br = P0[2 * T + tr];",
     "const double al = P0[T + tl], ar = P0[2 * T + tr], bl = P1[tl], br = P0[tr];"),
    ("tbar_halo_kept_after_again", "again = publish_then_vote(P1, t, T, tb[0], tb[C - 1], changed, tbl, tbr);",
     "{ double l_, r_; again = publish_then_vote(P1, t, T, tb[0], tb[C - 1], changed, l_, r_); if (it == 1) tbl = l_, tbr = r_; }"),
    ("tbar_halo_both_from_first_word", "const double l = P1[T + tl], r = P1[tr];", "const double l = P1[tl], r = P1[tr];"),
]
