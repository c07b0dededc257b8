"""Broken builds of ebm_run_until for the mutation check of tests/tools/mutants.py, whose list, anchor rule and build this
file uses unchanged: the same commands, restricted to the mutants below.

    python tests/tools/mutants.py check until        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build until        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run until          (GPU box: tests/test_gpu_until.py against each build)

What tests/test_gpu_until.py does with each (profiles/r13_until_mutants.txt):
  passage_level_must_be_passed_not_met    a measured level is met with equality at the bit, so nobody stops there: every
                                          case with a measured level fails (25 of 27)
  passage_nan_mean_counts_as_crossed      the Ti columns stop at round 1: test_nan_mean_never_crosses fails, alone
  passage_check_reads_the_list_position   from round 2 on the flags of the wrong columns are written: every case with a
                                          compaction fails (26 of 27)
  passage_round_steps_the_stale_list      frozen columns are stepped in place of live ones: the same 26.  The line is the
                                          round driver's (ActiveRounds::advance), which ebm_equilibrate shares: the mutant
                                          breaks it the same way — from the first compaction on converged columns are
                                          stepped and live ones left behind, so the cases of tests/test_gpu_equilibrate.py
                                          and tests/test_gpu_equilibrate_lists.py in which a column freezes before the last
                                          year fail too"""
KIND = "csrc"
TESTS = ("tests/test_gpu_until.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("passage_level_must_be_passed_not_met", "const bool crossed = p.direction[col] > 0 ? acc >= level : acc <= level;",
     "const bool crossed = p.direction[col] > 0 ? acc > level : acc < level;"),
    ("passage_nan_mean_counts_as_crossed", "const bool crossed = p.direction[col] > 0 ? acc >= level : acc <= level;",
     "const bool crossed = p.direction[col] > 0 ? !(acc < level) : !(acc > level);"),
    ("passage_check_reads_the_list_position", "const int lane = threadIdx.x, col = p.cols[blockIdx.x];",
     "const int lane = threadIdx.x, col = (int)blockIdx.x;"),
    ("passage_round_steps_the_stale_list", "        std::swap(cur, nxt);\n", "", "ebm_drive.hip"),
]
