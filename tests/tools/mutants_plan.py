"""Mutation check of the step launch plan (csrc/ebm_plan.h) against its host test: python tests/tools/mutants.py run plan
Each mutant is one textual change of the header in a temporary copy of the tree; tests/test_host_plan.py must fail there.  No GPU
test can see these: the kernel families compute the same bits, and a missed LDS raise shows on a few geometries only.  One
line per mutant: KILLED by <first failing test> or SURVIVED (profiles/r20_plan_mutants.txt has the verdicts)."""
KIND = "tree"
TESTS = ("tests/test_host_plan.py", "-x")
LIMIT = 300
MUTANTS = [
    ("resident_lds_without_the_solve_rows", "plan(K_MIZ_RESIDENT, 20, true)", "plan(K_MIZ_RESIDENT, 18, true)", "csrc/ebm_plan.h"),
    ("register_kernel_at_512_reads_noise_from_memory", "return plan(K_MIZ_FUSED, 6, T > kFusedRegThreads);",
     "return plan(K_MIZ_FUSED, 6, T >= kFusedRegThreads);", "csrc/ebm_plan.h"),
    ("column_count_never_prefers_the_resident_kernel", "(T > kFusedRegThreads || cfg.fused_in_lds)", "(T > kFusedRegThreads)", "csrc/ebm_plan.h"),
    ("two_cell_sums_at_768_threads", "if (T > ((C == 2 && !save) ? kFusedRegThreads2 : kFusedRegThreads)) return none;",
     "if (T > ((C == 2) ? kFusedRegThreads2 : kFusedRegThreads)) return none;", "csrc/ebm_plan.h"),
    ("two_cell_step_stores_split", "family == K_MIZ_STEP && C == 4};", "family == K_MIZ_STEP};", "csrc/ebm_plan.h"),
    ("lds_raised_from_64_KiB_not_above", "p.lds_bytes > kDefaultMaxLds;", "p.lds_bytes >= kDefaultMaxLds;", "csrc/ebm_plan.h"),
    ("one_step_stash_of_two_fields", "plan(K_MIZ_STEP, 6 + 3 * C, false)", "plan(K_MIZ_STEP, 6 + 2 * C, false)", "csrc/ebm_plan.h"),
    ("extension_fused_in_registers", "save ? C == 4 : v.imex || (C == 4", "save ? C == 4 : (C == 4", "csrc/ebm_plan.h"),
    ("classic_fused_noise_in_the_kernel", "return plan(K_CLASSIC, 6, v.mode == OUT_LOOP);", "return plan(K_CLASSIC, 6, false);", "csrc/ebm_plan.h"),
    ("two_cell_geometry_never_768", "if (cells == 2 && cfg.threads > 512) cfg.threads = 768;", "", "csrc/ebm_plan.h"),
]
