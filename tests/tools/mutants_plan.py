"""Mutation check of the step launch plan (csrc/ebm_plan.h) against its host test: python tests/tools/mutants_plan.py
Each mutant is one textual change of the header, patched in place and restored; tests/test_host_plan.py must fail.  No GPU
test can see these: the kernel families compute the same bits, and a missed LDS raise shows on a few geometries only.  One
line per mutant: KILLED by <first failing test> or SURVIVED (profiles/r20_plan_mutants.txt has the verdicts)."""
import os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "energybalancemodel.jl_amd", "csrc", "ebm_plan.h")
MUTANTS = [
    ("resident_lds_without_the_solve_rows", "plan(K_MIZ_RESIDENT, 20, true)", "plan(K_MIZ_RESIDENT, 18, true)"),
    ("register_kernel_at_512_reads_noise_from_memory", "return plan(K_MIZ_FUSED, 6, T > kFusedRegThreads);",
     "return plan(K_MIZ_FUSED, 6, T >= kFusedRegThreads);"),
    ("column_count_never_prefers_the_resident_kernel", "(T > kFusedRegThreads || cfg.fused_in_lds)", "(T > kFusedRegThreads)"),
    ("two_cell_sums_at_768_threads", "if (T > ((C == 2 && !save) ? kFusedRegThreads2 : kFusedRegThreads)) return none;",
     "if (T > ((C == 2) ? kFusedRegThreads2 : kFusedRegThreads)) return none;"),
    ("two_cell_step_stores_split", "family == K_MIZ_STEP && C == 4};", "family == K_MIZ_STEP};"),
    ("lds_raised_from_64_KiB_not_above", "p.lds_bytes > kDefaultMaxLds;", "p.lds_bytes >= kDefaultMaxLds;"),
    ("one_step_stash_of_two_fields", "plan(K_MIZ_STEP, 6 + 3 * C, false)", "plan(K_MIZ_STEP, 6 + 2 * C, false)"),
    ("extension_fused_in_registers", "save ? C == 4 : v.imex || (C == 4", "save ? C == 4 : (C == 4"),
    ("classic_fused_noise_in_the_kernel", "return plan(K_CLASSIC, 6, v.mode == OUT_LOOP);", "return plan(K_CLASSIC, 6, false);"),
    ("two_cell_geometry_never_768", "if (cells == 2 && cfg.threads > 512) cfg.threads = 768;", ""),
]


def main():
    text = open(HEADER).read()
    survived = 0
    for name, old, new in MUTANTS:
        assert text.count(old) == 1, (name, text.count(old))
        try:
            open(HEADER, "w").write(text.replace(old, new))
            r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_host_plan.py", "-x", "-q", "-p", "no:cacheprovider"],
                               cwd=ROOT, capture_output=True, text=True)
        finally:
            open(HEADER, "w").write(text)
        first = next((l for l in r.stdout.splitlines() if l.startswith(("FAILED", "ERROR"))), "")
        survived += r.returncode == 0
        print(f"{name}: " + ("SURVIVED tests/test_host_plan.py" if r.returncode == 0 else f"KILLED, first: {first[:140]}"), flush=True)
    print(f"{len(MUTANTS)} mutants, {survived} survived")
    return 1 if survived else 0


if __name__ == "__main__":
    sys.exit(main())
