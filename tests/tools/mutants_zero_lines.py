"""Broken builds of zero-line elision (csrc/ebm_miz_step.h ZERO_LINES, FieldBook::zero_flags_trusted) for the mutation check of
tests/tools/mutants.py, whose anchor rule and build this file uses unchanged: the same commands, restricted to the mutants below.
Each build computes wrong numbers or wrong flags only — no access moves — and each is meant for tests/test_gpu_zero_lines.py.

    python tests/tools/mutants_zero_lines.py check        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants_zero_lines.py build        (CPU: one full build per mutant under build/)
    bash   tests/tools/mutants_run.sh                      (GPU box: the -m gpu suite against every build/libebm_mut_*.so)

  store_skipped_without_the_old_flag    a pair that is zero now is not stored whatever memory holds: a line that melts to
                                        zero keeps its old values in HBM (fields differ from the handle without flags)
  ballot_is_the_lanes_own_value         "all 64 lanes are zero" replaced by "this lane is zero": lanes of one wave disagree,
                                        some skip their store, and lane 0's view becomes the flag (flags and fields differ)
  pair_flags_swapped                    pair 0 reads pair 1's flag and the other way round (fields differ wherever the two
                                        pairs of a wave differ: the 258-cell shape's second wave, every ice edge)
  outside_writers_leave_the_flags_trusted   nobody but the clear takes the trust away any more: not set_field, resampling,
                                        import, the layout passes, nor the plain step that follows an outside write — the
                                        next eliding step believes flags over lines that hold a caller's values
What tests/test_gpu_zero_lines.py does with each: profiles/r19_zero_lines_mutants.txt."""
import sys

import mutants

mutants.MUTANTS = [
    ("store_skipped_without_the_old_flag", "if (!(zero_ && (zold & zero_flag_bit(j, (slot_)))))", "if (!zero_)", "ebm_miz_step.h"),
    ("ballot_is_the_lanes_own_value", "    return __builtin_amdgcn_ballot_w64(mine) == 0ull;", "    return !mine;", "ebm_device.h"),
    ("pair_flags_swapped", "__device__ __forceinline__ constexpr unsigned zero_flag_bit(int j, int slot) { return 1u << (4 * j + slot); }",
     "__device__ __forceinline__ constexpr unsigned zero_flag_bit(int j, int slot) { return 1u << (4 * (1 - j) + slot); }", "ebm_device.h"),
    ("outside_writers_leave_the_flags_trusted", "    void zero_flags_disturbed() { zero_flags_trusted_ = false; }",
     "    void zero_flags_disturbed() {}", "ebm_fieldbook.h"),
]

if __name__ == "__main__":
    if sys.argv[1:2] == ["build"]:
        mutants.build(sys.argv[2:])
    elif sys.argv[1:2] == ["check"]:
        sys.exit(mutants.check())
    else:
        print("\n".join(m[0] for m in mutants.MUTANTS))
