"""Broken builds of zero-line elision (csrc/ebm_miz_step.h ZERO_LINES, FieldBook::zero_flags_trusted) for the mutation check of
tests/tools/mutants.py, whose anchor rule and build this file uses unchanged: the same commands, restricted to the mutants below.
Each build computes wrong numbers or wrong flags only — no access moves — and each is meant for tests/test_gpu_zero_lines.py.

    python tests/tools/mutants.py check zero_lines        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build zero_lines        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run zero_lines          (GPU box: tests/test_gpu_zero_lines.py against each build)

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
KIND = "csrc"
TESTS = ("tests/test_gpu_zero_lines.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("store_skipped_without_the_old_flag", "if (!(zero_ && (zold & zero_flag_bit(j, (slot_)))))", "if (!zero_)", "ebm_miz_step.h"),
    ("ballot_is_the_lanes_own_value", "    return __builtin_amdgcn_ballot_w64(mine) == 0ull;", "    return !mine;", "ebm_device.h"),
    ("pair_flags_swapped", "__device__ __forceinline__ constexpr unsigned zero_flag_bit(int j, int slot) { return 1u << (4 * j + slot); }",
     "__device__ __forceinline__ constexpr unsigned zero_flag_bit(int j, int slot) { return 1u << (4 * (1 - j) + slot); }", "ebm_device.h"),
    ("outside_writers_leave_the_flags_trusted", "    void zero_flags_disturbed() { zero_flags_trusted_ = false; }",
     "    void zero_flags_disturbed() {}", "ebm_fieldbook.h"),
]
