"""Broken builds of phase D's input loads in the one-step kernels (csrc/ebm_miz_step.h), for the mutation check of
tests/tools/mutants.py, whose anchor rule and build this file uses unchanged: the same commands, restricted to the mutants
below.  Wrong-number mutants only — an index, a flag, a field taken for another; none removes a wait or a barrier.

    python tests/tools/mutants.py check pair_loads        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build pair_loads        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run pair_loads          (GPU box: tests/test_gpu_pair_loads.py against each build)

Each must fail tests/test_gpu_pair_loads.py (profiles/r25_pair_loads_mutants.txt):
  second_pair_loaded_at_first_pairs_index    every pair's Ei and D come from pair 0's place in the field
  second_pairs_Ei_gated_by_first_pairs_flag  pair 1's Ei is loaded, or left at +0.0, on the word of pair 0's flag
  second_pairs_D_gated_by_first_pairs_flag   the same for D
  second_pairs_Ei_and_D_swapped              pair 1's cell updates take the requested D for Ei and Ei for D"""
KIND = "csrc"
TESTS = ("tests/test_gpu_pair_loads.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("second_pair_loaded_at_first_pairs_index", "const unsigned ks = state_index<C, TT>(kq, j);", "const unsigned ks = state_index<C, TT>(kq, 0);"),
    ("second_pairs_Ei_gated_by_first_pairs_flag", "Ei2 = load_pair_unless_zero(st + S_Ei * a.fstride + ks, zold & zero_flag_bit(j, S_Ei));",
     "Ei2 = load_pair_unless_zero(st + S_Ei * a.fstride + ks, zold & zero_flag_bit(0, S_Ei));"),
    ("second_pairs_D_gated_by_first_pairs_flag", "Dk2 = load_pair_unless_zero(st + S_D * a.fstride + ks, zold & zero_flag_bit(j, S_D));",
     "Dk2 = load_pair_unless_zero(st + S_D * a.fstride + ks, zold & zero_flag_bit(0, S_D));"),
    ("second_pairs_Ei_and_D_swapped", "const double2 Ei2 = Ei2a[j], Dk2 = Dk2a[j];",
     "const double2 Ei2 = j ? Dk2a[j] : Ei2a[j], Dk2 = j ? Ei2a[j] : Dk2a[j];"),
]
