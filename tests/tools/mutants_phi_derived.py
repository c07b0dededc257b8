"""Broken builds of the one-step kernel that derives phi and of its runtime rule, for the mutation check of
tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged: the same commands, restricted to the
mutants below.

    python tests/tools/mutants.py check phi_derived        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build phi_derived        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run phi_derived          (GPU box: tests/test_gpu_phi_derived.py against each build)

What tests/test_gpu_phi_derived.py does with each of its 102 cases (profiles/r14_phi_derived_mutants.txt):
  phi_restore_skipped                   the un-split pass moves the stale phi field instead of forming it: every case that
                                        reads phi after a derived step fails (73)
  set_field_h_leaves_the_state_consistent   after set_field("h") (or Ei, phi) the next step derives phi from the new h
                                        instead of loading the caller's: test_a_callers_field_is_honoured (all 18), test_interleaved_calls (both)
  derived_kernel_takes_set_0s_Lf        phi of every column formed with the first parameter set's latent heat:
                                        test_launch_and_parameter_variants[two_Lf] on the three shapes, alone
  derived_phi_not_capped_in_phase_A     the cap at 1 dropped where the kernel forms phi for itself only (the shared piece,
                                        and with it every kernel that stores phi, keeps it): every case whose state has
                                        cells with -Ei / (Lf h) > 1 and derives at least once (76)"""
KIND = "csrc"
TESTS = ("tests/test_gpu_phi_derived.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("phi_restore_skipped", "return split ? Pass::SPLIT_STATE : phi_stored_ ? Pass::UNSPLIT_STATE : Pass::UNSPLIT_STATE_FORM_PHI;",
     "return split ? Pass::SPLIT_STATE : Pass::UNSPLIT_STATE;", "ebm_fieldbook.h"),
    # (every outside writer goes through this one event of the book: ebm_set_field is the one the tests reach first)
    ("set_field_h_leaves_the_state_consistent", "    void written_outside() { phi_consistent_ = false; }", "    void written_outside() {}",
     "ebm_fieldbook.h"),
    ("derived_kernel_takes_set_0s_Lf", "for (int i = 0; i < C; ++i) ph[i] = concentration(p, Ei[i], hk[i]);",
     "for (int i = 0; i < C; ++i) ph[i] = concentration(*reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p)), Ei[i], hk[i]);"),
    ("derived_phi_not_capped_in_phase_A", "for (int i = 0; i < C; ++i) ph[i] = concentration(p, Ei[i], hk[i]);",
     "for (int i = 0; i < C; ++i) ph[i] = (hk[i] == 0.0) ? 0.0 : ieee_div(-Ei[i], p.Lf * hk[i]);"),
]
