"""Broken builds of the forcing noise's multi-wave, size-dependent and carry paths, for the mutation check of
tests/tools/mutants.py, whose anchor rule and build this file uses unchanged: the same commands, restricted to the mutants
below.  Each changes arithmetic or a predicate only — no address, no index bound, no launch shape — so a mutant computes
wrong numbers and cannot fault.

    python tests/tools/mutants.py check noise        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build noise        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run noise          (GPU box: tests/test_gpu_noise_sizes.py must fail against each build)
The verdicts below also say what tests/test_gpu_noise.py does (the noise tests as they were: 180 cells, one or two waves),
which `run` does not ask.

What each does (profiles/r18_noise_mutants.txt has the verdicts):
  noise_768_kernel_takes_the_register_sequence   miz_fused_kernel<2, ..., 768> evaluates the sequence itself although the
                                        launcher has run noise_sequence_kernel for it: N_c advances twice per launch
  integrate_sequence_kernel_only_for_one_wave    plan_step's resident plan says noise_from_memory for the SAVE kernel at 64
                                        threads only: beyond one wave ebm_integrate's resident SAVE kernel reads a
                                        row of nseq that nobody wrote.  (The term dropped altogether, as first proposed, is
                                        caught by tests/test_gpu_noise.py::test_integrate_with_noise at 64 threads.)
  sequence_lane_is_the_thread_from_the_third_wave   sequence() takes threadIdx.x, not threadIdx.x & 63, for its lane from
                                        thread 128 on: those waves draw no innovation and disagree with the first two
                                        about N_c.  (From thread 64 on, as first proposed, tests/test_gpu_noise.py catches it
                                        in its one case of two waves: 180 cells at two cells per thread are 128 threads.)
  step_counter_loses_its_high_word      noise_innovation feeds Philox the low 32 bits of the step only: steps 2^32 + k
                                        repeat steps k.  Both noise files must fail (tests/test_gpu_noise.py:
                                        test_innovations_match_the_host_restatement)"""
KIND = "csrc"
TESTS = ("tests/test_gpu_noise_sizes.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("noise_768_kernel_takes_the_register_sequence", "constexpr bool kNoiseMem = TT > kFusedRegThreads;",
     "constexpr bool kNoiseMem = TT > 768;", "ebm_miz_fused.h"),
    ("integrate_sequence_kernel_only_for_one_wave", "plan(K_MIZ_RESIDENT, 20, true)",
     "plan(K_MIZ_RESIDENT, 20, !save || T == 64)", "ebm_plan.h"),
    ("sequence_lane_is_the_thread_from_the_third_wave", "const int l = (int)(threadIdx.x & 63u);",
     "const int l = (int)(threadIdx.x < 128u ? threadIdx.x & 63u : threadIdx.x);", "ebm_noise.h"),
    ("step_counter_loses_its_high_word", "unsigned w[4] = {(unsigned)un, (unsigned)(un >> 32),", "unsigned w[4] = {(unsigned)un, 0u,",
     "ebm_noise.h"),
]
