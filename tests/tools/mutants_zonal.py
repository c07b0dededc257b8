"""Broken builds of the zonal diffusion substep (ebm_zonal_diffusion, csrc/ebm_zonal.hip) for the mutation check of
tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.  Every mutant computes a wrong number at a
right address: each changed index stays inside the buffer the unbroken kernel addresses, no barrier or fence is touched (the
four kernels have none) and no loop bound changes.

    python tests/tools/mutants.py check zonal        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build zonal        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run zonal          (GPU box: tests/test_gpu_zonal.py against each build)

The `kernels` list has the unrolled bodies of the unsegmented sweep, one line of the reduced solve and two table lines; these
are the tail loops, the two segment kernels, the sweeps of the reduced solve and the member / segment decoding.  What
tests/test_gpu_zonal.py does with each: profiles/r37_mutants_zonal.txt.
  sweep_tail_last_row_coefficient_sign               the forward tail of zonal_sweep_kernel carries f_l = +a ep_{l-1}: seen only
                                                     where the tail runs (nlon - 2 not a multiple of 16)
  sweep_tail_back_substitution_drops_the_wrap_term   the backward tail (rows below the last full group of 16) loses ep_l W
  segment_forward_tail_spike_dropped                 u_s loses the terms P_i dp_i of the forward tail of a segment
  segment_forward_body_spike_dropped                 ... and those of the unrolled body
  segment_takes_its_own_end_for_the_left_neighbour   L = y_s in place of y_{s-1}
  segment_backward_tail_drops_the_left_term          the backward tail of a segment loses ep_l L
  segments_of_the_first_member                       every workgroup of the backward kernel decodes member 0: the other members
                                                     keep the parked dp_i in Z (and member 0 is written more than once, inside
                                                     its own rows)
  reduced_back_substitution_drops_the_wrap_term      rows S - 3 .. 0 of the reduced system lose ep_l W: needs S >= 3
  reduced_forward_last_row_coefficient_sign          the reduced system's forward sweep carries f_l = +a'' ep_{l-1}
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_zonal.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("sweep_tail_last_row_coefficient_sign", "        f = -a * E[(size_t)l * P];", "        f = a * E[(size_t)l * P];", "ebm_zonal.hip"),
    ("sweep_tail_back_substitution_drops_the_wrap_term",
     "const double U = __builtin_fma(a * M[(size_t)l * P], Un, __builtin_fma(E[(size_t)l * P], W, d[(size_t)l * P]));",
     "const double U = __builtin_fma(a * M[(size_t)l * P], Un, d[(size_t)l * P]);", "ebm_zonal.hip"),
    ("segment_forward_tail_spike_dropped", "        u = __builtin_fma(E[(size_t)i * P], dp, u);\n", "", "ebm_zonal.hip"),
    ("segment_forward_body_spike_dropped", "            u = __builtin_fma(ee[k], dp, u);\n", "", "ebm_zonal.hip"),
    ("segment_takes_its_own_end_for_the_left_neighbour", "L = sy[so + (size_t)((seg + S - 1) % S) * P];", "L = sy[so + (size_t)seg * P];",
     "ebm_zonal.hip"),
    ("segment_backward_tail_drops_the_left_term",
     "const double U = __builtin_fma(a * M[(size_t)l * P], Un, __builtin_fma(E[(size_t)l * P], L, d[(size_t)l * P]));",
     "const double U = __builtin_fma(a * M[(size_t)l * P], Un, d[(size_t)l * P]);", "ebm_zonal.hip"),
    ("segments_of_the_first_member",
     "double rtheta) {\n    const int p = blockIdx.x * blockDim.x + threadIdx.x;\n    if (p >= pitch) return;\n"
     "    const int seg = blockIdx.y % S, member = blockIdx.y / S, m = nlon / S;",
     "double rtheta) {\n    const int p = blockIdx.x * blockDim.x + threadIdx.x;\n    if (p >= pitch) return;\n"
     "    const int seg = blockIdx.y % S, member = 0, m = nlon / S;", "ebm_zonal.hip"),
    ("reduced_back_substitution_drops_the_wrap_term",
     "const double U = __builtin_fma(a2 * M[(size_t)l * P], Un, __builtin_fma(E[(size_t)l * P], W, sy[o + (size_t)l * P]));",
     "const double U = __builtin_fma(a2 * M[(size_t)l * P], Un, sy[o + (size_t)l * P]);", "ebm_zonal.hip"),
    ("reduced_forward_last_row_coefficient_sign", "        f = -a2 * E[(size_t)l * P];", "        f = a2 * E[(size_t)l * P];", "ebm_zonal.hip"),
]
