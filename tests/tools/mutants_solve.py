"""Mutation check of the tridiagonal solve and the halo exchanges (csrc/ebm_solve.h) against their play on the host:
    python tests/tools/mutants.py run solve                (CPU; no GPU, no build of the library)
Each mutant is one textual change of the header in a temporary copy of the tree; tests/test_host_solve.py must fail there.
The races among them — two threads that leave the same barrier, one reading what the other writes — pass every GPU test by
luck of timing (tests/tools/mutants_kernels.py tried two and gave them up); the host play runs the threads of a barrier
interval one after the other in many orders and sees the result depend on the order.  profiles/r33_solve_mutants.txt has the
verdicts.

Every barrier of the header is removed once.  None of these mutants survives: no barrier of the solve or of the exchanges is
redundant under the schedules played.  (The barrier that callers are told to put before reusing P0/P1 is theirs and is not
in the header: test_two_solves_back_to_back records that a second solve on the same buffers does not need it.)"""
KIND = "tree"
TESTS = ("tests/test_host_solve.py", "-x")
LIMIT = 600
H = "csrc/ebm_solve.h"
MUTANTS = [
    # the two races the main list abandoned: the reduction's second buffer over the last third of the first (compact, plain),
    # and the interface solution written into the buffers the reduction's last level is read from
    ("compact_reduction_buffers_overlap_by_a_third", "*S1 = COMPACT ? P0 + 3 * G : P1;", "*S1 = COMPACT ? P0 + 2 * G : P1;", H),
    ("plain_reduction_buffers_overlap_by_a_third", "*S1 = COMPACT ? P0 + 3 * G : P1;", "*S1 = COMPACT ? P0 + 3 * G : P1 + G;", H),
    ("interface_solution_into_the_reductions_buffer", "double *const Y = COMPACT ? P1 : P0;", "double *const Y = COMPACT ? P0 : P1;", H),
    # every barrier of partition_solve_r, in the order of the text
    ("no_barrier_after_the_chunk_summaries", "    W1[2 * T + t] = wr;\n    __syncthreads();\n", "    W1[2 * T + t] = wr;\n", H),
    ("no_barrier_before_the_compact_rows", "    if (COMPACT) __syncthreads();", "    ;", H),
    ("no_barrier_after_the_interface_rows", "        P0[2 * T + q * G + g] = pd;\n    }\n    __syncthreads();\n", "        P0[2 * T + q * G + g] = pd;\n    }\n", H),
    ("no_barrier_after_the_second_level_summaries", "        U[2 * G + t] = w2;\n    }\n    __syncthreads();\n", "        U[2 * G + t] = w2;\n    }\n", H),
    ("no_barrier_before_the_reduction", "        S0[2 * G + t] = qd;\n    }\n    __syncthreads();\n", "        S0[2 * G + t] = qd;\n    }\n", H),
    ("no_barrier_between_reduction_levels", "            dst[2 * G + t] = qd;\n        }\n        __syncthreads();\n", "            dst[2 * G + t] = qd;\n        }\n", H),
    ("no_barrier_after_the_interface_solution", "    __syncthreads();\n    pd = Y[", "    pd = Y[", H),
    # ... and of the exchanges
    ("halo_exchange_without_its_barrier", "    E1[t] = last;\n    __syncthreads();\n", "    E1[t] = last;\n", H),
    ("wave_halo_without_its_barrier", "    if (lane == 0) E[16 + w] = first;\n    __syncthreads();\n", "    if (lane == 0) E[16 + w] = first;\n", H),
    # buffers in the wrong place: the reduction's first buffer over the last third of the second-level summaries (read by
    # the neighbour in the interval that writes it), and a third too far (R = 2: past the end of P1, into the guard band)
    ("reduction_first_buffer_over_the_summaries", "*S0 = COMPACT ? P0 : P1 + 3 * G,", "*S0 = COMPACT ? P0 : P1 + 2 * G,", H),
    ("reduction_first_buffer_past_the_end_of_P1", "*S0 = COMPACT ? P0 : P1 + 3 * G,", "*S0 = COMPACT ? P0 : P1 + 4 * G,", H),
    # reads of words nobody wrote: the guard bands and the poison are NaN, and NaN times the exact zero is NaN
    ("reduction_neighbours_unclamped", "const int im = t - s >= 0 ? t - s : t, ip = t + s < G ? t + s : t;", "const int im = t - s, ip = t + s;", H),
    # (the last thread's own summary in place of zero: seen because the random family leaves c of the last row as drawn)
    ("next_chunk_summary_not_zeroed_past_the_meridian", "    un = has_next ? un : 0.0;\n", "", H),
    # plain algebra, as in the main list
    ("partition_interface_row_sign", "const double RB = __builtin_fma(ce, vn, __builtin_fma(-ae, cp[C - 2], be));",
     "const double RB = __builtin_fma(ce, vn, __builtin_fma(ae, cp[C - 2], be));", H),
    ("second_level_left_coupling_sign", "lq[i] = -(a2[i] * lq[i - 1]) * w;", "lq[i] = (a2[i] * lq[i - 1]) * w;", H),
    ("cyclic_reduction_lower_sign", "const double nqa = -(qa * am) * r;", "const double nqa = (qa * am) * r;", H),
]
