"""Broken builds of ebm_export_columns / ebm_import_columns for the mutation check of tests/tools/mutants.py, whose anchor
rule and build this file uses unchanged, restricted to the mutants below.  Every mutant stays within the bounds of the
arrays and of the caller's buffer.

    python tests/tools/mutants.py check exchange        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build exchange        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run exchange          (GPU box: tests/test_gpu_exchange.py against each build)

What tests/test_gpu_exchange.py does with each is recorded in profiles/r15_exchange_mutants.txt."""
KIND = "csrc"
TESTS = ("tests/test_gpu_exchange.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    # the two halves of a pair-split row swapped: natural unit u at split unit ((u & 1) ^ 1) * T + (u >> 1)
    ("exchange_wrong_split_unit", "const int p = split ? (u & 1) * T + (u >> 1) : u;", "const int p = split ? ((u & 1) ^ 1) * T + (u >> 1) : u;"),
    # every imported column takes record 0 whatever `records` says
    ("import_ignores_records", "(a.records ? (long long)a.records[i] : i)", "(a.records ? 0LL : i)"),
    ("import_leaves_the_noise_state", "else if (a.nstate) a.nstate[col] = tail->x;", "else if (false) a.nstate[col] = tail->x;"),
    ("import_leaves_the_active_set", "        else act[u] = slot[u];\n", "        else (void)0;\n"),
    # what the exporter sent is written although the field is stale in the destination
    ("import_writes_stale_slots", "ebm::ExchangeArgs a = exchange_args(h, r, r.current, const_cast<double *>(dev_buf));",
     "ebm::ExchangeArgs a = exchange_args(h, r, mask, const_cast<double *>(dev_buf));"),
]
