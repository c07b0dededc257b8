"""Broken builds of the column scalars (ebm_column_scalars, csrc/ebm_launch.hip: column_scalar) for the mutation check of
tests/tools/mutants.py, whose list, anchor rule and build this file uses unchanged.

    python tests/tools/mutants.py check scalars        (CPU: every anchor occurs exactly once)
    python tests/tools/mutants.py build scalars        (CPU: one full build per mutant under build/)
    python tests/tools/mutants.py run scalars          (GPU box: tests/test_gpu_column_scalars.py against each build)

  edge_hit_is_strict              `>` / `<` for `>=` / `<=`: a level equal to a cell value (the crafted columns' first hit cell holds
                                  the level to the bit) is passed by
What tests/test_gpu_column_scalars.py does with each: profiles/r29_scalars_mutants.txt (all five killed).
  edge_interpolates_one_cell_on   a and b taken from K and K + 1
  band_ends_one_cell_early        the last cell of every band is not searched: a first hit at k1 becomes "no edge"
  edge_takes_the_last_hit         the cross-lane reduction keeps the later of two hits
  no_edge_is_nan                  NaN for +Inf: the ice-free column, and the member that crosses through +Inf, which then never does
"""
KIND = "csrc"
TESTS = ("tests/test_gpu_column_scalars.py", "-m", "gpu")
LIMIT = 300
MUTANTS = [
    ("edge_hit_is_strict", "return kind == S_EDGE_GE ? v >= level : v <= level;", "return kind == S_EDGE_GE ? v > level : v < level;"),
    ("edge_interpolates_one_cell_on", "const double a = f[K - 1], b = f[K];", "const double a = f[K], b = f[K < k1 ? K + 1 : K];"),
    ("band_ends_one_cell_early", "v[u] = k <= k1 ? f[k] : __builtin_nan(\"\");", "v[u] = k < k1 ? f[k] : __builtin_nan(\"\");"),
    ("edge_takes_the_last_hit", "__device__ __forceinline__ int earlier_hit(int a, int b) { return a < b ? a : b; }",
     "__device__ __forceinline__ int earlier_hit(int a, int b) { return a == kNoHit ? b : b == kNoHit ? a : a > b ? a : b; }"),
    ("no_edge_is_nan", "if (K == kNoHit) return __builtin_inf();", "if (K == kNoHit) return __builtin_nan(\"\");"),
]
