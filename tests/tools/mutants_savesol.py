"""Mutation check of the savesol! schedule (csrc/ebm_savesol.h) against its host test: python tests/tools/mutants.py run savesol
Each mutant is one textual change of the header in a temporary copy of the tree; tests/test_host_savesol.py must fail there.  On
the GPU these show only through tests that run whole years, on the corners their seeds happen to draw.  One line per mutant:
KILLED by <first failing test> or SURVIVED (profiles/r28_savesol_mutants.txt has the verdicts)."""
KIND = "tree"
TESTS = ("tests/test_host_savesol.py", "-x")
LIMIT = 300
MUTANTS = [
    ("summer_tested_before_winter", "if (ti == c.winter_inx) s.season = SEASON_WINTER;\n    else if (ti == c.summer_inx) s.season = SEASON_SUMMER;",
     "if (ti == c.summer_inx) s.season = SEASON_SUMMER;\n    else if (ti == c.winter_inx) s.season = SEASON_WINTER;", "csrc/ebm_savesol.h"),
    ("mean_also_on_a_seasonal_year_end", "    else if (ti == c.nt) s.mean = c.want_sums;", "    if (ti == c.nt) s.mean = c.want_sums;", "csrc/ebm_savesol.h"),
    ("sums_not_restarted_on_a_seasonal_year_end", "s.restart = c.want_sums && ti == c.nt && s.season != SEASON_NONE;", "s.restart = false;",
     "csrc/ebm_savesol.h"),
    ("raw_kept_from_the_step_before_the_last_year", "tinx > c.total() - c.nt ? ti - 1 : -1;", "tinx >= c.total() - c.nt ? ti - 1 : -1;", "csrc/ebm_savesol.h"),
    ("lastonly_raw_indexed_by_tinx", "tinx > c.total() - c.nt ? ti - 1 : -1;", "tinx > c.total() - c.nt ? tinx - 1 : -1;", "csrc/ebm_savesol.h"),
    ("two_plain_steps_not_fused", "it.n = plain >= 2 ? plain : 1;", "it.n = plain >= 3 ? plain : 1;", "csrc/ebm_savesol.h"),
    ("kept_steps_fused", "    if (save_step(c, tinx).raw_index >= 0) return tinx;\n", "", "csrc/ebm_savesol.h"),
    ("stretch_runs_through_a_wanted_season", "if (wanted && inx >= 1", "if (!wanted && inx >= 1", "csrc/ebm_savesol.h"),
    ("stretch_runs_through_a_year_end", "long long e = before + c.nt;", "long long e = c.total();", "csrc/ebm_savesol.h"),
    ("season_of_last_year_ends_this_stretch", "&& before + inx >= tinx) e =", ") e =", "csrc/ebm_savesol.h"),
    ("snapshot_of_an_unwanted_season", "(ti == c.winter_inx && c.want_winter) ||", "(ti == c.winter_inx) ||", "csrc/ebm_savesol.h"),
    ("stretch_longer_than_the_cap", "std::min(next_event(c, tinx) - tinx, kMaxStretch)", "(next_event(c, tinx) - tinx)", "csrc/ebm_savesol.h"),
    ("chunk_not_clamped_to_nraw", "        if (chunk_ > nraw_) chunk_ = nraw_;\n", "", "csrc/ebm_savesol.h"),
    ("chunk_of_no_snapshot", "        if (chunk_ < 1) chunk_ = 1;\n", "", "csrc/ebm_savesol.h"),
    ("half_not_toggled", "        half_ ^= 1;\n", "", "csrc/ebm_savesol.h"),
    ("raw_base_not_advanced", "        raw_base_ += staged_;\n", "", "csrc/ebm_savesol.h"),
    ("flush_one_kept_step_late", "return ++staged_ == chunk_ && flush(f);", "return staged_++ == chunk_ && flush(f);", "csrc/ebm_savesol.h"),
]
