"""The tridiagonal solve and the halo exchanges of csrc/ebm_solve.h, played on the host (tests/host_solve_main.cpp, plain g++,
no HIP): a workgroup is T fibers, a scheduler owns every barrier and runs one barrier interval at a time in an order it
chooses — ascending, descending, waves reversed, lanes reversed, one straggler first or last, seeded permutations — from LDS
poisoned with NaN between guard bands.  Per case: the results and the LDS image at every barrier are the same bits under
every schedule (whole images), no NaN reaches a result, the guard bands stay as they were.  That is what sees a race between
threads that leave the same barrier, an overrun, and a read of a word nobody wrote; no GPU run can, except by luck of timing.

partition_solve_r<C, R, COMPACT>: C = 2, 4; R = 2, 4, 8 (compact with 4 and 8); every workgroup size of ebm_kernel_table.h for
R = 4 and seven of them for R = 2 and 8 (the whole product takes about 60 s of one core, the reduced one 40 s, which the
shards below divide); four families of systems, each at T C rows and at a ragged length padded with identity rows; against a
long double Thomas solve beside fp64 Thomas's own error.

Out of reach here: the kernels that call these functions — their own reuse of P0/P1 between the solve and what they do next
is theirs —, a race that writes the value already there, and the hardware's memory model.

THE EXIT CONTRACT, measured: two solves back to back in every thread pass with one barrier between them AND WITH NONE, in
every variant.  The header's "callers put a barrier before reuse" is stricter than a second solve on the same buffers needs:
on exit only the interface solution is still read (P0, compact: P1), and the next solve's first interval writes only the
other buffer (P1, compact: P0), which is exactly the header's entry rule.  A caller that writes the still-read buffer at
once IS reported in every variant (reuse-nosync): exit-side hazards are visible.  No product code changes for this."""
import os
import re
import subprocess

import pytest

from support import compile_host_program

FLAGS = ("-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off")     # only the header's explicit fma calls fuse
SHARDS = max(1, min(8, os.cpu_count() or 1))
SCHEDULES = 4 + 8 + 8            # four fixed orders, four stragglers first and last, eight seeds
VARIANTS = 10                    # C = 2, 4 times (R2 plain, R4 plain, R4 compact, R8 plain, R8 compact)
SOLVE_CASES = (4 * 16 + 6 * 7) * 8      # (variant, T) pairs times four families times two lengths
SMALL_CASES = VARIANTS * 3 * 8

# Accuracy bars: (partition error) / max(fp64 Thomas error, 1 unit), both against the long double solve in units of
# eps max|x|; four times the largest ratio of each family over the whole sweep of the unbroken header
# (profiles/r33_solve_host.txt: random 2.190, t0 7.273, imex 2.787), the margin for other compilers' contraction choices
# on the host.  The decoupled family needs no measurement: x = d * (1 / b), one reciprocal and one product, 2 units.
RATIO_BAR = {"random": 4 * 2.190, "t0": 4 * 7.273, "imex": 4 * 2.787}
DECOUPLED_BAR_UNITS = 2.0


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_host_program("host_solve_main.cpp", str(tmp_path_factory.mktemp("host_solve") / "host_solve"), FLAGS)


def play(prog, *args, shards=SHARDS):
    """The program's shards side by side: (exit statuses, output lines of all)."""
    procs = [subprocess.Popen([prog, *args, "--shard", str(i), str(shards)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for i in range(shards)]
    done = [p.communicate() + (p.returncode,) for p in procs]
    for out, err, rc in done:
        assert rc in (0, 1), (rc, out[-2000:], err[-2000:])
    return [rc for _, _, rc in done], [line for out, _, _ in done for line in out.splitlines()]


def totals(lines):
    out = {}
    for line in lines:
        w = line.split()
        if w[0] == "runs":
            assert int(w[4]) == SCHEDULES, line
            for k in (1, 5, 7, 9):
                out[w[k]] = out.get(w[k], 0) + int(w[k + 1])
    return out


def reported(lines):
    """name -> (reported, cases) of the program's per-variant lines."""
    out = {}
    for line in lines:
        m = re.fullmatch(r"reported (.+): (\d+) of (\d+)", line)
        if m:
            have = out.get(m[1], (0, 0))
            out[m[1]] = (have[0] + int(m[2]), have[1] + int(m[3]))
    return out


def reports(lines):
    return [line for line in lines if line.startswith("REPORT")][:10]


@pytest.fixture(scope="module")
def sweep(prog):
    return play(prog, "solve")


def test_partition_solve_is_the_same_under_every_schedule(sweep):
    rcs, lines = sweep
    assert not any(rcs) and not reports(lines), reports(lines)
    t = totals(lines)
    assert t["cases"] == SOLVE_CASES and t["runs"] == SOLVE_CASES * SCHEDULES and t["reported"] == 0, t
    assert t["barriers"] > 10 * t["runs"], t        # (five barriers and the reduction's levels, six with compact)


def test_partition_solve_against_extended_precision(sweep):
    _, lines = sweep
    ratio, units, cases = {}, {}, 0
    for line in lines:
        m = re.fullmatch(r"case solve .* (random|t0|decoupled|imex) (?:full|ragged) \d+: partition (\S+) thomas (\S+) ratio (\S+)", line)
        if m:
            cases += 1
            ratio[m[1]] = max(ratio.get(m[1], 0.0), float(m[4]))
            units[m[1]] = max(units.get(m[1], 0.0), float(m[2]))
    print("largest ratios:", ratio, "largest errors in units:", units)
    assert cases == SOLVE_CASES
    assert units["decoupled"] <= DECOUPLED_BAR_UNITS, units
    for family, bar in RATIO_BAR.items():
        assert ratio[family] <= bar, (family, ratio[family], bar)


def test_two_solves_back_to_back(prog):
    """With one barrier between them, as the header asks: nothing is reported.  With none: nothing either, in any variant (the
    module's docstring says why) — which is held here, because a second solve's entry rule is what makes it so."""
    for mode in ("sync", "nosync"):
        rcs, lines = play(prog, "contract", mode)
        assert not any(rcs) and not reports(lines), (mode, reports(lines))
        t, r = totals(lines), reported(lines)
        assert t["cases"] == 4 * VARIANTS and t["runs"] == 4 * VARIANTS * SCHEDULES, (mode, t)
        assert len(r) == VARIANTS and all(v == (0, 4) for v in r.values()), (mode, r)


def test_a_caller_that_reuses_the_buffer_still_read_on_exit(prog):
    """The control of the exit contract: every thread writes one word of the buffer the header says may still be read (P0,
    compact: P1) — after a barrier nothing is reported, without one every case of every variant is."""
    rcs, lines = play(prog, "contract", "reuse-sync")
    assert not any(rcs) and not reports(lines), reports(lines)
    assert all(v == (0, 4) for v in reported(lines).values()) and len(reported(lines)) == VARIANTS
    rcs, lines = play(prog, "contract", "reuse-nosync")
    r = reported(lines)
    assert len(r) == VARIANTS and all(v == (4, 4) for v in r.values()), r
    assert any(rcs)


def test_halo_exchanges_against_direct_neighbours(prog):
    """Every workgroup size, distinct values in every thread, each exchange twice in a row with its callers' barrier between
    the calls; without that barrier every case is reported but the one-wave halo_exchange_waves, which reads no LDS word."""
    rcs, lines = play(prog, "halo", "sync")
    assert not any(rcs) and not reports(lines), reports(lines)
    t = totals(lines)
    assert t["cases"] == 32 and t["runs"] == 32 * SCHEDULES and t["reported"] == 0, t
    assert reported(lines) == {"halo_exchange": (0, 16), "halo_exchange_waves": (0, 16)}
    rcs, lines = play(prog, "halo", "nosync")
    assert reported(lines) == {"halo_exchange": (16, 16), "halo_exchange_waves": (15, 16)}, reported(lines)


def test_the_play_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer (the fiber switches annotated) and UBSan — a stand-alone program: nothing is
    preloaded — over T = 64, 192, 1024, and the halo exchanges at every size."""
    san = compile_host_program("host_solve_main.cpp", str(tmp_path / "host_solve_san"),
                               FLAGS + ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rcs, lines = play(san, "solve", "--sizes", "small")
    assert not any(rcs) and not reports(lines), reports(lines)
    t = totals(lines)
    assert t["cases"] == SMALL_CASES and t["runs"] == SMALL_CASES * SCHEDULES and t["reported"] == 0, t
    rcs, lines = play(san, "halo", "sync")
    assert not any(rcs) and totals(lines)["runs"] == 32 * SCHEDULES
