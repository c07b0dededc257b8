"""The first Newton pass of the one-step kernels as csrc/ebm_miz_step.h strings it together, played on the host
(tests/host_step_lds_main.cpp, plain g++, no HIP): halo_exchange_two (r and the masked g behind one barrier), the kernel's
second barrier, the solve, publish_then_vote (Tbar's halo published before the vote and read after it), and, where the vote
said "again", a second pass with the plain g exchange — under the schedules of tests/host_solve_main.cpp, whose scheduler,
poisoned LDS and verdicts are compiled into the program unedited (its main renamed), with every LDS word poisoned again once
the kernel's order says it is dead.

This is the part that tests/test_host_solve.py names as out of its reach: the kernel's own reuse of P0 / P1 between the solve
and what follows.  Still out of reach: the pointwise physics (r, h, Tw are data here), a race that writes the value already
there, and the hardware's memory model.

The shipped order reports nothing at T = 64, 128, 192, 320, 1024, with one pass and with two.  Three orders that the kernel's
comments argue against are each reported in every case:
    no-second-barrier   the barrier between halo_exchange_two and the solve left out: the chunk summary W1[t] = P1[t] races
                        the neighbour's read of g's last value
    read-before-vote    Tbar's words read before the vote's barrier
    tbar-in-p0          Tbar's words written into P0, over the interface solution Y that other threads still read
"""
import re
import subprocess

import pytest

from support import compile_host_program

FLAGS = ("-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off")     # only the header's explicit fma calls fuse
SIZES = 5                        # T = 64, 128, 192, 320, 1024
CASES = 2 * SIZES                # each with one pass and with two
SCHEDULES = 4 + 8 + 8            # four fixed orders, four stragglers first and last, eight seeds
BROKEN = ("no-second-barrier", "read-before-vote", "tbar-in-p0")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_host_program("host_step_lds_main.cpp", str(tmp_path_factory.mktemp("host_step_lds") / "host_step_lds"), FLAGS)


def play(prog, order):
    """(exit status, reported cases, cases, runs, REPORT lines)"""
    p = subprocess.run([prog, "play", order], capture_output=True, text=True)
    assert p.returncode in (0, 1), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    m = [re.fullmatch(r"reported step: (\d+) of (\d+)", line) for line in lines]
    m = [x for x in m if x]
    t = [line.split() for line in lines if line.startswith("runs ")]
    assert len(m) == 1 and len(t) == 1 and int(t[0][4]) == SCHEDULES, lines[-5:]
    return p.returncode, int(m[0][1]), int(m[0][2]), int(t[0][6]), [line for line in lines if line.startswith("REPORT")]


def test_the_shipped_order_is_the_same_under_every_schedule(prog):
    rc, reported, cases, runs, reports = play(prog, "shipped")
    assert rc == 0 and not reports, reports[:10]
    assert (reported, cases, runs) == (0, CASES, CASES * SCHEDULES)


@pytest.mark.parametrize("order", BROKEN)
def test_a_broken_order_is_reported_in_every_case(prog, order):
    """The controls: each hazard shows as a result or an LDS image that depends on the schedule, at every size, with one pass
    and with two."""
    rc, reported, cases, _, reports = play(prog, order)
    assert rc == 1 and (reported, cases) == (CASES, CASES), (order, reported, cases)
    assert len(reports) == CASES and all("schedule" in r for r in reports), reports[:10]


def test_the_play_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer (the fiber switches annotated) and UBSan — a stand-alone program: nothing is
    preloaded."""
    san = compile_host_program("host_step_lds_main.cpp", str(tmp_path / "host_step_lds_san"),
                               FLAGS + ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rc, reported, cases, runs, reports = play(san, "shipped")
    assert rc == 0 and not reports and (reported, cases, runs) == (0, CASES, CASES * SCHEDULES), reports[:10]
    for order in BROKEN:
        rc, reported, cases, _, _ = play(san, order)
        assert rc == 1 and (reported, cases) == (CASES, CASES), order
