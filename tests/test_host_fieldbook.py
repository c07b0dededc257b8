"""The handle's field book (csrc/ebm_fieldbook.h: which fields are current, which layout memory holds, whether phi is
stored) without a GPU: a stand-alone program (tests/host_fieldbook_main.cpp, plain g++, no HIP) plays the library's calls
against its own model of device memory and checks the book's answers after every call.

The walk is exhaustive: every sequence of 1 to 5 events over the program's alphabet of 20, for each of four shapes (MIZ at
four cells per thread with and without the deriving kernel, MIZ at two cells, classic) — 3 368 420 sequences per shape,
about 3 s in all at -O2.  The sanitizer leg walks depth 3."""
import os
import re
import subprocess

import pytest

from support import compile_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 5
SHAPES = ("miz4_derive", "miz4_imex", "miz2", "classic")
EVENTS = ("step_state step_diag step_save graph fused fused_diag fused_active get_prog get_diag get_T0 set_prog set_diag "
          "view_prog mean resample export import params sums_phi sums_other").split()
# the passes a shape can need: all five with the deriving kernel, the three moves without it, none with one layout
PASSES = {"miz4_derive": {"split_state", "unsplit_state", "unsplit_state_form_phi", "restore_phi", "unsplit_diag"},
          "miz4_imex": {"split_state", "unsplit_state", "unsplit_diag"}, "miz2": set(), "classic": set()}
# the calls a shape refuses whatever the state: the classic model has neither T0 nor phi
NEVER = {"classic": {"get_T0", "sums_phi"}}


def compile_program(out, extra_flags=()):
    return compile_host_program("host_fieldbook_main.cpp", out, ("-Wall",) + tuple(extra_flags))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("host_fieldbook") / "host_fieldbook"))


def walk(prog, depth):
    """The walk's counts per shape: dict(sequences, chosen, not_chosen, passes {name: n}, events {name: (played, refused)})."""
    r = subprocess.run([prog, "walk", str(depth)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "shape":
            cur = out[w[1]] = dict(sequences=int(w[3]), chosen=int(w[5]), not_chosen=int(w[7]), passes={}, events={})
        elif w[0] == "pass":
            cur["passes"][w[1]] = int(w[2])
        elif w[0] == "event":
            cur["events"][w[1]] = (int(w[2]), int(w[4]))
    return out


def check_counts(got, depth):
    """Not vacuous: every event was played, every pass the shape can need was executed (and no other), the deriving kernel
    was both chosen and refused where the handle has it and never chosen elsewhere."""
    assert tuple(got) == SHAPES
    for shape, c in got.items():
        assert c["sequences"] == sum(len(EVENTS) ** k for k in range(1, depth + 1)), shape
        assert tuple(c["events"]) == tuple(EVENTS), shape
        for ev, (played, refused) in c["events"].items():
            assert played + refused == c["sequences"] // len(EVENTS), (shape, ev)
            if ev in NEVER.get(shape, ()):
                assert played == 0, (shape, ev)
            else:
                assert played > 0, (shape, ev)
        for name, n in c["passes"].items():
            assert (n > 0) == (name in PASSES[shape]), (shape, name, n)
        assert len(c["passes"]) == 5
        assert c["not_chosen"] > 0, shape
        assert (c["chosen"] > 0) == (shape == "miz4_derive"), shape


def test_every_short_sequence_of_calls_keeps_the_book_true(prog):
    check_counts(walk(prog, DEPTH), DEPTH)


def test_the_walk_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded), depth 3."""
    san = compile_program(str(tmp_path / "host_fieldbook_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check_counts(walk(san, 3), 3)


def test_replay_prints_the_passes_and_the_conversions(prog):
    """Replay mode on a sequence whose passes DESIGN.md section 3 spells out: the first step splits; the read after two
    deriving steps un-splits forming phi; a diagnostic step splits again (phi is stored: nothing to restore) and its reader
    un-splits the diagnostic fields; a fused launch un-splits the state; a change of the parameters finds phi stored."""
    seq = "step_state step_state get_prog step_diag get_diag fused params graph".split()
    r = subprocess.run([prog, "replay", "miz4_derive", *seq], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["step_state: split_state", "step_state:", "get_prog: unsplit_state_form_phi",
                                     "step_diag: split_state", "get_diag: unsplit_diag", "fused: unsplit_state", "params:",
                                     "graph: split_state", "n_conversions 5"]
    # a stale diagnostic field is refused, and phi is restored in place for a reader of the rows as they lie
    r = subprocess.run([prog, "replay", "miz4_derive", "step_state", "get_diag", "sums_phi", "get_prog"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["step_state: split_state", "get_diag: (refused)", "sums_phi: restore_phi",
                                     "get_prog: unsplit_state", "n_conversions 2"]
    assert re.fullmatch(r"n_conversions 0\n", subprocess.run([prog, "replay", "classic"], capture_output=True, text=True).stdout)
