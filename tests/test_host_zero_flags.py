"""The field book's zero-line rule (csrc/ebm_fieldbook.h: zero_flags_trusted — when the device's flags "this KiB of Ei, Ew, h
or D holds only zero bits" may be believed) without a GPU: a stand-alone program (tests/host_zero_flags_main.cpp, plain g++,
no HIP) plays the library's calls against its own model of the lines in device memory and of the eliding kernel, and checks
after every call that every flag the book trusts is true, and inside the kernel that no flagged line is taken for zero
while memory holds something else.

The walk is exhaustive: every sequence of 1 to 6 events over the program's alphabet of 13 — 5 229 042 sequences for a handle
that elides and as many for one that does not, well under a second at -O2.  The sanitizer leg walks depth 4."""
import os
import subprocess

import pytest

from support import compile_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 6
N_EVENTS = 13


def compile_program(out, extra_flags=()):
    return compile_host_program("host_zero_flags_main.cpp", out, ("-Wall", "-Werror") + tuple(extra_flags))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("host_zero_flags") / "host_zero_flags"))


def walk(prog, depth):
    r = subprocess.run([prog, "walk", str(depth)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "elide"
        out[int(w[1])] = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
    return out


def check_counts(got, depth):
    """Not vacuous: the eliding handle cleared its flags, launched the eliding kernel and the others, and the kernel skipped
    both loads and stores; the other handle never did any of that."""
    assert sorted(got) == [0, 1]
    for c in got.values():
        assert c["sequences"] == sum(N_EVENTS ** k for k in range(1, depth + 1))
    on, off = got[1], got[0]
    assert min(on["clears"], on["eliding"], on["plain"], on["skipped_stores"], on["skipped_loads"]) > 0
    assert off["clears"] == off["eliding"] == off["skipped_stores"] == off["skipped_loads"] == 0 and off["plain"] > 0


def test_every_short_sequence_of_calls_keeps_the_trusted_flags_true(prog):
    check_counts(walk(prog, DEPTH), DEPTH)


def test_the_walk_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded), depth 4."""
    san = compile_program(str(tmp_path / "host_zero_flags_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check_counts(walk(san, 4), 4)


def test_replay_prints_the_clears_and_the_trust(prog):
    """The first eliding step follows the split pass, so it clears; a steady loop clears nothing; a read un-splits (untrusted)
    and the next step clears; after set_field a graph replay takes its direct step with the kernel that loads phi and clears
    before the replay; a diagnostic step is another kernel."""
    seq = "step step get_prog step set_prog graph step_diag step step_chain0 resample step".split()
    r = subprocess.run([prog, "replay", *seq], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["step: clear trusted", "step: trusted", "get_prog: untrusted", "step: clear trusted",
                                     "set_prog: untrusted", "graph: clear trusted", "step_diag: untrusted", "step: clear trusted",
                                     "step_chain0: trusted", "resample: untrusted", "step: untrusted"]
