"""The step launch plan (csrc/ebm_plan.h: plan_step — which kernel family steps the columns, with how much dynamic LDS, whether
the noise sequence comes from memory, whether the diagnostics are stored pair-split; choose_launch; the 64 KiB rule of
prepare_kernels) without a GPU: a stand-alone program (tests/host_plan_main.cpp, plain g++, no HIP) prints the plan of every
variant of every geometry, and this file holds the table of rules, restated from the specification and not from the header,
and requires equality on every line.

The three MIZ kernel families compute the same bits, so no GPU test can see a wrong choice: this walk is the check."""
import os
import subprocess
from collections import Counter

import pytest

from support import compile_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, DIAG, SAVE, LOOP, LOOP_SAVE = range(5)
REG_THREADS = 512            # kFusedRegThreads (csrc/ebm_types.h)
KIB64 = 64 * 1024


def compile_program(out, extra_flags=()):
    return compile_host_program("host_plan_main.cpp", out, ("-Wall", "-Werror") + tuple(extra_flags))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("host_plan") / "host_plan"))


def expected_launch(nlat, requested):
    """(C, T): four cells per thread unless two are asked for and nlat <= 1536; whole waves; two cells beyond 512 threads: 768."""
    if nlat > 4096:
        return 0, 0
    c = 2 if requested == 2 and nlat <= 1536 else 4
    t = 64 * -(-nlat // (64 * c))
    return c, 768 if c == 2 and t > 512 else t


def expected_plan(c, t, in_lds, model, mode, phi, zero):
    """(family, LDS bytes, noise from memory, stores split) by the table of the specification; W = 8 T bytes."""
    w = 8 * t
    none = ("none", 0, 0, 0)
    if zero and not phi:
        return none
    if model == "classic":
        if phi or mode == LOOP_SAVE:             # the classic model has neither a deriving kernel nor fused sums
            return none
        return "classic", 6 * w, int(mode == LOOP), 0
    imex = model == "imex"
    if phi:
        return ("miz_step", 18 * w, 0, 1) if mode == STATE and not imex and c == 4 else none
    if mode in (STATE, DIAG, SAVE):
        return none if imex and c != 4 else ("miz_step", (6 + 3 * c) * w, 0, int(c == 4))
    if mode == LOOP:
        if imex or (c == 4 and (t > REG_THREADS or in_lds)):
            return ("miz_resident", 20 * w, 1, 0) if c == 4 else none
        if t <= 512 or (t == 768 and c == 2):
            return "miz_fused", 6 * w, int(t > REG_THREADS), 0
        return none
    assert mode == LOOP_SAVE
    if c == 4:
        return "miz_resident", 20 * w, 1, 0
    return ("miz_fused", 6 * w, 0, 0) if not imex and t <= 512 else none


def check_walk(prog):
    r = subprocess.run([prog, "walk"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    launches, plans, raises = {}, {}, {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "launch":
            launches[(int(w[1]), int(w[2]))] = (int(w[3]), int(w[4]))
        elif w[0] == "plan":
            key = (int(w[1]), int(w[2]), int(w[3]), w[4], int(w[5]), int(w[6]), int(w[7]), int(w[8]))
            assert w[9] == "->" and key not in plans, line
            plans[key] = (w[10], int(w[11]), int(w[12]), int(w[13]), int(w[14]))
        else:
            assert w[0] == "raise", line
            raises[int(w[1])] = int(w[2])

    # choose_launch: every nlat and request, and the 25 geometries
    assert launches == {(n, q): expected_launch(n, q) for n in range(2, 4098) for q in (0, 2, 4)}
    geometries = sorted(set(launches.values()) - {(0, 0)})
    assert geometries == [(2, t) for t in (*range(64, 513, 64), 768)] + [(4, t) for t in range(64, 1025, 64)]
    assert len(geometries) == 25

    # every variant of every geometry, line by line
    want = {}
    for c, t in geometries:
        for in_lds in (0, 1):
            for model in ("classic", "miz", "imex"):
                for grid in (0, 1):
                    for mode in range(5):
                        for phi in (0, 1):
                            for zero in (0, 1):
                                family, lds, mem, split = expected_plan(c, t, in_lds, model, mode, phi, zero)
                                raised = int(family != "none" and lds > KIB64)
                                want[(c, t, in_lds, model, grid, mode, phi, zero)] = (family, lds, mem, split, raised)
    assert len(want) == 25 * 2 * 3 * 2 * 5 * 4
    assert plans.keys() == want.keys()
    wrong = [(k, plans[k], want[k]) for k in want if plans[k] != want[k]]
    assert not wrong, wrong[:10]
    assert raises == {KIB64 - 1: 0, KIB64: 0, KIB64 + 1: 1}        # above 64 KiB, not from 64 KiB

    # not vacuous
    families = Counter(p[0] for p in plans.values())
    assert set(families) == {"none", "classic", "miz_step", "miz_fused", "miz_resident"}, families
    assert any(p[4] for p in plans.values()) and any(p[0] != "none" and not p[4] for p in plans.values())
    assert any(p[2] for p in plans.values() if p[0] == "miz_fused") and any(not p[2] for p in plans.values() if p[0] == "miz_fused")
    # 448 threads at four cells: only the resident kernels cross 64 KiB
    assert plans[(4, 448, 0, "miz", 0, STATE, 0, 0)] == ("miz_step", 64512, 0, 1, 0)
    assert plans[(4, 448, 1, "miz", 0, LOOP, 0, 0)] == ("miz_resident", 71680, 1, 0, 1)
    assert plans[(4, 448, 0, "miz", 0, LOOP, 0, 0)] == ("miz_fused", 21504, 0, 0, 0)
    # 768 threads at two cells: the one-step kernels cross it
    assert plans[(2, 768, 0, "miz", 0, STATE, 0, 0)] == ("miz_step", 73728, 0, 0, 1)
    assert plans[(2, 768, 0, "miz", 1, LOOP, 0, 0)] == ("miz_fused", 36864, 1, 0, 0)
    assert plans[(2, 768, 0, "miz", 1, LOOP_SAVE, 0, 0)][0] == "none"


def test_every_variant_of_every_geometry_has_the_plan_of_the_table(prog):
    check_walk(prog)


def test_the_walk_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded), the same walk."""
    check_walk(compile_program(str(tmp_path / "host_plan_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))
