"""The savesol! schedule (csrc/ebm_savesol.h: what every step of an ebm_integrate owes its outputs, which stretches are fused,
where a raw snapshot lies in the two-half staging buffer) without a GPU: a stand-alone program (tests/host_savesol_main.cpp,
plain g++, no HIP) prints the walk of every small configuration, and this file holds the rule, restated from the reference's
text (savesol!, src/infrastructure.jl:549-591; the loop of oracle/ebm_oracle.py's integrate) and not from the header, one step
at a time, and requires equality on every line.

What the restatement adds to the reference are the wanted outputs: an output nobody wants is not taken; a step stores the
diagnostic fields only if it falls on the index of a wanted season (of either one, where the two indices coincide) or is the
run's last; the mean is formed only if sums are kept.  A step is plain if it keeps no raw snapshot, falls on no wanted
season's index and does not end a year.

On the GPU a wrong schedule shows only through tests that run whole years, on the corners their seeds draw: this walk is the
check."""
import functools
import os
import subprocess
import time
from collections import Counter

import pytest

from support import compile_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, WINTER, SUMMER = range(3)
CAP = 1 << 30


def compile_program(out, extra_flags=()):
    return compile_host_program("host_savesol_main.cpp", out, ("-Wall", "-Werror") + tuple(extra_flags))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("host_savesol") / "host_savesol"))


def output(prog, *args):
    r = subprocess.run([prog, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


@functools.lru_cache(maxsize=None)       # (a configuration is walked with and without may_fuse, and again under the sanitizers)
def restated(nt, dur, lastonly, winter, summer, raw, want_winter, want_summer, sums):
    """savesol! for tinx = 1 .. nt * dur: per step (fields of an `s` line after FIRST and SUMS, is it plain)."""
    steps = []
    for tinx in range(1, nt * dur + 1):                      # 1-based like the reference
        ti = (tinx - 1) % nt + 1                             # mod1(tinx, nt)
        year = -(-tinx // nt)                                # ceil(T[tinx]), T[tinx] = (2 tinx - 1) / (2 nt)
        dest = -1
        if raw:
            if not lastonly:
                dest = tinx - 1
            elif tinx > nt * dur - nt:
                dest = ti - 1
        season, mean = NONE, 0
        if ti == winter:
            season = WINTER
        elif ti == summer:
            season = SUMMER
        elif ti == nt:
            mean = sums
        restart = int(sums and ti == nt and season != NONE)  # no mean of this year: the next one starts from zero
        snapshot = int((ti == winter and want_winter) or (ti == summer and want_summer))
        last = int(tinx == nt * dur)
        plain = dest < 0 and not snapshot and ti != nt
        steps.append(((ti - 1, ti % nt, year, dest, season, snapshot, int(snapshot or last), last, mean, restart), plain))
    return steps


def configurations(text):
    """[(cfg, [item, ...])]; an item is ("f", first, n, sums) or ("s", first, sums, fields)."""
    out = []
    for line in text.splitlines():
        w = line.split()
        n = tuple(map(int, w[1:]))
        if w[0] == "cfg":
            out.append((n, []))
        elif w[0] == "f":
            out[-1][1].append(("f", *n))
        else:
            assert w[0] == "s", line
            out[-1][1].append(("s", n[0], n[1], n[2:]))
    return out


def check_configuration(cfg, items, seen):
    nt, dur, lastonly, winter, summer, raw, want_winter, want_summer, sums, fuse = cfg
    steps = restated(*cfg[:-1])
    at = 0
    for i, item in enumerate(items):
        assert item[1] == at, (cfg, item, "the items tile the steps in order")
        if item[0] == "s":
            _, first, with_sums, got = item
            want, plain = steps[first]
            assert got == want and with_sums == sums, (cfg, item, want)
            if fuse and plain:             # a plain step on its own: its successor is not plain, nor is its predecessor a single plain step
                assert first + 1 == len(steps) or not steps[first + 1][1], (cfg, item, "two plain steps not fused")
                assert not (i and items[i - 1][0] == "s" and steps[first - 1][1]), (cfg, item, "two plain steps not fused")
            at += 1
            if want[8] or want[9]:
                seen["mean" if want[8] else "restart"] += 1
            if want[4] == WINTER and winter == summer:
                seen["coinciding"] += 1
            if want[5] and not (want_winter if want[4] == WINTER else want_summer):
                seen["snapshot_of_the_other_season"] += 1
        else:
            _, first, n, with_sums = item
            assert fuse and 2 <= n <= CAP, (cfg, item, "fused items only with may_fuse, of two steps at least")
            assert with_sums == sums, (cfg, item, "fused items carry the sums iff they are wanted")
            assert all(plain for _, plain in steps[first:first + n]), (cfg, item, "a fused step is not plain")
            # maximal: neither the step before nor the step after could have joined
            assert first == 0 or not steps[first - 1][1], (cfg, item, "not maximal: the step before is plain")
            assert first + n == len(steps) or not steps[first + n][1], (cfg, item, "not maximal: the step after is plain")
            at += n
            seen["fused"] += 1
            if raw and lastonly and dur > 1 and first + n == nt * (dur - 1) - 1:
                seen["fused_up_to_the_year_before_the_kept_one"] += 1
            assert not (raw and (not lastonly or first >= nt * (dur - 1))), (cfg, item, "a kept step is fused")
    assert at == nt * dur, (cfg, "the items end with the run")


def check_walk(prog):
    found = configurations(output(prog, "sweep"))
    want = {(nt, dur, lastonly, winter, summer, raw, ww, ws, sums, fuse)
            for nt in range(1, 9) for dur in (1, 2, 3) for winter in range(nt + 2) for summer in range(nt + 2)
            for lastonly in (0, 1) for raw in (0, 1) for ww in (0, 1) for ws in (0, 1) for sums in (0, 1) for fuse in (0, 1)}
    assert len(found) == len(want) and {cfg for cfg, _ in found} == want
    seen = Counter()
    for cfg, items in found:
        check_configuration(cfg, items, seen)
    # not vacuous: a season on a year's last step with sums wanted (restart, no mean) and the ordinary mean; a coinciding
    # winter and summer index, also with only summer wanted; fused stretches, and under lastonly the last of them ending
    # with the year before the kept one (every step of the kept year is on its own: asserted above)
    for what in ("restart", "mean", "coinciding", "snapshot_of_the_other_season", "fused", "fused_up_to_the_year_before_the_kept_one"):
        assert seen[what] > 100, (what, seen)
    # two cases by hand.  nt = 4, two years, lastonly, everything wanted, winter on step 2, summer on the year's last step:
    by_cfg = dict(found)
    assert by_cfg[(4, 2, 1, 2, 4, 1, 1, 1, 1, 1)] == [
        ("s", 0, 1, (0, 1, 1, -1, NONE, 0, 0, 0, 0, 0)), ("s", 1, 1, (1, 2, 1, -1, WINTER, 1, 1, 0, 0, 0)),
        ("s", 2, 1, (2, 3, 1, -1, NONE, 0, 0, 0, 0, 0)), ("s", 3, 1, (3, 0, 1, -1, SUMMER, 1, 1, 0, 0, 1)),
        ("s", 4, 1, (0, 1, 2, 0, NONE, 0, 0, 0, 0, 0)), ("s", 5, 1, (1, 2, 2, 1, WINTER, 1, 1, 0, 0, 0)),
        ("s", 6, 1, (2, 3, 2, 2, NONE, 0, 0, 0, 0, 0)), ("s", 7, 1, (3, 0, 2, 3, SUMMER, 1, 1, 1, 0, 1))]
    # nt = 8, one year, sums only, indices that never match: seven steps in one launch sequence, then the year's end
    assert by_cfg[(8, 1, 1, 0, 9, 0, 0, 0, 1, 1)] == [("f", 0, 7, 1), ("s", 7, 1, (7, 0, 1, -1, NONE, 0, 1, 1, 1, 0))]


def test_every_small_configuration_walks_as_savesol_says(prog):
    check_walk(prog)


def test_long_stretches_are_computed_not_searched_for(prog):
    """The integrate benchmark's shape, 65536 steps a year for two years with the sums only: per year one stretch of nt - 1
    steps and the year's last step.  And a year longer than the cap of a stretch: the cap cuts it, nothing else does — a walk
    that tested one step at a time would take 2^30 tests to find that."""
    nt = 65536
    t0 = time.perf_counter()
    (cfg, items), = configurations(output(prog, "walk", nt, 2, 1, 0, 0, 0, 0, 0, 1, 1))
    took = time.perf_counter() - t0
    assert [item[:3] for item in items] == [("f", 0, nt - 1), ("s", nt - 1, 1), ("f", nt, nt - 1), ("s", 2 * nt - 1, 1)]
    check_configuration(cfg, items, Counter())
    nt = CAP + 5
    t0 = time.perf_counter()
    (cfg, items), = configurations(output(prog, "walk", nt, 1, 1, 0, 0, 0, 0, 0, 1, 1))
    took = max(took, time.perf_counter() - t0)
    assert items == [("f", 0, CAP, 1), ("f", CAP, 4, 1), ("s", nt - 1, 1, (nt - 1, 0, 1, -1, NONE, 0, 1, 1, 1, 0))]
    assert took < 1.0, took


def check_staging(prog):
    npitch, nvars = 7, 3
    snapshot = 8 * npitch * nvars
    blocks = []
    for line in output(prog, "staging").splitlines():
        w = line.split()
        if w[0] == "stage":
            blocks.append((tuple(map(int, w[1:])), []))
        else:
            blocks[-1][1].append((w[0], *map(int, w[1:])))
    asked = Counter()
    for (budget, p, v, nraw, chunk, total, half1, var_stride), lines in blocks:
        assert (p, v) == (npitch, nvars)
        fits = budget // snapshot
        assert chunk == min(max(fits, 1), nraw), (budget, nraw, chunk)       # at least one snapshot, at most all of them
        assert (total, half1, var_stride) == (2 * nvars * chunk * npitch, nvars * chunk * npitch, chunk * npitch)
        asked["too small" if fits < 1 else "more than nraw" if fits > nraw else "nraw" if fits == nraw else fits] += 1
        kept, flushes, pending = 0, [], []
        for line in lines:
            if line[0] == "k":
                pending.append(line[1:])
                kept += 1
                continue
            _, half, count, raw_base, dst = line
            assert half == len(flushes) % 2, (budget, nraw, line, "the halves alternate")
            assert 1 <= count <= chunk and raw_base == sum(f[1] for f in flushes), (budget, nraw, line)
            assert dst == (nvars - 1) * nraw + raw_base
            # every kept step since the last flush lies in this half, one after the other
            assert pending == [(half, i, i * npitch) for i in range(count)], (budget, nraw, line, pending)
            # after every chunk-th kept step, and once at the end
            assert count == chunk or kept == nraw, (budget, nraw, line)
            flushes.append((half, count))
            pending = []
        assert not pending and kept == nraw and sum(f[1] for f in flushes) == nraw, (budget, nraw)
        assert len(flushes) == -(-nraw // chunk)
    assert {nraw for (_, _, _, nraw, *_), _ in blocks} == set(range(1, 21))
    assert set(asked) >= {"too small", 1, 2, 3, "nraw", "more than nraw"}, asked
    assert any(len(lines) - b[3] > 2 for b, lines in blocks)                 # a half is used again


def test_raw_staging_slots_and_flushes(prog):
    check_staging(prog)


def test_the_walk_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded), the same checks."""
    san = compile_program(str(tmp_path / "host_savesol_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    check_walk(san)
    check_staging(san)
