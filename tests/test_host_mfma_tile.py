"""The dense tile that the covariance, the update and the gain share (csrc/ebm_mfma_tile.h), played on the host
(tests/host_mfma_tile_main.cpp, plain g++, no HIP: it sees only the constexpr part of the header — the lane map, the operand
map, the D map and the two LDS accessors).

    coverage   over 256 lanes x 2 x 2 accumulators x 4 registers the D map hits every cell of the 64 x 64 tile exactly once
    play       one workgroup on small distinct integers: operands through the header's operand map from a line-major and from
               a k-major LDS image (padding poisoned), the instruction as the header's one comment states it, results through
               the D map; equal to the plain triple loop for 1, 2, 3 and 4 groups issued.  Integers: exact, no tolerance.

What this cannot see.  Whether the header's comment matches the hardware: the program restates the instruction from that
sentence, so a sentence that is wrong about v_mfma_f64_16x16x4_f64 plays consistently here — the exact integer cases of
tests/test_gpu_ensemble_cov.py, test_gpu_update_columns.py and test_gpu_kalman_gain.py hold that, on the GPU.  Anything about
the three kernels' staging into LDS, their tails, rule 6 or their stores: the images here are filled by the program.  And the
device part of the header (the builtin's argument order, the unrolling), which no host compiler reads."""
import re
import subprocess

import pytest

from support import compile_host_program

FLAGS = ("-Wall", "-Werror")
LAYOUTS = ("line-major", "k-major")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_host_program("host_mfma_tile_main.cpp", str(tmp_path_factory.mktemp("host_mfma_tile") / "host_mfma_tile"), FLAGS)


def play(prog, *control):
    """(exit status, {(layout, groups): wrong cells})"""
    p = subprocess.run([prog, "play", *control], capture_output=True, text=True)
    assert p.returncode in (0, 1), (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    m = [re.fullmatch(r"play (\S+) groups (\d) wrong (\d+)", line) for line in p.stdout.splitlines()]
    assert m and all(m), p.stdout[-2000:]
    return p.returncode, {(x[1], int(x[2])): int(x[3]) for x in m}


def test_the_d_map_covers_the_tile_exactly_once(prog):
    p = subprocess.run([prog, "coverage"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.split() == "coverage results 4096 outside 0 cells 4096 once 4096".split()


def test_a_played_workgroup_is_the_triple_loop(prog):
    rc, wrong = play(prog)
    assert wrong == {(layout, groups): 0 for layout in LAYOUTS for groups in (1, 2, 3, 4)} and rc == 0, wrong


def test_the_f32_row_formula_is_caught(prog):
    """The control: D restated as the f32 instructions hold it, (l >> 4) * 4 + g — which the hardware runs clean on fp64
    and which puts three of every four results in a wrong row — is wrong in both layouts at every group count."""
    rc, wrong = play(prog, "f32-rows")
    assert rc == 1 and set(wrong) == {(layout, groups) for layout in LAYOUTS for groups in (1, 2, 3, 4)}
    assert all(n == 64 * 64 * 3 // 4 for n in wrong.values()), wrong


def test_the_play_under_the_sanitizers(tmp_path):
    """The same program with AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)."""
    san = compile_host_program("host_mfma_tile_main.cpp", str(tmp_path / "host_mfma_tile_san"),
                               FLAGS + ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert subprocess.run([san, "coverage"], capture_output=True).returncode == 0
    rc, wrong = play(san)
    assert rc == 0 and not any(wrong.values()), wrong
