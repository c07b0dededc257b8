"""CPU test of the mutation lists (tests/tools/mutants_<list>.py): every mutant's anchor still occurs exactly once in the source
it breaks.  A refactor that moves or duplicates a line silently retires the mutant that was anchored on it — ten of the
`kernels` list had gone that way before this test — and `mutants.py check` notices in a few seconds, with no build and no GPU."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_anchor_of_every_list_occurs_exactly_once():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "mutants.py"), "check"], cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out
    last = proc.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 whose anchor does not occur exactly once"), out
    assert int(last.split(" lists, ")[0]) >= 23, last
