"""Host test (no GPU): the order of requests at the head of phase A of the headline's one-step kernel,
miz_step_kernel<4, sin, OUT_STATE, 1024, false, true, true> (csrc/ebm_miz_step.h), read in its gfx950 assembly.  hipcc
cross-compiles the one instantiation in a few seconds; skipped where there is no hipcc.

The order is easy to lose — one new line above the loads brings the chain of dependent scalar loads back — and nothing else
sees it: results are the same either way ("a phase requests its inputs before anything that waits or writes")."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "energybalancemodel.jl_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def makefile_flags():
    """FLAGS of csrc/Makefile, for gfx950 and without EXTRA: what the library's kernels are compiled with."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(l for l in f if l.startswith("FLAGS ="))
    flags = line.split("=", 1)[1].replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags and "-ffp-contract=off" in flags, flags
    return flags


UNIT = ('#include "ebm_miz_step.h"\n'
        "template __global__ void ebm::miz_step_kernel<4, 1, ebm::OUT_STATE, 1024, false, true, true>(const ebm::StepArgs);\n")

pytestmark = pytest.mark.skipif(HIPCC is None, reason="no hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """The instructions of the kernel, one per entry, labels, directives and comments dropped."""
    d = tmp_path_factory.mktemp("step_head")
    src, out = str(d / "headline.hip"), str(d / "headline.s")
    with open(src, "w") as f:
        f.write(UNIT)
    subprocess.run([HIPCC, *makefile_flags(), "-I", CSRC, "-S", "--cuda-device-only", "-o", out, src], check=True, capture_output=True)
    lines = []
    with open(out) as f:
        for line in f:
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                lines.append(line)
    end = next(i for i, l in enumerate(lines) if l.startswith("s_endpgm"))
    return lines[:end]


def first(lines, prefix, start=0):
    return next(i for i in range(start, len(lines)) if lines[i].startswith(prefix))


def test_two_scalar_waits_before_the_first_state_load(asm):
    """At most two s_waitcnt lgkmcnt precede the first global_load_dwordx4: the kernel arguments, and the batch with the wave's
    own flag word."""
    head = asm[:first(asm, "global_load_dwordx4")]
    waits = [l for l in head if l.startswith("s_waitcnt") and "lgkmcnt" in l]
    assert len(waits) <= 2, waits
    assert not any(l.startswith("global_load") for l in head), "the mask word or a table is requested before the state"


def test_state_then_mask_then_tables(asm):
    """Phase A's vector requests, all before the workgroup's first barrier: six 16-byte loads of the state (two pairs of Ew, Ei,
    h), each behind the branch on its zero-line flag — that is how a state load is told from a table's —, then the mask word,
    then six loads of the tables (lo, up, x) with no branch among them."""
    phase_a = asm[:first(asm, "s_barrier")]
    loads = [i for i, l in enumerate(phase_a) if l.startswith("global_load")]
    kinds = [phase_a[i].split()[0] for i in loads]
    assert kinds == ["global_load_dwordx4"] * 6 + ["global_load_ushort"] + ["global_load_dwordx4"] * 6, kinds

    def branches(lo, hi):
        return sum(l.startswith("s_cbranch") for l in phase_a[lo:hi])
    previous = 0
    for i in loads[:6]:
        assert branches(previous, i) >= 1, ("a load that no flag guards stands among the state's", phase_a[i])
        previous = i
    assert branches(loads[7], loads[12]) == 0, "the tables are requested in one run, unconditionally"
