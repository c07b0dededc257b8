"""Mutation check of the test suite: deliberately broken copies of the product must be caught.

    python tests/tools/mutants.py list
    python tests/tools/mutants.py check [LIST ...]        (CPU, no build; no argument: every list)
    python tests/tools/mutants.py build LIST [NAME ...]   (CPU; csrc lists only: one full build per mutant under build/)
    python tests/tools/mutants.py run   LIST [NAME ...]   (GPU box, or CPU for the host, plan, savesol and solve lists)

The lists are the data modules tests/tools/mutants_<list>.py, found by file name: KIND, TESTS (the pytest arguments that must
catch every mutant), LIMIT (seconds per pytest session) and MUTANTS, tuples (name, anchor, replacement[, file[, "survives"]]).
Each mutant is ONE small textual change — a sign, a dropped select, a broken halo — of the kind a transcription error would
be.  The anchor must occur exactly once: in the named file, or, of a 3-tuple, in all source files of the list's directory
together, and the file that holds it is the one edited.  That directory is csrc/ for KIND "csrc", whose mutants `build` compiles
from a patched copy of csrc/ into build/libebm_mut_<name>.so and `run` loads through EBM_LIB, and the package directory for
KIND "tree", whose mutants `run` patches into a temporary copy of the tree, running pytest inside the copy.  Nothing here is
product code, and no product file is ever edited in place.

`run` first runs TESTS against the unbroken product and gives no verdict unless that passes.  Then one line per mutant:
KILLED (pytest's exit status is 1 and it names a FAILED test), SURVIVED (exit status 0: a hole in the suite, unless the mutant
is marked "survives", an equivalent one kept as a control) or BROKEN (anything else — a collection error, no test ran, a
library that was not built — which says nothing about the suite).  A time limit, an abort, a segmentation fault or a GPU fault
ends the run there: nothing more is started.  Exit status 0: the baseline passed and every mutant did what its list expects.
`run LIST --oracle-free` runs the list's ORACLE_FREE arguments in place of TESTS.  The sessions' outputs are
mut_<name>.txt, the verdicts mutants_<list>.log, both in the suite's output directory (that of tests/conftest.py's
measured_errors.jsonl, git-ignored): the one place under the repository root that `run` writes to."""
import collections, glob, importlib.util, os, re, shutil, signal, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = "energybalancemodel.jl_amd"
BASE = {"csrc": os.path.join(PKG, "csrc"), "tree": PKG}
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import _ERRLOG  # noqa: E402             the suite's record of measured errors: the sessions' outputs go beside it
OUT = os.path.dirname(_ERRLOG)
NOT_COPIED = shutil.ignore_patterns(".git", "profiles", "build", os.path.basename(OUT), "__pycache__", ".pytest_cache")
TROUBLE = {124: "its time limit", 137: "a kill", 134: "an abort", 139: "a segmentation fault"}
GPU_FAULT = "an illegal memory access was encountered"


def lists():
    found = {}
    for path in sorted(glob.glob(os.path.join(HERE, "mutants_*.py"))):
        spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3], path)
        found[spec.name[len("mutants_"):]] = module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
    return found


def fields(mutant):
    return (*mutant, None, None)[:5]                # name, anchor, replacement, file, "survives"


def locate(base, old, where):
    """The file of the directory `base` that a mutant edits, or a string saying why there is none."""
    files = [where] if where else sorted(f for f in os.listdir(base) if f.endswith((".hip", ".h", ".py")))
    counts = {f: open(os.path.join(base, f)).read().count(old) for f in files}
    hits = {f: n for f, n in counts.items() if n}
    if sum(hits.values()) != 1:
        return None, f"anchor occurs {sum(hits.values())} times" + (f" ({hits})" if hits else "")
    return next(iter(hits)), None


def patch(tree, lst, mutant):
    """Apply one mutant to the copy `tree` of the repository (or of the part of it that holds the list's directory)."""
    name, old, new, where, _ = fields(mutant)
    base = os.path.join(tree, BASE[lst.KIND])
    target, why = locate(base, old, where)
    assert target is not None, (name, why)
    path = os.path.join(base, target)
    text = open(path).read()
    open(path, "w").write(text.replace(old, new))


def check(names):
    found, total, bad = lists(), 0, 0
    for key in names or found:
        lst = found[key]
        for m in lst.MUTANTS:
            target, why = locate(os.path.join(ROOT, BASE[lst.KIND]), m[1], fields(m)[3])
            if target is None:
                print(f"{key}: {m[0]}: {why}")
                bad += 1
        print(f"{key}: {len(lst.MUTANTS)} mutants")
        total += len(lst.MUTANTS)
    print(f"{len(names or found)} lists, {total} mutants, {bad} whose anchor does not occur exactly once")
    return 1 if bad else 0


def build(key, only):
    lst = lists()[key]
    assert lst.KIND == "csrc", f"{key}: a {lst.KIND} list needs no build"
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for m in lst.MUTANTS:
        if only and m[0] not in only:
            continue
        work = os.path.join(tempfile.gettempdir(), f"mutant_{m[0]}")
        shutil.rmtree(work, ignore_errors=True)
        shutil.copytree(os.path.join(ROOT, BASE["csrc"]), os.path.join(work, BASE["csrc"]), ignore=NOT_COPIED)
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, "include"))
        patch(work, lst, m)
        out = os.path.join(ROOT, "build", f"libebm_mut_{m[0]}.so")
        subprocess.check_call(["make", "-j8", "-C", os.path.join(work, BASE["csrc"]), f"OUT={out}", f"BUILD={work}/obj"],
                              stdout=subprocess.DEVNULL)
        print("built", out, flush=True)


class Trouble(Exception):
    pass


def session(tests, limit, cwd, lib, log):
    """One pytest session under its own time limit, its output in `log`: (exit status, output)."""
    env = dict(os.environ, EBM_TEST_NO_CHILDREN="1", PYTHONDONTWRITEBYTECODE="1")
    if lib:
        env["EBM_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", *tests, "-q", "-p", "no:cacheprovider"]
    with open(log, "w") as fh:
        proc = subprocess.Popen(cmd, cwd=cwd, env=env, stdout=fh, stderr=subprocess.STDOUT)
        try:
            rc = proc.wait()
        except BaseException:
            proc.terminate()                        # `timeout` hands the signal on to pytest
            proc.wait()
            raise
    text = open(log, errors="replace").read()
    rc = 128 - rc if rc < 0 else rc                 # a signal's number, as a shell would report it
    if rc in TROUBLE or GPU_FAULT in text:
        raise Trouble(f"ended on {TROUBLE[rc]} (exit status {rc})" if rc in TROUBLE else f"'{GPU_FAULT}', exit status {rc}")
    return rc, text


def in_copy(lst, mutant, tests, log):
    """A `tree` session: pytest inside a temporary copy of the tree, patched with `mutant` unless that is None."""
    tmp = tempfile.mkdtemp(prefix="ebm_mutant_")
    try:
        tree = shutil.copytree(ROOT, os.path.join(tmp, "tree"), ignore=NOT_COPIED)
        if mutant:
            patch(tree, lst, mutant)
        return session(tests, lst.LIMIT, tree, None, log)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def counts(text):
    """(failed, passed) of pytest's summary line."""
    last = next((l for l in reversed(text.splitlines()) if re.search(r"\d+ (failed|passed|skipped|deselected|errors?)\b", l)), "")
    return tuple(int((re.search(rf"(\d+) {what}", last) or [0, 0])[1]) for what in ("failed", "passed"))


def run(key, args):
    lst = lists()[key]
    oracle_free = "--oracle-free" in args
    only = [a for a in args if a != "--oracle-free"]
    tests, stem = (lst.ORACLE_FREE, "mut_anchors_") if oracle_free else (lst.TESTS, "mut_")
    unknown = set(only) - {m[0] for m in lst.MUTANTS}
    assert not unknown, f"{key} has no mutant {sorted(unknown)}"
    os.makedirs(OUT, exist_ok=True)
    report = open(os.path.join(OUT, f"mutants_{key}.log"), "w")

    def say(line):
        print(line, flush=True)
        report.write(line + "\n")
        report.flush()

    name, log = "baseline", os.path.join(OUT, f"{stem}baseline_{key}.txt")
    try:
        rc, text = in_copy(lst, None, tests, log) if lst.KIND == "tree" else session(tests, lst.LIMIT, ROOT, None, log)
        if rc != 0 or counts(text)[1] == 0:
            say(f"{key}: the baseline does not pass ({' '.join(tests)}: exit status {rc}, {counts(text)[1]} passed): no verdicts; see {log}")
            return 2
        say(f"{key}: baseline: {counts(text)[1]} passed")
        unexpected = 0
        for m in lst.MUTANTS:
            name, _, _, _, expect = fields(m)
            if only and name not in only:
                continue
            log = os.path.join(OUT, f"{stem}{name}.txt")
            lib = os.path.join(ROOT, "build", f"libebm_mut_{name}.so")
            if lst.KIND == "tree":
                rc, text = in_copy(lst, m, tests, log)
            elif os.path.exists(lib):
                rc, text = session(tests, lst.LIMIT, ROOT, lib, log)
            else:
                rc, text = None, ""
            failed = [l for l in text.splitlines() if l.startswith("FAILED ")]
            if rc == 1 and failed:
                verdict = "KILLED"
                say(f"{name}: KILLED, {'%d failed, %d passed' % counts(text)}, first: {failed[0][:140]}")
                if "-x" not in tests:
                    per_function = collections.Counter(re.split(r"[\[ ]", l.split("::")[1])[0] for l in failed)
                    for function in sorted(per_function):
                        say(f"    {per_function[function]:6d} {function}")
            elif rc == 0:
                verdict = "SURVIVED"
                say(f"{name}: SURVIVED, {counts(text)[1]} passed" + (" (equivalent by construction: expected)" if expect == "survives" else ""))
            else:
                verdict = "BROKEN"
                say(f"{name}: BROKEN, " + (f"{lib} is not built" if rc is None else f"pytest's exit status {rc} is no verdict; see {log}"))
            unexpected += verdict != ("SURVIVED" if expect == "survives" else "KILLED")
        say(f"{key}: {unexpected} of {len(only) or len(lst.MUTANTS)} mutants did not do what the list expects")
        return 1 if unexpected else 0
    except Trouble as t:
        say(f"{key}: {name}: {t}; nothing more is started; see {log}")
        return 3
    except KeyboardInterrupt:
        say(f"{key}: interrupted during {name}")
        return 130


if __name__ == "__main__":
    signal.signal(signal.SIGTERM, signal.default_int_handler)       # a runner that is ended ends its session and removes its copy
    command, args = sys.argv[1:2], sys.argv[2:]
    if command == ["list"]:
        for key, lst in lists().items():
            print(f"{key}: {lst.KIND}, {len(lst.MUTANTS)} mutants, limit {lst.LIMIT} s, pytest {' '.join(lst.TESTS)}")
            print("".join(f"    {m[0]}\n" for m in lst.MUTANTS), end="")
    elif command == ["check"]:
        sys.exit(check(args))
    elif command == ["build"] and args:
        build(args[0], args[1:])
    elif command == ["run"] and args:
        sys.exit(run(args[0], args[1:]))
    else:
        sys.exit(__doc__)
