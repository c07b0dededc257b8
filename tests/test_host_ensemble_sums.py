"""CPU tests of the weighted ensemble sums (ebm_ensemble_sums): the NumPy restatement of the definition against exact sums,
the arithmetic from sums to moments, the sharded sums against the unsharded ones within the stated bound, the all-reduce
path of EnsembleRun.moments over two gloo ranks with a stand-in for the engine, and the symbols in the header, the library
and the bindings.

The bounds are derived, not fitted.  The terms t0 = w, t1 = w d, t2 = (w d) d are float64 numbers that the definition fixes
to the bit; what differs between two ways of adding them is the rounding of the adds alone.  A term of a call over m columns
passes through at most D(m) = min(m, 32) + ceil(m / 32) - 2 rounded adds (adds_per_term: inside its block, then over the
blocks; an add to 0.0 is exact), so that call's sum is within gamma(D(m)) sum|terms| of the exact sum of its terms, gamma(D) =
D 2^-53 / (1 - D 2^-53).  math.fsum rounds the exact sum once more: + 2^-53 sum|terms|.  Adding the sums of n shards in
rank order puts n - 1 more rounded adds on top of the deepest shard's.  Hence
    |restatement - fsum|     <= gamma(D(ncol) + 1) sum|terms|
    |sharded - unsharded|    <= gamma(D(ncol) + max_r D(ncol_r) + n - 1) sum|terms|
The figure (n - 1) 2^-53 sum|terms| that the feature's issue gives for the second line does not hold: it counts the combining
adds only, and the shards' boundaries are not block boundaries, so the two sides also differ by their own roundings (33
columns on 2 shards: 3.4 2^-53 sum|terms| on this file's data)."""
import ctypes
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from ensemble_sums_ref import abs_term_sums, adds_per_term, ensemble_sums_ref, gamma, same_bits

U = 2.0 ** -53
NAMES = ("ebm_ensemble_sums", "ebm_ensemble_sums_device")


def benign(nvars, ncol, nlat, seed):
    """Finite data of mixed sign over a few binades, some NaN cells, weights with zeros and negative entries, a center."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (nvars, ncol, nlat)) * 2.0 ** rng.integers(-3, 4, (nvars, ncol, nlat))
    x[rng.random(x.shape) < 0.05] = np.nan
    w = rng.uniform(-0.5, 2.0, ncol)
    w[rng.random(ncol) < 0.2] = 0.0
    center = rng.normal(0.0, 0.5, (nvars, nlat))
    return x, w, center


def exact_sums(x, w, center):
    """The three sums with exactly rounded totals (math.fsum) of the float64 terms as the definition rounds them."""
    nvars, ncol, nlat = x.shape
    out = np.zeros((nvars, 3, nlat))
    for v in range(nvars):
        for k in range(nlat):
            t = [[], [], []]
            for c in range(ncol):
                if w[c] == 0.0 or math.isnan(x[v, c, k]):
                    continue
                d = x[v, c, k] - (center[v, k] if center is not None else 0.0)
                t[0].append(w[c]); t[1].append(w[c] * d); t[2].append((w[c] * d) * d)
            out[v, :, k] = [math.fsum(q) for q in t]
    return out


@pytest.mark.parametrize("ncol", [1, 31, 32, 33, 97])
def test_restatement_against_fsum(ncol):
    x, w, center = benign(2, ncol, 7, 10 + ncol)
    for ww, cc in ((None, None), (w, None), (w, center), (None, center)):
        got = ensemble_sums_ref(x, ww, cc)
        want = exact_sums(x, np.ones(ncol) if ww is None else ww, cc)
        bound = gamma(adds_per_term(ncol) + 1) * abs_term_sums(x, ww, cc)
        assert (np.abs(got - want) <= bound).all(), (ncol, float(np.max(np.abs(got - want) - bound)))
    # unit weights, no NaN, integers: every sum is exact, whatever the order
    xi = np.random.default_rng(1).integers(-9, 10, (1, ncol, 5)).astype(np.float64)
    got = ensemble_sums_ref(xi)
    assert np.array_equal(got[0, 0], np.full(5, float(ncol))) and np.array_equal(got[0, 1], xi[0].sum(axis=0))
    assert np.array_equal(got[0, 2], (xi[0] ** 2).sum(axis=0))


def test_restatement_rules():
    """NaN cells and zero weights do not contribute, Inf propagates, a zero weight hides an Inf, no contributor gives 0.0."""
    x = np.array([[[1.0, np.nan, np.inf, -0.0, np.nan], [2.0, np.nan, 1.0, -0.0, 3.0], [4.0, np.nan, np.inf, -0.0, np.nan]]])
    s = ensemble_sums_ref(x)
    assert s[0, 0].tolist() == [3.0, 0.0, 3.0, 3.0, 1.0] and s[0, 1].tolist()[:2] == [7.0, 0.0] and s[0, 1, 2] == np.inf
    assert s[0, 1, 3] == 0.0 and not np.signbit(s[0, 1, 3]), "0.0 + -0.0 is +0.0"
    s = ensemble_sums_ref(x, np.array([0.0, 2.0, 0.0]))
    assert s[0, 0].tolist() == [2.0, 0.0, 2.0, 2.0, 2.0] and s[0, 1].tolist() == [4.0, 0.0, 2.0, 0.0, 6.0]
    assert np.isfinite(s).all(), "the members with the Inf cell have weight 0"
    s = ensemble_sums_ref(x, np.array([1.0, 1.0, -1.0]), np.array([[1.0, 0.0, 0.0, 0.0, 1.0]]))
    assert s[0, 0, 0] == 1.0 and s[0, 1, 0] == (0.0 + 1.0) - 3.0 and s[0, 2, 0] == (0.0 + 1.0) - 9.0
    assert np.isnan(s[0, 1, 2]), "Inf - Inf"


def test_moments_from_sums_known_answers(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    x = np.array([[[1.0, 5.0, np.nan], [3.0, 5.0, np.nan], [5.0, np.nan, np.nan], [7.0, 5.0, np.nan]]])       # [1, 4, 3]
    s1 = ensemble_sums_ref(x)
    m = pkg.moments_from_sums(s1)
    assert m["weight"][0].tolist() == [4.0, 3.0, 0.0] and m["mean"][0, :2].tolist() == [4.0, 5.0] and np.isnan(m["mean"][0, 2])
    assert "var" not in m
    center = ensemble.moments_center(m["mean"])
    assert center[0].tolist() == [4.0, 5.0, 0.0]
    m = pkg.moments_from_sums(s1, ensemble_sums_ref(x, None, center))
    assert m["var"][0, :2].tolist() == [5.0, 0.0] and np.isnan(m["var"][0, 2]) and np.isnan(m["mean"][0, 2])
    # weights: the mean of the members 1 and 3 only; a weight of 3 counts a member three times
    s1 = ensemble_sums_ref(x, np.array([0.0, 1.0, 0.0, 3.0]))
    m = pkg.moments_from_sums(s1)
    assert m["weight"][0].tolist() == [4.0, 4.0, 0.0] and m["mean"][0, 0] == 6.0
    m = pkg.moments_from_sums(s1, ensemble_sums_ref(x, np.array([0.0, 1.0, 0.0, 3.0]), ensemble.moments_center(m["mean"])))
    assert m["var"][0, 0] == 3.0                                   # (9 + 3 * 1) / 4
    # S0 == 0 with S1 != 0 (weights that cancel): NaN, not Inf
    m = pkg.moments_from_sums(ensemble_sums_ref(x[:, :2, :1], np.array([1.0, -1.0])))
    assert np.isnan(m["mean"]).all()
    with pytest.raises(ValueError):
        pkg.moments_from_sums(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError):
        pkg.moments_from_sums(np.zeros((2, 3, 3)), np.zeros((1, 3, 3)))


@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("ncol", [33, 97, 130])
def test_sharded_sums_within_the_stated_bound(pkg, ncol, nshards):
    """The per-shard restatement sums, added in rank order, against the unsharded sums: another order of the same terms,
    within the bound of the module docstring; and the sharded sums against the exact sum of the terms."""
    x, w, center = benign(2, ncol, 9, 7 * ncol + nshards)
    sizes = [pkg.shard_columns(ncol, nshards, r) for r in range(nshards)]
    deepest = max(adds_per_term(sl.stop - sl.start) for sl in sizes)
    for ww, cc in ((None, None), (w, center)):
        whole = ensemble_sums_ref(x, ww, cc)
        parts = np.zeros_like(whole)
        for sl in sizes:
            parts = parts + ensemble_sums_ref(x[:, sl], None if ww is None else ww[sl], cc)
        scale = abs_term_sums(x, ww, cc)
        assert (np.abs(parts - whole) <= gamma(adds_per_term(ncol) + deepest + nshards - 1) * scale).all()
        exact = exact_sums(x, np.ones(ncol) if ww is None else ww, cc)
        assert (np.abs(parts - exact) <= gamma(deepest + nshards - 1 + 1) * scale).all()
    # the combining adds alone do not bound it: the figure (n - 1) 2^-53 sum|terms| is exceeded on this data
    if (ncol, nshards) == (33, 2):
        x, _, _ = benign(2, ncol, 9, 7 * ncol + nshards)
        whole = ensemble_sums_ref(x)
        parts = ensemble_sums_ref(x[:, :17]) + ensemble_sums_ref(x[:, 17:])
        assert (np.abs(parts - whole) > (nshards - 1) * U * abs_term_sums(x)).any()


def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert "WEIGHTED SUMS ACROSS THE MEMBERS" in hdr and hdr.count("THIS TEXT IS THE DEFINITION") >= 7
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    julia = open(os.path.join(ROOT, "julia", "EBMHip.jl")).read()
    protos = {}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, bare)
        assert m, f"include/ebm_hip.h does not declare {name}"
        protos[name] = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert len(protos[name]) == 6, name
        assert name in pkg.EXPORTS and hasattr(cdll, name)
        assert len(getattr(lib, name).argtypes) == 6, name
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name
    # the same prototype but for the name of the last argument
    assert protos[NAMES[0]][:5] == protos[NAMES[1]][:5] == ["ebm_handle_t h", "int nvars", "const int *fields", "const double *w",
                                                            "const double *center"]
    assert protos[NAMES[0]][5] == "double *out" and protos[NAMES[1]][5] == "double *dev_out"
    import ctypes as C
    dp = C.POINTER(C.c_double)
    assert lib.ebm_ensemble_sums.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), dp, dp, dp]
    assert lib.ebm_ensemble_sums_device.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_int), dp, dp, C.c_void_p]


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    f = (ctypes.c_int * 1)(0)
    out = np.zeros(3)
    assert lib.ebm_ensemble_sums(None, 1, f, None, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert b"ebm_ensemble_sums" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
    assert lib.ebm_ensemble_sums_device(None, 1, f, None, None, ctypes.c_void_p(16)) == -1
    assert b"ebm_ensemble_sums_device" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()


def test_engine_checks_raise_before_any_device_call(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)               # no handle: a device call would fail on the missing attributes
    eng.ncol, eng.nlat, eng.model = 5, 4, "MIZ"

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    eng.lib, eng._h = NoCalls(), None
    ok_w, ok_c = np.ones(5), np.zeros((2, 4))
    for names, w, c in (((), None, None), (("T", "T"), None, None), (("T0",), None, None), (("Tg",), None, None),
                        (("T", "phi"), np.ones(4), None), (("T", "phi"), [1, 1, np.nan, 1, 1], None),
                        (("T", "phi"), [1, 1, np.inf, 1, 1], None), (("T", "phi"), ok_w, np.zeros((1, 4))),
                        (("T", "phi"), ok_w, np.full((2, 4), np.nan))):
        with pytest.raises(ValueError):
            eng.ensemble_sums(names, w, c)
    with pytest.raises(ValueError, match=r"weights\[2\]"):
        eng.ensemble_sums("T", [1, 1, np.nan, 1, 1])
    with pytest.raises(ValueError):
        eng.ensemble_sums_device(("T", "phi"), 0, ok_w, ok_c)
    names, ids, w, c = eng._check_sums_args("T", [0, -1, 2, 0, 1], None)
    assert names == ("T",) and ids == [10] and w.dtype == np.float64 and c is None
    eng._h = None


def test_docstrings_state_the_sharding_rule(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    doc = " ".join(ensemble.EnsembleRun.moments.__doc__.split())
    rule = "(D(ncol) + max_r D(ncol_r) + n - 1) * 2^-53 * sum|terms|"
    assert "another order" in doc and rule in doc and "D(m) = min(m, 32) + ceil(m / 32) - 2" in doc and "defined to the bit" in doc
    for name in ("DESIGN.md", "INTEGRATION.md", os.path.join("include", "ebm_hip.h")):
        text = " ".join(open(os.path.join(ROOT, name)).read().replace(" * ", " ").split())
        assert "ebm_ensemble_sums" in text and "D(ncol) + max_r D(ncol_r) + n - 1" in text, name


# ---- the all-reduce path, two ranks over gloo ------------------------------------------------------------------------------------

WORKER = textwrap.dedent("""
    import sys
    import numpy as np
    sys.path.insert(0, {root!r})
    sys.path.insert(0, {tests!r})
    import __graft_entry__ as graft
    import torch.distributed as dist
    from ensemble_sums_ref import abs_term_sums, adds_per_term, ensemble_sums_ref, gamma
    pkg = graft.load_package()
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]

    class Standin:
        '''The engine of this rank's shard: its fields on the host, its sums by the restatement.'''
        def __init__(self, fields):
            self.fields, self.calls = fields, []
        def ensemble_sums(self, names, weights=None, center=None):
            self.calls.append((tuple(names), weights is not None, center is not None))
            return ensemble_sums_ref(np.stack([self.fields[n] for n in names]), weights, center)

    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()
    U = 2.0 ** -53
    results = {{}}
    for ncol in (2, 33, 130):
        rng = np.random.default_rng(ncol)                   # the same ensemble on both ranks
        full = {{"T": rng.normal(5.0, 2.0, (ncol, 11)), "phi": rng.uniform(0.0, 1.0, (ncol, 11))}}
        full["phi"][rng.random((ncol, 11)) < 0.1] = np.nan
        full["T"][:, 3] = np.nan                            # a latitude without a contributor
        w = rng.uniform(0.0, 2.0, ncol)
        w[::3] = 0.0
        sl = pkg.shard_columns(ncol, ws, rank)
        for weights in (None, w):
            run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
            run.engine, run.ncol = Standin({{k: v[sl] for k, v in full.items()}}), sl.stop - sl.start
            mine = None if weights is None else weights[sl]
            names = ("T", "phi")
            x = np.stack([full[n] for n in names])
            summed = run.reduced_sums(names, mine, None, dist)
            whole = ensemble_sums_ref(x, weights, None)
            deepest = max(adds_per_term(pkg.shard_columns(ncol, ws, r).stop - pkg.shard_columns(ncol, ws, r).start) for r in range(ws))
            bound = gamma(adds_per_term(ncol) + deepest + ws - 1) * abs_term_sums(x, weights, None)
            assert (np.abs(summed - whole) <= bound).all(), (ncol, weights is None)
            got = run.moments(names, mine, dist)
            assert run.engine.calls[-2:] == [(names, weights is not None, False), (names, weights is not None, True)]
            s1 = ensemble_sums_ref(x, weights, None)
            want = pkg.moments_from_sums(s1, ensemble_sums_ref(x, weights, ensemble.moments_center(pkg.moments_from_sums(s1)["mean"])))
            for i, n in enumerate(names):
                assert set(got[n]) == {{"weight", "mean", "var"}}
                for k in got[n]:
                    assert got[n][k].shape == (11,)
                    assert np.array_equal(np.isnan(got[n][k]), np.isnan(want[k][i])), (n, k)
                    assert np.allclose(got[n][k], want[k][i], rtol=1e-12, atol=1e-12, equal_nan=True), (n, k)
                results[f"{{ncol}}_{{int(weights is not None)}}_{{n}}_{{rank}}"] = np.stack([got[n][k] for k in ("weight", "mean", "var")])
            assert np.isnan(got["T"]["mean"][3]) and np.isnan(got["T"]["var"][3]) and got["T"]["weight"][3] == 0.0
    # no process group: the shard's own sums, one call per pass
    run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
    run.engine, run.ncol = Standin({{"T": np.arange(12.0).reshape(4, 3)}}), 4
    got = run.moments("T")
    assert got["T"]["mean"].tolist() == [4.5, 5.5, 6.5] and got["T"]["var"].tolist() == [11.25] * 3 and len(run.engine.calls) == 2
    np.savez({out!r} + f".{{rank}}.npz", **results)
    dist.barrier()
    dist.destroy_process_group()
""")


def test_two_ranks_all_reduce_over_gloo(tmp_path, pkg):
    out = str(tmp_path / "moments")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    subprocess.check_call(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(pkg.free_port()), str(script)],
        env=env, timeout=240)
    a, b = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    assert len(a.files) == 3 * 2 * 2
    for k in a.files:                                       # every rank returns the moments of the whole ensemble
        assert same_bits(a[k], b[k.rsplit("_", 1)[0] + "_1"]), k
