"""CPU tests of the ensemble range, histogram and quantiles (ebm_ensemble_range, ebm_ensemble_histogram,
EnsembleRun.quantiles): the NumPy restatement of the two definitions (tests/ensemble_hist_ref.py) against np.histogram,
np.min and np.max on benign data, the clamp, the +-0.0 tie rule and empty latitudes; the quantile bracketing against the exact
inverted-CDF quantile with a stand-in engine built on the restatement, alone and over two gloo ranks; and the symbols in the
header, the library and the bindings."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT
from ensemble_hist_ref import HIST_BLOCK, ensemble_histogram_ref, ensemble_range_ref, same_bits, slots_ref

NAMES = ("ebm_ensemble_range", "ebm_ensemble_range_device", "ebm_ensemble_histogram", "ebm_ensemble_histogram_device")
CLAMPED = (1, 2, 3, 5, 7, 32, 63, 64)


def benign(nvars, ncol, nlat, seed, nbins):
    """Values, edges and NaN cells such that no value lies within rounding of a bin edge: the edges are lo = -4, hi = 4 (bin
    edges exact in binary for nbins a power of two, and np.linspace's otherwise), values at least 1e-9 off every edge."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5.0, 5.0, (nvars, ncol, nlat))
    edges = np.linspace(-4.0, 4.0, nbins + 1)
    near = np.abs(x[..., None] - edges).min(axis=-1) < 1e-9
    x[near] += 1e-6
    x[rng.random(x.shape) < 0.1] = np.nan
    return x, np.full((nvars, nlat), -4.0), np.full((nvars, nlat), 4.0), edges


@pytest.mark.parametrize("ncol", (1, 255, 256, 257, 600))
@pytest.mark.parametrize("nbins", (1, 7, 32, 64))
def test_restatement_against_numpy(ncol, nbins):
    x, lo, hi, edges = benign(2, ncol, 5, 100 * nbins + ncol, nbins)
    h = ensemble_histogram_ref(x, lo, hi, nbins)
    r = ensemble_range_ref(x)
    for v in range(2):
        for k in range(5):
            col = x[v, :, k][~np.isnan(x[v, :, k])]
            counts, _ = np.histogram(col, bins=edges)
            counts[-1] -= (col == 4.0).sum()                        # np.histogram closes its last bin; the definition does not
            assert h[v, 1:-1, k].tolist() == counts.tolist()
            assert h[v, 0, k] == (col < -4.0).sum() and h[v, -1, k] == (col >= 4.0).sum()
            assert r[v, 0, k] == col.size
            if col.size:
                assert r[v, 1, k] == col.min() and r[v, 2, k] == col.max()
    # weights: every slot is the sum of the weights of its members (dyadic weights: exact in any order)
    w = np.random.default_rng(ncol).integers(0, 5, ncol) / 4.0
    hw = ensemble_histogram_ref(x, lo, hi, nbins, w)
    for v in range(2):
        for k in range(5):
            ok = ~np.isnan(x[v, :, k])
            slot, _ = slots_ref(x[v, :, k], lo[v, k], hi[v, k], nbins)
            want = np.bincount(slot[ok], weights=w[ok], minlength=nbins + 2)
            assert hw[v, :, k].tolist() == want.tolist()
    assert same_bits(ensemble_range_ref(x, w)[:, 0], (~np.isnan(x) & (w != 0)[None, :, None]).sum(axis=1).astype(float))


def test_block_order_of_the_histogram():
    """Weights whose sum depends on the order: the restatement adds inside blocks of 256 in ascending order, then the blocks."""
    ncol = 2 * HIST_BLOCK + 3
    w = np.ones(ncol)
    w[0], w[HIST_BLOCK] = 2.0 ** 53, -2.0 ** 53
    x = np.zeros((1, ncol, 1))
    got = ensemble_histogram_ref(x, np.array([[-1.0]]), np.array([[1.0]]), 1, w)[0, 1, 0]
    first = 2.0 ** 53
    for _ in range(HIST_BLOCK - 1):
        first = first + 1.0                                        # absorbed: 2^53 + 1 rounds to 2^53
    second = -2.0 ** 53
    for _ in range(HIST_BLOCK - 1):
        second = second + 1.0
    assert got == ((0.0 + first) + second) + 3.0 and got != float(ncol - 2)


@pytest.mark.parametrize("nbins", CLAMPED)
def test_the_clamp_is_needed(nbins):
    """lo = -1, hi = 2, x = nextafter(2, -Inf): x < hi, yet t == nbins exactly."""
    x = np.array([np.nextafter(2.0, -np.inf), 2.0, -1.0, np.nextafter(-1.0, -np.inf), np.inf, -np.inf])
    slot, t = slots_ref(x, np.full(6, -1.0), np.full(6, 2.0), nbins)
    assert t[0] == float(nbins) and slot.tolist() == [nbins, nbins + 1, 1, 0, nbins + 1, 0]
    h = ensemble_histogram_ref(x[None, :, None], [[-1.0]], [[2.0]], nbins)
    want = np.zeros(nbins + 2)
    for s in slot:
        want[s] += 1.0
    assert h[0, :, 0].tolist() == want.tolist()


def test_restatement_rules():
    """-0.0 with lo = 0.0 is in bin 0; NaN cells and zero weights do not contribute; an empty latitude; the first of equal
    extremes gives the bits, whatever the blocking."""
    x = np.array([[[-0.0, np.nan, 1.0], [0.0, np.nan, np.nan], [0.5, np.nan, 3.0]]])            # [1, 3, 3]
    h = ensemble_histogram_ref(x, [[0.0, 0.0, 0.0]], [[1.0, 1.0, 2.0]], 2)
    assert h[0, :, 0].tolist() == [0.0, 2.0, 1.0, 0.0] and h[0, :, 1].tolist() == [0.0] * 4 and h[0, :, 2].tolist() == [0.0, 0.0, 1.0, 1.0]
    h = ensemble_histogram_ref(x, [[0.0, 0.0, 0.0]], [[1.0, 1.0, 2.0]], 2, np.array([0.0, -1.5, 2.0]))
    assert h[0, :, 0].tolist() == [0.0, -1.5, 2.0, 0.0] and h[0, :, 2].tolist() == [0.0, 0.0, 0.0, 2.0]
    r = ensemble_range_ref(x)
    assert r[0, :, 1].tolist() == [0.0, np.inf, -np.inf] and r[0, 0].tolist() == [3.0, 0.0, 2.0]
    assert np.signbit(r[0, 1, 0]) and r[0, 2, 0] == 0.5
    r = ensemble_range_ref(x, np.array([0.0, 1.0, 1.0]))
    assert not np.signbit(r[0, 1, 0]) and r[0, 0].tolist() == [2.0, 0.0, 1.0] and r[0, 1, 2] == r[0, 2, 2] == 3.0
    z = np.zeros((1, 70, 1))
    z[0, 40] = -0.0
    z[0, 0] = 5.0
    for block in (1, 32, 33, 70):
        got = ensemble_range_ref(z, None, block)
        assert got[0, 1, 0] == 0.0 and not np.signbit(got[0, 1, 0]), block
    z[0, 1] = -0.0
    for block in (1, 32, 33, 70):
        assert np.signbit(ensemble_range_ref(z, None, block)[0, 1, 0]), block


# ---- the quantile bracketing against the exact inverted-CDF quantile --------------------------------------------------------------

def exact_quantile(x, w, q):
    """The smallest contributing value whose cumulative weight reaches q * sum(w) (weights: small dyadic numbers, so the
    cumulative sums are exact), or NaN without a contributor."""
    ok = ~np.isnan(x) & (w != 0.0)
    if not ok.any():
        return np.nan
    order = np.argsort(x[ok], kind="stable")
    xs, cum = x[ok][order], np.cumsum(w[ok][order])
    return xs[np.argmax(cum >= q * cum[-1])]


class Standin:
    """An engine whose range and histogram are the restatement's, on host fields."""

    def __init__(self, fields):
        self.fields, self.calls = fields, []

    def ensemble_range(self, names, weights=None):
        self.calls.append(("range", tuple(names)))
        return ensemble_range_ref(np.stack([self.fields[n] for n in names]), weights)

    def ensemble_histogram(self, names, lo, hi, nbins, weights=None):
        self.calls.append(("histogram", tuple(names)))
        assert len(names) <= 12 and (np.asarray(lo) < np.asarray(hi)).all()
        return ensemble_histogram_ref(np.stack([self.fields[n] for n in names]), lo, hi, nbins, weights)


def quantile_fields(ncol, nlat, seed):
    rng = np.random.default_rng(seed)
    T = rng.normal(5.0, 2.0, (ncol, nlat)) + 8.0 * (rng.random((ncol, 1)) < 0.4)           # two branches
    phi = np.clip(rng.normal(0.3, 0.4, (ncol, nlat)), 0.0, 1.0)                           # ties at 0 and at 1
    phi[:, 0] = 0.0                                                                       # a constant latitude
    T[:, 1] = np.nan                                                                      # nobody
    T[rng.random((ncol, nlat)) < 0.1] = np.nan
    T[:, 2] = 1e-300 * rng.integers(1, 4, ncol)                                           # a tiny spread
    T[3 % ncol, 4] = np.inf                                                               # a non-finite maximum
    big = rng.normal(1e15, 1.0, (ncol, nlat))
    return {"T": T, "phi": phi, "big": big}


def widening(col, nbins, passes):
    """What the stated widening can add to a halfwidth: the first bracket and every pass's bin are widened by 16 ulps a side
    (passes + 1 times; of the bracket's larger end, at most a binade above the data's: twice its ulp), and a bracket
    narrower than nbins * 2^-1020 by that much a side."""
    return 2 * 16 * (passes + 1) * np.spacing(max(abs(col.max()), abs(col.min()))) + 2 * nbins * 2.0 ** -1020


def check_quantiles(got, fields, w, qs, nbins, passes):
    ww = np.ones(next(iter(fields.values())).shape[0]) if w is None else w
    for n, x in fields.items():
        v, hw = got[n]["value"], got[n]["halfwidth"]
        assert v.shape == hw.shape == (len(qs), x.shape[1])
        for k in range(x.shape[1]):
            col = x[:, k]
            ok = ~np.isnan(col) & (ww != 0.0)
            for j, q in enumerate(qs):
                want = exact_quantile(col, ww, q)
                if not ok.any():
                    assert np.isnan(v[j, k]) and np.isnan(hw[j, k]), (n, k, "no contributor")
                elif not np.isfinite(col[ok]).all():
                    assert np.isnan(v[j, k]) and hw[j, k] == np.inf, (n, k, "non-finite range")
                elif col[ok].max() == col[ok].min():
                    assert v[j, k] == want and hw[j, k] == 0.0, (n, k, "constant")
                else:
                    assert abs(v[j, k] - want) <= hw[j, k], (n, k, q, v[j, k], want, hw[j, k])
                    spread = col[ok].max() - col[ok].min()
                    assert hw[j, k] <= spread * float(nbins) ** -passes + widening(col[ok], nbins, passes), (n, k, q, hw[j, k], spread)


@pytest.mark.parametrize("ncol, nbins, passes", [(1, 32, 4), (2, 32, 4), (300, 32, 4), (300, 64, 3), (300, 2, 20), (77, 1, 3), (300, 7, 1)])
def test_quantile_bracketing_against_the_exact_quantile(pkg, ncol, nbins, passes):
    fields = quantile_fields(ncol, 6, ncol + nbins)
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    rng = np.random.default_rng(ncol)
    w = rng.integers(0, 4, ncol) / 2.0                              # zeros among them; dyadic: exact cumulative weights
    for weights in (None, w):
        run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
        run.engine, run.ncol = Standin(fields), ncol
        got = run.quantiles(("T", "phi", "big"), qs, weights, nbins=nbins, passes=passes)
        check_quantiles(got, fields, weights, qs, nbins, passes)
        # fifteen pairs: two groups, each one range call in all and one histogram call per pass (and repeat)
        kinds = [c[0] for c in run.engine.calls]
        assert kinds.count("range") == 1 and all(len(c[1]) <= 12 for c in run.engine.calls)
        if ncol > 2:                                                # (one or two members: a constant latitude needs no histogram)
            assert kinds.count("histogram") >= 2 * passes
            assert max(len(c[1]) for c in run.engine.calls if c[0] == "histogram") == 12
    # all weights zero: nobody contributes anywhere
    run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
    run.engine, run.ncol = Standin(fields), ncol
    got = run.quantiles("phi", 0.5, np.zeros(ncol))
    assert np.isnan(got["phi"]["value"]).all() and got["phi"]["value"].shape == (1, 6)
    assert [c[0] for c in run.engine.calls] == ["range"], "no histogram is needed"
    with pytest.raises(ValueError):
        run.quantiles("phi", 0.5, -np.ones(ncol))
    with pytest.raises(ValueError):
        run.quantiles("phi", 1.5)
    with pytest.raises(ValueError):
        run.quantiles("phi", 0.5, nbins=65)


def test_a_value_pushed_out_of_the_bracket_is_recovered(pkg):
    """An engine whose histogram moves every value by a few ulps more than the widening allows for: the sought value lands
    below or above now and then, the pass is repeated with a wider bracket, and the answer still holds."""
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (1, 200, 8))
    calls = []

    def shifted(lo, hi):
        calls.append(1)
        moved = x + (hi - lo)[:, None, :] * (0.6 if len(calls) % 2 else -0.6) * (len(calls) > 1)      # far out of the bracket
        h = ensemble_histogram_ref(x if len(calls) % 3 == 0 or len(calls) == 1 else moved, lo, hi, 8)
        return h
    r = ensemble_range_ref(x)
    v, hw = ensemble.bracket_quantiles(shifted, r, np.array([0.5]), 8, 3)
    want = np.quantile(x[0], 0.5, axis=0, method="inverted_cdf")
    assert len(calls) > 3, "honesty: passes were repeated"
    assert (np.abs(v[0] - want) <= hw[0]).all()


def test_a_bracket_that_cannot_be_restored_fails_as_such(pkg):
    """A histogram that always reports the weight below the bracket: the widening runs out of finite numbers and says so."""
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]

    def always_below(lo, hi):
        h = np.zeros((1, 10, 3))
        h[:, 0] = 5.0
        return h
    r = np.array([[[5.0] * 3, [0.0] * 3, [1e300] * 3]])
    with pytest.raises(RuntimeError, match="could not be restored"):
        ensemble.bracket_quantiles(always_below, r, np.array([0.5]), 8, 2)


# ---- symbols -----------------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert hdr.count("THIS TEXT IS THE DEFINITION") >= 8
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    julia = open(os.path.join(ROOT, "julia", "EBMHip.jl")).read()
    nargs = dict(zip(NAMES, (5, 5, 8, 8)))
    protos = {}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, bare)
        assert m, f"include/ebm_hip.h does not declare {name}"
        protos[name] = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert len(protos[name]) == nargs[name], name
        assert name in pkg.EXPORTS and hasattr(cdll, name)
        assert len(getattr(lib, name).argtypes) == nargs[name], name
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name
    assert protos[NAMES[0]][:4] == protos[NAMES[1]][:4] == ["ebm_handle_t h", "int nvars", "const int *fields", "const double *w"]
    assert protos[NAMES[2]][:7] == protos[NAMES[3]][:7] == ["ebm_handle_t h", "int nvars", "const int *fields", "const double *w",
                                                            "int nbins", "const double *lo", "const double *hi"]
    for host, dev in (NAMES[:2], NAMES[2:]):
        assert protos[host][-1] == "double *out" and protos[dev][-1] == "double *dev_out"
    import ctypes as C
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert lib.ebm_ensemble_range.argtypes == [C.c_void_p, C.c_int, ip, dp, dp]
    assert lib.ebm_ensemble_range_device.argtypes == [C.c_void_p, C.c_int, ip, dp, C.c_void_p]
    assert lib.ebm_ensemble_histogram.argtypes == [C.c_void_p, C.c_int, ip, dp, C.c_int, dp, dp, dp]
    assert lib.ebm_ensemble_histogram_device.argtypes == [C.c_void_p, C.c_int, ip, dp, C.c_int, dp, dp, C.c_void_p]
    for name in ("range", "histogram", "quantiles", "ensemble_range", "ensemble_histogram", "ensemble_range_tensor",
                 "ensemble_histogram_tensor"):
        assert callable(getattr(pkg.EnsembleRun, name)), name
    for name in ("ensemble_range", "ensemble_range_device", "ensemble_histogram", "ensemble_histogram_device"):
        assert callable(getattr(pkg.Engine, name)), name


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    f = (ctypes.c_int * 1)(0)
    out, lo, hi = np.zeros(9), np.zeros(1), np.ones(1)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.ebm_ensemble_range(None, 1, f, None, p(out)) == -1
    assert lib.ebm_last_error() == b"ebm_ensemble_range: null handle"
    assert lib.ebm_ensemble_range_device(None, 1, f, None, ctypes.c_void_p(16)) == -1
    assert lib.ebm_last_error() == b"ebm_ensemble_range_device: null handle"
    assert lib.ebm_ensemble_histogram(None, 1, f, None, 7, p(lo), p(hi), p(out)) == -1
    assert lib.ebm_last_error() == b"ebm_ensemble_histogram: null handle"
    assert lib.ebm_ensemble_histogram_device(None, 1, f, None, 7, p(lo), p(hi), ctypes.c_void_p(16)) == -1
    assert lib.ebm_last_error() == b"ebm_ensemble_histogram_device: null handle"


def test_engine_checks_raise_before_any_device_call(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)               # no handle: a device call would fail on the missing attributes
    eng.ncol, eng.nlat, eng.model = 5, 4, "MIZ"

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    eng.lib, eng._h = NoCalls(), None
    lo, hi = np.zeros((2, 4)), np.ones((2, 4))
    for names, w in (((), None), (("T", "T"), None), (("T0",), None), (("Tg",), None), (("T", "phi"), np.ones(4)),
                     (("T", "phi"), [1, 1, np.nan, 1, 1])):
        with pytest.raises(ValueError):
            eng.ensemble_range(names, w)
    for names, l, u, nbins, w in ((("T", "T0"), lo, hi, 7, None), (("T", "phi"), lo, hi, 0, None), (("T", "phi"), lo, hi, 65, None),
                                  (("T", "phi"), lo, hi, 7.5, None), (("T", "phi"), hi, lo, 7, None), (("T", "phi"), lo, lo, 7, None),
                                  (("T", "phi"), lo[:1], hi[:1], 7, None), (("T", "phi"), lo, hi * np.inf, 7, None),
                                  (("T", "phi"), lo - 1.7e308, hi + 1.7e308, 7, None), (("T", "phi"), lo, hi, 7, [1, 1, np.inf, 1, 1]),
                                  (("T",) * 13, np.zeros((13, 4)), np.ones((13, 4)), 7, None)):
        with pytest.raises(ValueError):
            eng.ensemble_histogram(names, l, u, nbins, w)
    with pytest.raises(ValueError, match=r"lo\[1\]\[2\]"):
        bad = hi.copy()
        bad[1, 2] = np.nan
        eng.ensemble_histogram(("T", "phi"), lo, bad, 7)
    with pytest.raises(ValueError):
        eng.ensemble_range_device(("T", "phi"), 0)
    with pytest.raises(ValueError):
        eng.ensemble_histogram_device(("T", "T"), lo, hi, 7, 0)
    names, ids, w, (l, u) = eng._check_histogram_args(("T", "phi", "T"), lo=np.zeros((3, 4)), hi=np.ones((3, 4)), nbins=7,
                                                      weights=[0, 1, 2, 0, 1])
    assert names == ("T", "phi", "T") and ids == [10, 4, 10] and w.dtype == np.float64 and l.shape == u.shape == (3, 4)


# ---- the all-reduce path, two ranks over gloo ------------------------------------------------------------------------------------

WORKER = textwrap.dedent("""
    import sys
    import numpy as np
    sys.path.insert(0, {root!r})
    sys.path.insert(0, {tests!r})
    import __graft_entry__ as graft
    import torch.distributed as dist
    from ensemble_hist_ref import ensemble_histogram_ref, ensemble_range_ref, same_bits
    from test_host_ensemble_hist import Standin, check_quantiles, quantile_fields
    pkg = graft.load_package()

    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()
    results = {{}}
    qs = (0.0, 0.05, 0.5, 0.95, 1.0)
    for ncol in (2, 33, 300):
        full = quantile_fields(ncol, 6, ncol)               # the same ensemble on both ranks
        full["T"][:, 4] = np.where(np.isinf(full["T"][:, 4]), 1.0, full["T"][:, 4])
        w = np.random.default_rng(ncol).integers(0, 4, ncol) / 2.0
        sl = pkg.shard_columns(ncol, ws, rank)
        for weights in (None, w):
            run = pkg.EnsembleRun.__new__(pkg.EnsembleRun)
            run.engine, run.ncol = Standin({{k: v[sl] for k, v in full.items()}}), sl.stop - sl.start
            mine = None if weights is None else weights[sl]
            names = ("T", "phi")
            x = np.stack([full[n] for n in names])
            assert same_bits(run.range(names, mine, dist), ensemble_range_ref(x, weights)), "SUM, MIN, MAX are exact"
            lo, hi = np.full((2, 6), -1.0), np.full((2, 6), 9.0)
            assert same_bits(run.histogram(names, lo, hi, 7, mine, dist), ensemble_histogram_ref(x, lo, hi, 7, weights)), \\
                "dyadic weights: the shards add to the unsharded histogram"
            got = run.quantiles(names, qs, mine, dist)
            check_quantiles(got, {{n: full[n] for n in names}}, weights, qs, 32, 4)
            for n in names:
                results[f"{{ncol}}_{{int(weights is not None)}}_{{n}}_{{rank}}"] = np.stack([got[n]["value"], got[n]["halfwidth"]])
    np.savez({out!r} + f".{{rank}}.npz", **results)
    dist.barrier()
    dist.destroy_process_group()
""")


def test_two_ranks_all_reduce_over_gloo(tmp_path, pkg):
    out = str(tmp_path / "quantiles")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    subprocess.check_call(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", str(pkg.free_port()), str(script)],
        env=env, timeout=240)
    a, b = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    assert len(a.files) == 3 * 2 * 2
    for k in a.files:                                       # every rank returns the quantiles of the whole ensemble
        assert same_bits(a[k], b[k.rsplit("_", 1)[0] + "_1"]), k
