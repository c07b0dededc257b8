"""CPU tests of the ensemble covariance (ebm_ensemble_covariance): the NumPy restatement of its terms against exact sums, the
mirror rule, the host-side checks of the binding, EnsembleRun.covariance and .eofs on a stand-in that answers the two device
methods with the restatement — a rank-2 ensemble whose EOFs are known, two shards against the unsharded call within the
stated bound — and the symbols in the header, the library and the bindings.

The bound is derived, not fitted.  The terms a and b are float64 numbers that the definition fixes to the bit; a sum of n
products through any order of correctly rounded multiplies, adds or fused multiply-adds, then nblocks - 1 adds of partials, is
within (n + nblocks) 2^-53 T of the exact sum to first order, T = sum |a b|; the factor 1 + 2^-4 covers the second-order terms
and the restatement's own np.longdouble roundings (ensemble_cov_ref.py), which this file holds against the exact rational sum
of the terms (fractions.Fraction) on a handful of elements."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from ensemble_cov_ref import K_COV_BLOCK, covariance_bound, ensemble_cov_ref, is_symmetric_call, mirror, terms
from support import same_bits

NAMES = ("ebm_ensemble_covariance", "ebm_ensemble_covariance_device")


def benign(ncol, nlat, seed):
    rng = np.random.default_rng(seed)
    xa = rng.normal(0.0, 1.0, (ncol, nlat)) * 2.0 ** rng.integers(-3, 4, (ncol, nlat))
    xb = rng.normal(1.0, 2.0, (ncol, nlat))
    xa[rng.random(xa.shape) < 0.05] = np.nan
    xb[rng.random(xb.shape) < 0.05] = np.nan
    w = rng.uniform(-0.5, 2.0, ncol)
    w[rng.random(ncol) < 0.2] = 0.0
    return xa, xb, w, rng.normal(0.0, 0.5, nlat), rng.normal(1.0, 0.5, nlat)


def exact_element(xa, xb, w, ca, cb, i, j):
    """out[i][j] as the exact rational sum of the float64 terms of the definition, written out member by member."""
    total, T = Fraction(0), Fraction(0)
    for c in range(xa.shape[0]):
        wc = 1.0 if w is None else float(w[c])
        x, y = float(xa[c, i]), float(xb[c, j])
        da = x if ca is None else x - float(ca[i])
        a = wc * da
        b = y if cb is None else y - float(cb[j])
        a = 0.0 if wc == 0.0 or math.isnan(x) else a
        b = 0.0 if wc == 0.0 or math.isnan(y) else b
        total += Fraction(a) * Fraction(b)
        T += abs(Fraction(a) * Fraction(b))
    return total, T


@pytest.mark.parametrize("ncol", [1, 5, 37, 130])
def test_restatement_against_exact_sums(ncol):
    xa, xb, w, ca, cb = benign(ncol, 7, 10 + ncol)
    for ww, a, b in ((None, None, None), (w, None, cb), (w, ca, cb), (None, ca, None)):
        got, T, n = ensemble_cov_ref(xa, xb, ww, a, b)
        assert n == (ncol if ww is None else np.count_nonzero(ww))
        for i, j in ((0, 0), (0, 6), (3, 2), (6, 0), (5, 5)):
            exact, t = exact_element(xa, xb, ww, a, b, i, j)
            assert abs(Fraction(float(T[i, j])) - t) <= t * Fraction(ncol + 1, 2 ** 53)
            # the longdouble sum rounded to double: one rounding of the result, ncol roundings of 2^-64
            assert abs(Fraction(float(got[i, j])) - exact) <= abs(exact) * Fraction(1, 2 ** 53) + t * Fraction(ncol + 1, 2 ** 63)
            # math.fsum of the float64 products: each product rounded once (2^-53 of its magnitude), their sum once
            ta, tb = terms(xa, xb, ww, a, b)
            fs = math.fsum(float(p) * float(q) for p, q in zip(ta[:, i], tb[:, j]))
            assert abs(float(got[i, j]) - fs) <= 2.0 ** -53 * (3.0 * float(T[i, j]) + abs(fs))       # (|exact| <= T)
    # integers: every sum is exact
    xi = np.random.default_rng(1).integers(-9, 10, (2, ncol, 5)).astype(np.float64)
    got, T, n = ensemble_cov_ref(xi[0], xi[1])
    assert np.array_equal(got, xi[0].T @ xi[1]) and np.array_equal(T, np.abs(xi[0]).T @ np.abs(xi[1])) and n == ncol


def test_restatement_rules():
    """NaN cells and zero weights give +0.0 terms on their own side only; Inf is data, and Inf * 0 is NaN."""
    xa = np.array([[1.0, np.nan], [2.0, 3.0], [np.inf, 1.0]])
    xb = np.array([[4.0, 5.0], [np.nan, 6.0], [7.0, np.nan]])
    a, b = terms(xa, xb)
    assert a.tolist() == [[1.0, 0.0], [2.0, 3.0], [np.inf, 1.0]] and b.tolist() == [[4.0, 5.0], [0.0, 6.0], [7.0, 0.0]]
    out, T, n = ensemble_cov_ref(xa, xb)
    assert n == 3 and out[1].tolist() == [7.0, 18.0] and out[0, 0] == np.inf and np.isnan(out[0, 1]), "Inf * 0"
    out, T, n = ensemble_cov_ref(xa, xb, np.array([1.0, -2.0, 0.0]))
    assert n == 2 and np.isfinite(out).all() and out.tolist() == [[4.0, 5.0 - 24.0], [0.0, -36.0]], "weight 0 hides the Inf"
    a, b = terms(xa, xb, np.array([1.0, -2.0, 0.0]), np.array([1.0, 1.0]), np.array([0.5, 0.5]))
    assert a.tolist() == [[0.0, 0.0], [-2.0, -4.0], [0.0, 0.0]] and b.tolist() == [[3.5, 4.5], [0.0, 5.5], [0.0, 0.0]]
    assert not np.signbit(a[a == 0.0]).any() and not np.signbit(b[b == 0.0]).any(), "replaced by +0.0"


def test_mirror_rule():
    xa, _, w, ca, cb = benign(37, 9, 3)
    assert is_symmetric_call(True, None, None) and is_symmetric_call(True, ca, ca.copy())
    assert not is_symmetric_call(False, None, None) and not is_symmetric_call(True, ca, None) and not is_symmetric_call(True, ca, cb)
    assert not is_symmetric_call(True, np.array([0.0]), np.array([-0.0])), "equal bit for bit, not as numbers"
    m = mirror(np.arange(9.0).reshape(3, 3))
    assert m.tolist() == [[0.0, 1.0, 2.0], [1.0, 4.0, 5.0], [2.0, 5.0, 8.0]]
    plain, _, _ = ensemble_cov_ref(xa, xa, w, ca, ca)
    sym, T, _ = ensemble_cov_ref(xa, xa, w, ca, ca, same_field=True)
    assert same_bits(sym, sym.T) and same_bits(T, T.T) and same_bits(np.triu(sym), np.triu(plain))
    assert not same_bits(plain, plain.T), "honesty: (w d_i) d_j and (w d_j) d_i round differently on this data"
    other, _, _ = ensemble_cov_ref(xa, xa, w, ca, cb, same_field=True)
    assert not same_bits(other, other.T), "two centers: no mirror"


def test_engine_checks_raise_before_any_device_call(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)               # no handle: a device call would fail on the missing attributes
    eng.ncol, eng.nlat, eng.model = 5, 4, "MIZ"

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    eng.lib, eng._h = NoCalls(), None
    ok_w, ok_c = np.ones(5), np.zeros(4)
    for a, b, w, ca, cb in (("T0", None, None, None, None), ("T", "Tg", None, None, None), (("T", "phi"), None, None, None, None),
                            (None, "T", None, None, None), ("T", "phi", np.ones(4), None, None), ("T", "phi", [1, 1, np.nan, 1, 1], None, None),
                            ("T", "phi", ok_w, np.zeros(5), None), ("T", "phi", ok_w, None, np.zeros((1, 4))),
                            ("T", "phi", ok_w, [0, np.inf, 0, 0], None), ("T", "phi", ok_w, ok_c, [0, 0, 0, np.nan])):
        with pytest.raises(ValueError):
            eng.ensemble_covariance(a, b, w, ca, cb)
    with pytest.raises(ValueError, match=r"weights\[2\]"):
        eng.ensemble_covariance("T", None, [1, 1, np.inf, 1, 1])
    with pytest.raises(ValueError, match=r"center_a\[1\]"):
        eng.ensemble_covariance("T", None, None, [0, np.inf, 0, 0])
    with pytest.raises(ValueError, match=r"center_b\[3\]"):
        eng.ensemble_covariance("T", "phi", None, ok_c, [0, 0, 0, np.nan])
    with pytest.raises(ValueError, match="dev_ptr"):
        eng.ensemble_covariance_device("T", "phi", ok_w, ok_c, ok_c, 0)
    fa, fb, w, ca, cb = eng.check_covariance_args("T", None, [0, -1, 2, 0, 1], [1, 2, 3, 4])
    assert (fa, fb) == (10, 10) and w.dtype == np.float64 and w.tolist() == [0.0, -1.0, 2.0, 0.0, 1.0] and ca.tolist() == [1.0, 2.0, 3.0, 4.0] and cb is None
    assert eng.check_covariance_args("Ti", "phi")[:2] == (7, 4)
    eng._h = None


class Standin:
    """What CovarianceMixin is written in terms of, answered by the restatements on host fields (a shard of them)."""

    def __init__(self, ensemble, fields):
        self.fields, self.calls = fields, []
        self.mixin = type("Run", (ensemble.CovarianceMixin,), {
            "ensemble_sums": lambda s, names, weights=None, center=None: self.sums(names, weights, center),
            "ensemble_covariance": lambda s, a, b=None, weights=None, ca=None, cb=None: self.cov(a, b, weights, ca, cb)})()

    def sums(self, names, weights, center):
        from ensemble_sums_ref import ensemble_sums_ref
        self.calls.append(("sums", tuple(names)))
        return ensemble_sums_ref(np.stack([self.fields[n] for n in names]), weights, center)

    def cov(self, a, b, weights, ca, cb):
        b = a if b is None else b
        self.calls.append(("cov", a, b))
        return ensemble_cov_ref(self.fields[a], self.fields[b], weights, ca, cb, same_field=a == b)[0]


def rank_two(ncol, nlat, seed):
    """T = 10 + s1 e1 + s2 e2 with orthonormal e1, e2 and centred, uncorrelated scores: the EOFs are e1 and e2."""
    rng = np.random.default_rng(seed)
    k = np.arange(nlat)
    e1, e2 = np.cos(np.pi * k / nlat), (k / nlat) ** 2
    e1 = e1 / np.linalg.norm(e1)
    e2 = e2 - (e2 @ e1) * e1
    e2 = e2 / np.linalg.norm(e2)
    s1, s2 = rng.normal(0.0, 3.0, ncol), rng.normal(0.0, 1.0, ncol)
    s1, s2 = s1 - s1.mean(), s2 - s2.mean()
    s2 = s2 - (s2 @ s1) / (s1 @ s1) * s1
    return 10.0 + np.outer(s1, e1) + np.outer(s2, e2), (e1, e2), (s1 @ s1 / ncol, s2 @ s2 / ncol)


def test_covariance_and_eofs_on_a_standin(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    ncol, nlat = 41, 23
    T, (e1, e2), (v1, v2) = rank_two(ncol, nlat, 4)
    phi = np.random.default_rng(2).uniform(0.0, 1.0, (ncol, nlat))
    s = Standin(ensemble, {"T": T, "phi": phi})
    got = s.mixin.covariance("T")
    assert s.calls == [("sums", ("T",)), ("cov", "T", "T")], "one pass of sums, one matrix"
    assert set(got) == {"mean_a", "mean_b", "cov", "n"} and got["cov"].shape == got["n"].shape == (nlat, nlat) and (got["n"] == ncol).all()
    assert same_bits(got["cov"], got["cov"].T) and same_bits(got["mean_a"], got["mean_b"])
    assert np.allclose(got["cov"], np.cov(T.T, bias=True), rtol=1e-10, atol=1e-13) and np.allclose(got["mean_a"], T.mean(axis=0), rtol=1e-14)
    cross = s.mixin.covariance("T", "phi")
    assert np.allclose(cross["cov"], np.cov(T.T, phi.T, bias=True)[:nlat, nlat:], rtol=1e-9, atol=1e-13)
    assert np.allclose(s.mixin.covariance("phi", "T")["cov"], cross["cov"].T, rtol=1e-9, atol=1e-13)
    # weights: the members of weight zero are gone, a weight of 2 counts a member twice
    w = np.ones(ncol)
    w[::3], w[1::3] = 0.0, 2.0
    rep = np.concatenate([T[w > 0], T[w == 2.0]])
    assert np.allclose(s.mixin.covariance("T", None, w)["cov"], np.cov(rep.T, bias=True), rtol=1e-9, atol=1e-13)
    # a latitude without a contributor: NaN row and column, n = 0 there
    holes = T.copy()
    holes[:, 5] = np.nan
    h = Standin(ensemble, {"T": holes}).mixin.covariance("T")
    assert np.isnan(h["cov"][5]).all() and np.isnan(h["cov"][:, 5]).all() and (h["n"][5] == 0).all() and np.isfinite(np.delete(np.delete(h["cov"], 5, 0), 5, 1)).all()
    with pytest.raises(ValueError, match="not finite"):
        Standin(ensemble, {"T": holes}).mixin.eofs("T", 1)
    # EOFs: the two known modes, largest-magnitude entry positive, variances and fractions
    eof = s.mixin.eofs("T", 3)
    assert eof["modes"].shape == (3, nlat) and eof["variance"].shape == eof["explained"].shape == (3,)
    for mode, e in zip(eof["modes"], (e1, e2)):
        assert np.allclose(mode, e * np.sign(e[np.argmax(np.abs(e))]), atol=1e-10) and mode[np.argmax(np.abs(mode))] > 0.0
    assert np.allclose(eof["variance"][:2], [v1, v2], rtol=1e-10) and abs(eof["variance"][2]) < 1e-12 * v1
    assert np.allclose(eof["explained"][:2], [v1 / (v1 + v2), v2 / (v1 + v2)], rtol=1e-10)
    # quadrature weights: orthonormal under them; a zero weight removes the latitude from the modes
    quad = np.linspace(0.5, 2.0, nlat)
    quad[0] = 0.0
    q = s.mixin.eofs("T", 2, quad=quad)["modes"]
    assert np.allclose((q * quad) @ q.T, np.eye(2), atol=1e-10) and (q[:, 0] == 0.0).all()
    for bad in (0, nlat + 1, 1.5, True):
        with pytest.raises(ValueError, match="nmodes"):
            s.mixin.eofs("T", bad)
    with pytest.raises(ValueError, match="quad"):
        s.mixin.eofs("T", 1, quad=-np.ones(nlat))


class TwoRanks:
    """Two ranks of a process group in two threads of this process: what CovarianceMixin asks of ``dist`` (is_initialized,
    get_world_size, get_backend, ReduceOp, all_reduce), the all-reduce adding the ranks' tensors in rank order, in place."""

    class ReduceOp:
        SUM = "SUM"

    def __init__(self):
        import threading
        self.barrier, self.slots, self.local, self.reduced = threading.Barrier(2), [None, None], threading.local(), []

    def is_initialized(self):
        return True

    def get_world_size(self):
        return 2

    def get_backend(self):
        return "gloo"

    def all_reduce(self, t, op=None):
        assert op == "SUM"
        rank = self.local.rank
        self.slots[rank] = t.clone()
        self.barrier.wait()
        total = self.slots[0] + self.slots[1]
        self.barrier.wait()                                 # both have read both slots
        t.copy_(total)
        if rank == 0:
            self.reduced.append(tuple(t.shape))

    def run(self, per_rank):
        """per_rank(rank) on each of the two ranks at once; their results in rank order."""
        import threading
        out, errors = [None, None], []

        def work(rank):
            self.local.rank = rank
            try:
                out[rank] = per_rank(rank)
            except BaseException as e:                      # noqa: B036 (reported below; the peer must not wait for ever)
                errors.append(e)
                self.barrier.abort()
        threads = [threading.Thread(target=work, args=(r,)) for r in (0, 1)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not errors, errors
        return out


@pytest.mark.parametrize("ncol", [37, K_COV_BLOCK + 9])
def test_two_shards_give_the_covariance_of_the_whole_ensemble_within_the_stated_bound(pkg, ncol):
    """CovarianceMixin.covariance and .eofs with ``dist`` over two ranks, each holding its shard of the members: the sums are
    all-reduced, then the matrices, and every rank divides by the S0 of the whole ensemble.  The bound: each shard's matrix is
    within its own bound of the exact sum of ITS terms about the center both ranks hold (the means the call returns), the
    add of the two rounds once, the division once; the restatement of the whole ensemble about the same center is within
    its bound of the same exact sum."""
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    nlat = 9
    xa, xb, w, _, _ = benign(ncol, nlat, ncol)
    xa[:, 4] = np.abs(xa[:, 4]) + 1.0                       # (no NaN here: a latitude where every member contributes)
    w = np.abs(w)
    fields = {"T": xa, "phi": xb}
    shards = [pkg.shard_columns(ncol, 2, r) for r in (0, 1)]
    group = TwoRanks()
    stand = [Standin(ensemble, {k: v[sl] for k, v in fields.items()}) for sl in shards]
    for a, b in (("T", None), ("T", "phi"), ("phi", "T")):
        got = group.run(lambda r: stand[r].mixin.covariance(a, b, w[shards[r]], group))
        assert all(same_bits(got[0][k], got[1][k]) for k in ("mean_a", "mean_b", "cov", "n")), "every rank returns the whole ensemble's"
        g = got[0]
        ya, yb = fields[a], fields[a if b is None else b]
        ca, cb = ensemble.moments_center(g["mean_a"]), ensemble.moments_center(g["mean_b"])
        whole, T, n = ensemble_cov_ref(ya, yb, w, ca, cb, same_field=b is None)
        bound = covariance_bound(T, n, ncol)
        for sl in shards:
            bound = bound + covariance_bound(ensemble_cov_ref(ya[sl], yb[sl], w[sl], ca, cb, same_field=b is None)[1],
                                             int(np.count_nonzero(w[sl])), sl.stop - sl.start)
        s0 = np.minimum.outer(np.where(np.isnan(ya), 0.0, w[:, None]).sum(axis=0), np.where(np.isnan(yb), 0.0, w[:, None]).sum(axis=0))
        assert np.allclose(g["n"], s0, rtol=1e-13) and (g["n"] > 0).all(), "the S0 of the whole ensemble, not of a shard"
        want = whole / g["n"]
        assert (np.abs(g["cov"] - want) <= (bound + 2.0 ** -53 * np.abs(whole)) / g["n"] + 2.0 ** -52 * np.abs(want)).all(), (a, b)
        # and against the unsharded call, whose center differs by the rounding of the means: a transposed or half-reduced
        # matrix is off by orders of magnitude more
        alone = Standin(ensemble, fields).mixin.covariance(a, b, w)
        scale = np.sqrt(np.outer(np.nanvar(ya, axis=0) + 1.0, np.nanvar(yb, axis=0) + 1.0))
        assert (np.abs(g["cov"] - alone["cov"]) <= 1e-12 * scale * w.max()).all() and np.allclose(g["mean_a"], alone["mean_a"], rtol=1e-13)
        if b is not None:
            assert not np.allclose(g["cov"], g["cov"].T, rtol=1e-3), "honesty: a transpose would show"
    assert group.reduced.count((nlat, nlat)) == 3 and stand[0].calls.count(("cov", "T", "phi")) == 1
    # eofs across the ranks: the modes of the whole ensemble, on every rank
    T2, (e1, e2), (v1, v2) = rank_two(ncol, nlat, 8)
    stand = [Standin(ensemble, {"T": T2[sl]}) for sl in shards]
    eof = group.run(lambda r: stand[r].mixin.eofs("T", 2, None, None, group))
    assert same_bits(eof[0]["modes"], eof[1]["modes"])
    for mode, e in zip(eof[0]["modes"], (e1, e2)):
        assert np.allclose(mode, e * np.sign(e[np.argmax(np.abs(e))]), atol=1e-9)
    assert np.allclose(eof[0]["variance"], [v1, v2], rtol=1e-9)
    doc = " ".join(ensemble.CovarianceMixin.covariance.__doc__.split())
    assert "NOT equal bit for bit" in doc and "another order" in doc


def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert "COVARIANCE ACROSS THE MEMBERS" in hdr and hdr.count("THIS TEXT IS THE DEFINITION") >= 8
    flat = " ".join(hdr.replace(" * ", " ").split())
    assert f"kCovBlock = {K_COV_BLOCK}" in flat and "(n + nblocks) 2^-53 T_ij (1 + 2^-4)" in flat and "Inf 0 is NaN" in flat
    assert "ebm_ensemble_covariance*" in flat, "the list of readers in the Validity paragraph"
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    julia = open(os.path.join(ROOT, "julia", "EBMHip.jl")).read()
    internal = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "csrc", "ebm_internal.h")).read()
    assert re.search(r"constexpr int kCovBlock = %d;" % K_COV_BLOCK, internal)
    protos = {}
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, bare)
        assert m, f"include/ebm_hip.h does not declare {name}"
        protos[name] = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert name in pkg.EXPORTS and hasattr(cdll, name)
        assert len(getattr(lib, name).argtypes) == 7, name
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name
    assert protos[NAMES[0]][:6] == protos[NAMES[1]][:6] == ["ebm_handle_t h", "int field_a", "int field_b", "const double *w",
                                                            "const double *center_a", "const double *center_b"]
    assert protos[NAMES[0]][6] == "double *out" and protos[NAMES[1]][6] == "double *dev_out"
    C = ctypes
    dp = C.POINTER(C.c_double)
    assert lib.ebm_ensemble_covariance.argtypes == [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp]
    assert lib.ebm_ensemble_covariance_device.argtypes == [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, C.c_void_p]


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    out = np.zeros(4)
    assert lib.ebm_ensemble_covariance(None, 0, 0, None, None, None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == -1
    assert b"ebm_ensemble_covariance" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
    assert lib.ebm_ensemble_covariance_device(None, 0, 0, None, None, None, ctypes.c_void_p(16)) == -1
    assert b"ebm_ensemble_covariance_device" in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()
