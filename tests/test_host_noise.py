"""CPU tests of the forcing noise (ebm_set_column_noise, include/ebm_hip.h): the host restatement of the generator
against the published Philox4x32-10 answers and the 53-bit uniform construction; the four symbols in the header, the
library, the bindings and INTEGRATION.md; their null-handle refusals without a GPU; the Python argument checks of
Engine.set_column_noise and EnsembleRun(noise=...), which run before any device call."""
import ctypes
import os
import re
import sys
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT
from support import bare_engine


def _noise(pkg):
    return import_module(pkg.__name__ + ".noise")


# Random123's known-answer vectors for Philox4x32-10 (counter words, key words, output words)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_philox_restatement_reproduces_the_known_answers(pkg, ctr, key, want):
    got = _noise(pkg).philox4x32_10(np.array(ctr), np.array(key))
    assert [int(w) for w in got] == list(want)


def test_philox_restatement_broadcasts_over_counters(pkg):
    n = _noise(pkg)
    ctrs = np.array([c for c, _, _ in KAT])
    keys = np.array([k for _, k, _ in KAT])
    assert np.array_equal(n.philox4x32_10(ctrs, keys), np.array([w for _, _, w in KAT], dtype=np.uint32))


def test_uniforms_of_edge_words(pkg):
    n = _noise(pkg)
    u1, u2 = n.uniforms(np.zeros(4, dtype=np.uint32))
    assert u1 == 2.0 ** -53 and u2 == 0.0                    # a = 0: the smallest u1, never 0 (log stays finite)
    u1, u2 = n.uniforms(np.full(4, 0xFFFFFFFF, dtype=np.uint32))
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -53              # all ones: u1 = 1 exactly, u2 < 1
    # a takes the 32 bits of w0 above the top 21 bits of w1
    u1, _ = n.uniforms(np.array([1, 0x800, 0, 0], dtype=np.uint32))
    assert u1 == (2 ** 21 + 1 + 1) * 2.0 ** -53


def test_counter_layout_is_step_then_stream(pkg):
    """words() puts lo32(n), hi32(n), lo32(stream), hi32(stream) into the counter and lo32/hi32(seed) into the key."""
    n = _noise(pkg)
    seed, stream, step = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x1_0000_0005
    got = n.words(seed, [stream], step, 1)[0, 0]
    want = n.philox4x32_10(np.array([step & 0xFFFFFFFF, step >> 32, stream & 0xFFFFFFFF, stream >> 32]),
                           np.array([seed & 0xFFFFFFFF, seed >> 32]))
    assert np.array_equal(got, want)


def test_ar1_recurrence_and_tau(pkg):
    n = _noise(pkg)
    xi = np.array([[1.0, -2.0, 0.5]])
    N = n.ar1(xi, 2.0, 0.5)
    s = 2.0 * np.sqrt(1.0 - 0.25)
    assert N[0, 0] == s * 1.0 and N[0, 1] == 0.5 * N[0, 0] + s * -2.0 and N[0, 2] == 0.5 * N[0, 1] + s * 0.5
    assert n.rho_from_tau(0.5, 0.01) == np.exp(-0.01 / 0.5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            n.rho_from_tau(bad, 0.01)


NEW = {
    "ebm_set_column_noise": (r"ebm_handle_t\s+h\s*,\s*const\s+double\s*\*\s*sigma\s*,\s*const\s+double\s*\*\s*rho\s*,"
                             r"\s*const\s+unsigned\s+long\s+long\s*\*\s*stream\s*,\s*unsigned\s+long\s+long\s+seed", 5),
    "ebm_get_noise_state": (r"ebm_handle_t\s+h\s*,\s*double\s*\*\s*N", 2),
    "ebm_set_noise_state": (r"ebm_handle_t\s+h\s*,\s*const\s+double\s*\*\s*N", 2),
    "ebm_noise_innovations": (r"ebm_handle_t\s+h\s*,\s*long\s+long\s+first_step\s*,\s*int\s+nsteps\s*,\s*double\s*\*\s*out", 4),
}


@pytest.mark.parametrize("name", sorted(NEW))
def test_symbols_are_declared_exported_bound_and_documented(pkg, name):
    args, arity = NEW[name]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ebm_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + args + r"\s*\)\s*;", hdr), name
    assert name in pkg.EXPORTS
    assert hasattr(ctypes.CDLL(pkg.LIB_PATH), name)
    _lib = sys.modules[pkg.__name__ + "._lib"]
    assert len(getattr(_lib.load(), name).argtypes) == arity
    assert re.search(r"\b" + name + r"\b", open(os.path.join(ROOT, "INTEGRATION.md")).read())


def test_the_definition_is_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    block = hdr[hdr.index("Per-column STOCHASTIC FORCING"):hdr.index("int ebm_set_column_noise")]
    assert "THIS TEXT IS THE DEFINITION" in block
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "cospi", "sqrt(1 - rho_c^2)"):
        assert word in block, word


def test_null_handle_is_refused_without_a_gpu(pkg):
    _lib = sys.modules[pkg.__name__ + "._lib"]
    lib = _lib.load()
    one = np.array([1.0])
    zero = np.array([0.0])
    assert lib.ebm_set_column_noise(None, _lib.dptr(one), _lib.dptr(zero), None, 0) == -1
    assert b"null handle" in lib.ebm_last_error()
    assert lib.ebm_get_noise_state(None, _lib.dptr(zero)) == -1
    assert lib.ebm_set_noise_state(None, _lib.dptr(zero)) == -1
    assert lib.ebm_noise_innovations(None, 0, 1, _lib.dptr(zero)) == -1
    assert b"bad argument" in lib.ebm_last_error()


@pytest.mark.parametrize("kw, msg", [
    (dict(sigma=float("nan")), "sigma"),
    (dict(sigma=[1.0, float("inf"), 1.0]), "sigma"),
    (dict(sigma=-0.1), "sigma"),
    (dict(sigma=[1.0, 1.0]), "shape"),
    (dict(sigma=1.0, rho=1.0), "rho"),
    (dict(sigma=1.0, rho=-0.1), "rho"),
    (dict(sigma=1.0, rho=float("nan")), "rho"),
    (dict(sigma=1.0, rho=[0.5, 0.5]), "shape"),
    (dict(sigma=1.0, tau=0.0), "tau"),
    (dict(sigma=1.0, tau=-1.0), "tau"),
    (dict(sigma=1.0, tau=float("nan")), "tau"),
    (dict(sigma=1.0, rho=0.5, tau=1.0), "rho or tau"),
    (dict(sigma=1.0, streams=[0, 1]), "streams"),
    (dict(sigma=1.0, streams=[0, -1, 2]), "streams"),
    (dict(sigma=1.0, streams=[0.5, 1.0, 2.0]), "streams"),
    (dict(sigma=1.0, seed=-1), "seed"),
    (dict(sigma=1.0, seed=2 ** 64), "seed"),
])
def test_engine_noise_checks_come_before_any_device_call(pkg, kw, msg):
    with pytest.raises(ValueError, match=msg):
        bare_engine(pkg, dt=1.0 / 2000).set_column_noise(**kw)


def test_engine_noise_state_and_innovation_checks(pkg):
    eng = bare_engine(pkg, dt=1.0 / 2000)
    for bad in ([0.0, 0.0], [0.0, float("nan"), 0.0]):
        with pytest.raises(ValueError):
            eng.set_noise_state(bad)
    with pytest.raises(ValueError, match="first_step"):
        eng.noise_innovations(-1, 4)
    with pytest.raises(ValueError, match="nsteps"):
        eng.noise_innovations(0, -4)


def test_tau_maps_to_rho_on_the_host(pkg):
    sig, rho, streams, seed = bare_engine(pkg, dt=1.0 / 2000).check_noise_args(0.7, tau=0.25, seed=5, streams=np.array([7, 8, 9]))
    assert np.array_equal(sig, [0.7] * 3) and np.array_equal(rho, [np.exp(-(1.0 / 2000) / 0.25)] * 3)
    assert streams.dtype == np.uint64 and list(streams) == [7, 8, 9] and seed == 5


def _st(pkg):
    return pkg.SpaceTime("sin", 18, 20, 1)


@pytest.mark.parametrize("noise, streams, msg", [
    (dict(sigma=-1.0), None, "sigma"),
    (dict(sigma=1.0, rho=1.0), None, "rho"),
    (dict(sigma=1.0, tau=0.0), None, "tau"),
    (dict(rho=0.5), None, "expected dict"),
    (dict(sigma=1.0, colour="red"), None, "expected dict"),
    (dict(sigma=1.0), [0, 1], "streams"),
    (None, [0, 1, 2], "noise_streams without noise"),
])
def test_ensemble_noise_checks_come_before_any_device_call(pkg, monkeypatch, noise, streams, msg):
    ens = import_module(pkg.__name__ + ".ensemble")

    def no_engine(*a, **k):
        raise AssertionError("Engine created before the argument checks refused the call")
    monkeypatch.setattr(ens, "Engine", no_engine)
    st = _st(pkg)
    par = pkg.default_parameters("MIZ")
    with pytest.raises(ValueError, match=msg):
        ens.EnsembleRun("MIZ", st, par, {"Ei": np.zeros((3, st.nx))}, noise=noise, noise_streams=streams)


def test_ensemble_equilibrate_refuses_noise(pkg):
    ens = import_module(pkg.__name__ + ".ensemble")
    run = ens.EnsembleRun.__new__(ens.EnsembleRun)
    run.st, run.has_schedules, run.has_noise, run.step_index = _st(pkg), False, True, 0
    run.engine = bare_engine(pkg, dt=1.0 / 2000)
    with pytest.raises(ValueError, match="noise="):
        run.equilibrate(5)
