"""The host runtime's table math (csrc/ebm_tables.h) against the oracle, without a GPU: a stand-alone program
(tests/host_tables_main.cpp, plain g++, no HIP) fills the tables, the tests compare bits."""
import os
import re
import subprocess

import numpy as np
import pytest

from support import assert_same_bits as same_bits, compile_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLATS = (2, 3, 5, 64, 65, 180, 257)
GRIDS = ("identity", "sin")
# enum GeomTable of csrc/ebm_types.h
G = {n: i for i, n in enumerate("X 0 1 2 3 4 LO DI UP KSUB KDIAG KSUP AW SB".split())}
MODEL = {"MIZ": 0, "Classic": 1}
GRID = {"identity": 0, "sin": 1}


def compile_program(out, extra_flags=()):
    """The flags are the library's own arithmetic: no contraction of a*b+c (csrc/Makefile)."""
    return compile_host_program("host_tables_main.cpp", out, ("-ffp-contract=off",) + tuple(extra_flags))


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return compile_program(str(tmp_path_factory.mktemp("host_tables") / "host_tables"))


def param_order():
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    names = re.findall(r"EBM_P_(\w+)", re.search(r"enum ebm_param \{(.*?)\}", hdr, re.S).group(1))
    assert names[-1] == "COUNT"
    return names[:-1]


def run(prog, args, inputs, tmp):
    """One call of the program: `inputs` as raw doubles in, raw doubles out."""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.asarray(inputs, dtype=np.float64).tofile(fin)
    r = subprocess.run([prog, *map(str, args), fin, fout], capture_output=True, text=True)
    return r, (np.fromfile(fout, dtype=np.float64) if r.returncode == 0 else None)


def tables(prog, oracle, tmp, model, kind, nlat, par=None):
    st = oracle.SpaceTime(kind, nlat, 2000, 1)
    par = dict(oracle.default_parval, **(par or {}))
    gstride = nlat + 3                                  # padding behind every table: it must stay zero
    vec = [par[k] for k in param_order()]
    r, out = run(prog, ["tables", MODEL[model], GRID[kind], nlat, gstride], [st.dt, *st.x, *vec], tmp)
    assert r.returncode == 0, r.stderr
    slab = out[5:].reshape(len(G), gstride)
    assert not slab[:, nlat:].any(), "padding written"
    return st, par, out[:5], {n: slab[i, :nlat] for n, i in G.items()}


@pytest.mark.parametrize("nlat", NLATS)
@pytest.mark.parametrize("kind", GRIDS)
def test_miz_tables_are_the_oracles_bits(prog, oracle, tmp_path, kind, nlat):
    st, par, _, t = tables(prog, oracle, str(tmp_path), "MIZ", kind, nlat)
    g = oracle.DiffusionGeometry(kind, st.x, par["D"])
    same_bits(t["X"], st.x, "G_X")
    zero = np.zeros(nlat)
    stencil = (g.sub, g.diag, g.sup, zero, zero) if kind == "identity" else (g.mph, g.mmh, g.dxp, g.dxm, g.w)
    for i, want in enumerate(stencil):
        same_bits(t[str(i)], want, f"G_{i}")
    for name, want in (("LO", g.lo), ("DI", g.di), ("UP", g.up)):
        same_bits(t[name], want, "G_" + name)


@pytest.mark.parametrize("nlat", NLATS)
@pytest.mark.parametrize("kind", GRIDS)
def test_classic_tables_are_the_oracles_bits(prog, oracle, tmp_path, kind, nlat):
    st, par, derived, t = tables(prog, oracle, str(tmp_path), "Classic", kind, nlat)
    s = oracle.ClassicStatics(st.x, nlat, st.dt, par)
    g = oracle.DiffusionGeometry("identity", st.x, 1.0)            # get_diffop unscaled, whatever the grid (src/classic.jl:21)
    zero = np.zeros(nlat)
    for i, want in enumerate((g.sub, g.diag, g.sup, zero, zero)):
        same_bits(t[str(i)], want, f"G_{i}")
    for name, want in (("LO", g.lo), ("DI", g.di), ("UP", g.up), ("KSUB", s.k_sub), ("KDIAG", s.k_diag),
                       ("KSUP", s.k_sup), ("AW", s.aw), ("SB", s.S_base)):
        same_bits(t[name], want, "G_" + name)
    same_bits(derived, [s.cg_tau, s.dt_tau, s.dc, s.M, s.kLf], "cg_tau, dt_tau, dc, M, kLf")


def periodic_solve(a, n, b, M, E, W):
    """The elimination the tables are made for (csrc/ebm_zonal.hip, zonal_sweep_kernel), written out:
    U_l = cp_l U_{l+1} + ep_l W + dp_l with W = U_{n-1}, the last row reduced alongside."""
    dp = np.empty(n - 1)
    dp[0] = b[0] * M[0]
    R, f = 0.0, -a
    for l in range(n - 2):
        R -= f * dp[l]
        f = -a * E[l]
        dp[l + 1] = (a * dp[l] + b[l + 1]) * M[l + 1]
    U = np.empty(n)
    U[n - 1] = (b[n - 1] + R - (f - a) * dp[n - 2]) * W
    for l in range(n - 2, -1, -1):
        U[l] = a * M[l] * U[l + 1] + E[l] * U[n - 1] + dp[l]
    return U


# Largest max|U - ref| / max|ref| over the 16 systems below against numpy.linalg.solve on the dense matrix, measured with
# this file: 5.7e-14 (n = 4, a = 1e3, where the matrix has condition number 1 + 4a = 4001, so that the dense solve is itself
# only good to about 9e-13; every a <= 1 is below 2e-16 and the other a = 1e3 systems below 3.5e-15).  The bar is 10 x the
# largest figure.
PERIODIC_BAR = 5.7e-13


@pytest.mark.parametrize("a", (0.0, 1e-3, 1.0, 1e3))
@pytest.mark.parametrize("n", (3, 4, 64, 257))
def test_periodic_tables_solve_the_periodic_system(prog, tmp_path, n, a):
    B = 1.0 + 2.0 * a
    r, out = run(prog, ["periodic", n], [a, B], str(tmp_path))
    assert r.returncode == 0, r.stderr
    M, E, W = out[:n - 1], out[n - 1:2 * (n - 1)], out[-1]
    A = np.zeros((n, n))
    for l in range(n):
        A[l, l] += B
        A[l, (l - 1) % n] += -a
        A[l, (l + 1) % n] += -a
    b = np.random.default_rng(1000 * n + int(a)).standard_normal(n)
    ref = np.linalg.solve(A, b)
    err = float(np.max(np.abs(periodic_solve(a, n, b, M, E, W) - ref)) / np.max(np.abs(ref)))
    print(f"periodic n={n} a={a}: relative error {err:.3e}")
    assert err <= PERIODIC_BAR


def test_zonal_segments(prog):
    nlons = list(range(3, 600)) + [1024, 1536, 2048, 2049, 4096, 6144, 8192, 65536]
    got = [int(v) for v in subprocess.run([prog, "segments", *map(str, nlons)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    for nlon, S in zip(nlons, got):
        fits = [c for c in (4, 8, 16, 32) if nlon % c == 0 and nlon // c >= 64]
        assert S == (1 if nlon < 256 or not fits else max(fits)), nlon


def test_zonal_tables_coefficient_and_refusal(prog, oracle, tmp_path):
    """The host half of the zonal tables: a_k = (dt/cw) D / ((1 - x_k)(1 + x_k) dlambda^2) in the pair-split index space of
    four cells per thread, zero on the padding latitudes; a cell centre on the pole is refused with the caller's message."""
    nlat, T, nlon = 180, 64, 512                        # pitch 256; 512 longitudes: 8 segments of 64
    st = oracle.SpaceTime("sin", nlat, 2000, 1)
    par = oracle.default_parval
    vec = [par[k] for k in param_order()]
    r, out = run(prog, ["zonal", nlon, nlat, T, 4], [st.dt, *st.x, *vec], str(tmp_path))
    assert r.returncode == 0, r.stderr
    seg, chain_rows, red_rows = (int(v) for v in out[:3])
    assert (seg, chain_rows, red_rows) == (8, 64, 8)
    P = 4 * T
    a = out[3 + (2 * chain_rows + 2 * red_rows) * P:][:P]
    p = np.arange(P)
    k = 4 * ((p % (2 * T)) // 2) + 2 * (p // (2 * T)) + p % 2
    dl = 2.0 * np.pi / nlon
    xk = st.x[np.minimum(k, nlat - 1)]
    want = np.where(k < nlat, (st.dt / par["cw"]) * par["D"] / (((1.0 - xk) * (1.0 + xk)) * (dl * dl)), 0.0)
    same_bits(a, want, "a")
    x = st.x.copy()
    x[-1] = 1.0
    r, _ = run(prog, ["zonal", nlon, nlat, T, 4], [st.dt, *x, *vec], str(tmp_path))
    assert r.returncode == 3 and "needs |x| < 1 at every cell centre" in r.stderr
