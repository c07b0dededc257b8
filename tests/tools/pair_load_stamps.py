"""Diagnostic: how long the second pair of a lane waits for its Ei and D in phase D of the MIZ one-step kernel (needs the
-DEBM_STAMPS build of the library as argv[1]; argv[2] = number of columns, default 2048; argv[3] = a title).  Prints the
per-WAVE s_memtime timeline of tests/tools/wave_stamps.py (min / median / max over the waves, median over the workgroups,
in ticks since the workgroup's first instruction), then slot 7 (the second pair's Ei and D have arrived) minus slot 4 (the
first pair is done, its stores issued): over all waves, per wave of the median workgroup, and per wave as the median over
the workgroups."""
import ctypes as C, sys, os
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
pkg = g.load_package()
from energybalancemodel_jl_amd import _lib
_lib.LIB_PATH = sys.argv[1]
lib = _lib.load()
nlat, ncol, nt = 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 2048, 1048576
st = pkg.SpaceTime("sin", nlat, nt, 1)
par = pkg.default_parameters("MIZ")
eng = pkg.Engine("MIZ", st.grid_kind, st.x, pkg.engine.param_vector(par, pkg.default_parval), st.dt, ncol)
eng.set_column_forcing(0.5 * np.sin(2 * np.pi * np.arange(ncol) / ncol))
eng.set_time_table(st.t)
eng.run(0, 300, None, False); eng.sync()
lib.ebm_debug_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
lib.ebm_debug_stamps(eng._h, None)
eng.run(300, 3, None, False); eng.sync()
buf = np.zeros(ncol * (16 + 128), dtype=np.uint64)
lib.ebm_debug_stamps(eng._h, buf.ctypes.data_as(C.POINTER(C.c_ulonglong)))
s = buf[ncol * 16:].reshape(ncol, 16, 8).astype(np.int64)
names = ["first instruction", "inputs arrived", "phase D starts", "Tbar halo done", "first pair done",
         "arithmetic done", "stores issued"]
ref = s[:, :, 0].min(axis=1)[:, None]
for k, name in enumerate(names):
    rel = s[:, :, k] - ref
    print(f"{name:18s} first wave {np.median(rel.min(axis=1)):8.0f}   median wave {np.median(np.median(rel, axis=1)):8.0f}"
          f"   last wave {np.median(rel.max(axis=1)):8.0f}")
wg = ncol // 2
print(f"workgroup {wg}, rows = waves 0..15, columns as above:")
print(s[wg][:, :7] - s[wg][:, 0].min())
wait = s[:, :, 7] - s[:, :, 4]
print(f"second pair's input wait (ticks), {sys.argv[3] if len(sys.argv) > 3 else sys.argv[1]}:")
print(f"all waves of all workgroups: min {wait.min()}   median {np.median(wait):.0f}   mean {wait.mean():.0f}   max {wait.max()}")
print(f"workgroup {wg}, waves 0..15: {wait[wg].tolist()}")
print(f"median over the workgroups, waves 0..15: {np.median(wait, axis=0).astype(np.int64).tolist()}")
