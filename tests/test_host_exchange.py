"""CPU tests of the packed column export / import (ebm_column_record, ebm_export_columns, ebm_import_columns) and of the
selection across shards: the symbols in the header, the library and the bindings and their null refusals without a GPU;
resample_plan carried out in NumPy; the host-side argument checks; and resample_global's collectives over two gloo ranks
with a stand-in for the engine."""
import ctypes
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("ebm_column_record", "ebm_export_columns", "ebm_import_columns")


def test_symbols_are_declared_bound_and_documented(pkg):
    hdr = open(os.path.join(ROOT, "include", "ebm_hip.h")).read()
    assert "EXPORT and IMPORT whole columns" in hdr and hdr.count("THIS TEXT IS THE DEFINITION") >= 6
    bare = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cdll = ctypes.CDLL(pkg.LIB_PATH)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    julia = open(os.path.join(ROOT, "julia", "EBMHip.jl")).read()
    for name, arity in zip(NAMES, (3, 5, 6)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, bare)
        assert m, f"include/ebm_hip.h does not declare {name}"
        assert len(m.group(1).split(",")) == arity, name
        assert name in pkg.EXPORTS and hasattr(cdll, name)
        assert len(getattr(lib, name).argtypes) == arity, name
        assert re.search(r"\b%s\b" % name, integration), name
        assert re.search(r"\blibebm\.%s\(" % name, julia), name


def test_null_handle_is_refused_with_a_message(pkg):
    lib = sys.modules[pkg.__name__ + "._lib"].load()
    cols = np.zeros(1, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    m, n = ctypes.c_uint(), ctypes.c_longlong()
    calls = {"ebm_column_record": lambda: lib.ebm_column_record(None, ctypes.byref(n), ctypes.byref(m)),
             "ebm_export_columns": lambda: lib.ebm_export_columns(None, 1, cols.ctypes.data_as(ip), ctypes.c_void_p(16), ctypes.byref(m)),
             "ebm_import_columns": lambda: lib.ebm_import_columns(None, 1, cols.ctypes.data_as(ip), None, ctypes.c_void_p(16), 31)}
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in lib.ebm_last_error() and b"null handle" in lib.ebm_last_error()


# ---- resample_plan ---------------------------------------------------------------------------------------------------------------

def carry_out(pkg, plans, tokens, n, ws):
    """The plan on an array of per-member tokens: every rank's send lists read from the OLD array, then per rank the local
    gather, then the remote records."""
    shards = [pkg.shard_columns(n, ws, r) for r in range(ws)]
    old = [tokens[s] for s in shards]
    sent = [old[r][pl.send_cols] for r, pl in enumerate(plans)]
    new = []
    for r, pl in enumerate(plans):
        parts = []
        for q in range(ws):
            a = int(plans[q].send_counts[:r].sum())
            parts.append(sent[q][a:a + int(plans[q].send_counts[r])])
            assert len(parts[-1]) == pl.recv_counts[q]
        received = np.concatenate(parts)
        mine = old[r][pl.local]
        mine[pl.recv_cols] = received[pl.recv_records]
        new.append(mine)
    return np.concatenate(new)


def structured_maps(n):
    c = np.arange(n)
    return [c.copy(), (c - 1) % n, (c + 1) % n, np.full(n, n - 1), np.zeros(n, dtype=np.int64), c[::-1].copy(), np.maximum(c - 1, 0)]


@pytest.mark.parametrize("ws", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1, 2, 7, 130])
def test_resample_plan_is_the_global_gather(pkg, n, ws):
    rng = np.random.default_rng(100 * n + ws)
    tokens = 1000 + 7 * np.arange(n)
    shards = [pkg.shard_columns(n, ws, r) for r in range(ws)]
    for p in structured_maps(n) + [rng.integers(0, n, n) for _ in range(8)]:
        plans = pkg.resample_plan(p, n, ws)
        assert len(plans) == ws
        assert np.array_equal(carry_out(pkg, plans, tokens, n, ws), tokens[p])
        for r, pl in enumerate(plans):
            size = shards[r].stop - shards[r].start
            assert pl.rank == r and pl.ncol == size and pl.local.shape == (size,) and len(pl.send) == ws
            assert len(pl.send[r]) == 0, "nothing is sent to oneself"
            for q in range(ws):
                s = pl.send[q]
                assert np.array_equal(s, np.unique(s)) and ((s >= 0) & (s < size)).all(), "sorted, distinct, local"
                # exactly the parents that rank q names on rank r
                named = np.unique([g - shards[r].start for g in p[shards[q]] if shards[r].start <= g < shards[r].stop])
                assert q == r or np.array_equal(s, named)
            fed = np.zeros(size, dtype=bool)
            fed[pl.recv_cols] = True
            assert len(np.unique(pl.recv_cols)) == len(pl.recv_cols)
            assert (pl.local[fed] == np.flatnonzero(fed)).all(), "a remotely fed column is not moved locally"
            assert (pl.recv_src != r).all()
            for c, q, i in zip(pl.recv_cols, pl.recv_src, pl.recv_idx):
                assert plans[q].send[r][i] + shards[q].start == p[shards[r].start + c]
            assert ((pl.local >= 0) & (pl.local < max(size, 1))).all()
    if ws == 1:
        assert np.array_equal(plans[0].local, p) and not len(plans[0].recv_cols)


def test_resample_plan_refuses_bad_input(pkg):
    for bad in ([0, 1, 2], [0, 1, 2, 3, 4], [0, 1, 2, 4], [0, -1, 2, 3], [0.0, 1.0, 2.0, 3.0], [True, False, True, False],
                [[0, 1], [2, 3]]):
        with pytest.raises(ValueError):
            pkg.resample_plan(np.array(bad), 4, 2)
    with pytest.raises(ValueError):
        pkg.resample_plan(np.arange(4), 4, 0)
    assert len(pkg.resample_plan(np.arange(4), 4, 2)) == 2


# ---- the binding's argument checks ------------------------------------------------------------------------------------------------

def test_engine_checks_raise_before_any_device_call(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)               # no handle: a device call would fail on the missing attributes
    eng.ncol = 5

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    eng.lib, eng._h = NoCalls(), None
    for cols, ptr in (([0, 5], 32), ([-1], 32), ([0.5], 32), ([[0, 1]], 32), ([True], 32), ([0], 24), ([0], 0), ([0], None), ([0], 1.0)):
        with pytest.raises(ValueError):
            eng.export_columns(cols, ptr)
    for cols, ptr, mask, records in (([1, 1], 32, 31, None), ([0, 5], 32, 31, None), ([0], 40, 31, None), ([0, 1], 32, 31, [0]),
                                     ([0, 1], 32, 31, [0, -1]), ([0, 1], 32, 31, [0.0, 1.0]), ([0], 32, -1, None), ([0], 32, 1 << 12, None),
                                     ([0], 32, 1.0, None), ([0], 32, None, None)):
        with pytest.raises(ValueError):
            eng.import_columns(cols, ptr, mask, records)
    c, r = eng.check_exchange_args([4, 0, 4], 32, [2, 0, 2])
    assert c.dtype == np.int32 and r.dtype == np.int32 and c.tolist() == [4, 0, 4] and r.tolist() == [2, 0, 2]
    c, r = eng.check_exchange_args([], 0)
    assert c.shape == (0,) and r is None
    eng._h = None


def test_ensemble_resample_names_what_exists(pkg):
    ensemble = sys.modules[pkg.__name__ + ".ensemble"]
    doc = ensemble.EnsembleRun.resample.__doc__
    assert "rank-local" in doc and "resample_global" in doc and "does not have yet" not in doc
    for name in ("export_tensor", "import_tensor", "resample_export", "resample_import", "resample_global"):
        assert callable(getattr(ensemble.EnsembleRun, name)), name


# ---- the collectives, two ranks over gloo -------------------------------------------------------------------------------------------

WORKER = textwrap.dedent("""
    import sys
    import numpy as np
    import torch
    sys.path.insert(0, {root!r})
    import __graft_entry__ as graft
    import torch.distributed as dist
    pkg = graft.load_package()

    class Rows(pkg.ColumnExchange):
        '''Stand-in for an EnsembleRun: a member's "record" is one row of three numbers.'''
        def __init__(self, rows, mask):
            self.rows, self.mask, self.log = rows.copy(), mask, []
        def export_tensor(self, cols):
            self.log.append(("export", len(cols)))
            return torch.from_numpy(self.rows[np.asarray(cols, dtype=np.int64)].reshape(len(cols), 3).copy()), self.mask
        def import_tensor(self, cols, tensor, mask, records=None):
            assert mask == self.mask
            self.log.append(("import", len(cols)))
            self.rows[np.asarray(cols)] = tensor.numpy()[np.arange(len(cols)) if records is None else np.asarray(records)]
        def resample(self, parents):
            self.log.append(("resample", len(parents)))
            self.rows = self.rows[np.asarray(parents)]

    dist.init_process_group("gloo")
    rank, ws = dist.get_rank(), dist.get_world_size()
    results = {{}}
    for n in (1, 2, 7, 130):
        tokens = np.stack([1000.0 + np.arange(n), -np.arange(n) / 7.0, np.full(n, float(n))], axis=1)
        sl = pkg.shard_columns(n, ws, rank)
        rng = np.random.default_rng(n)                       # the same maps on both ranks
        c = np.arange(n)
        maps = [c.copy(), (c - 1) % n, np.full(n, n - 1), np.zeros(n, dtype=np.int64), np.where(c < (n + 1) // 2, c, c - (n + 1) // 2),
                rng.integers(0, n, n), rng.integers(0, n, n)]
        for i, p in enumerate(maps):
            run = Rows(tokens[sl], 0x7ff)
            run.resample_global(p, n, dist)
            assert [w for w, _ in run.log] == ["export", "resample"] + (["import"] if any(w == "import" for w, _ in run.log) else [])
            full = pkg.gather_columns(run.rows, n, dist)
            if rank == 0:
                assert np.array_equal(full, tokens[p]), (n, i)
                results[f"{{n}}_{{i}}"] = full
    # the ranks must agree on mask and record size: both ranks raise, nobody hangs
    run = Rows(np.zeros((pkg.shard_columns(4, ws, rank).stop - pkg.shard_columns(4, ws, rank).start, 3)), 0x7ff if rank == 0 else 0x1f)
    try:
        run.resample_global(np.array([3, 2, 1, 0]), 4, dist)
        raise SystemExit("a mask mismatch went unnoticed")
    except RuntimeError as err:
        assert "mask" in str(err)
    assert [w for w, _ in run.log] == ["export"], "nothing was written"
    # no process group: the rank-local call
    run = Rows(np.arange(12.0).reshape(4, 3), 1)
    run.resample_global(np.array([1, 1, 3, 0]), 4, None)
    assert run.log == [("resample", 4)]
    if rank == 0:
        np.savez({out!r}, **results)
    dist.barrier()
    dist.destroy_process_group()
""")


def test_two_ranks_exchange_over_gloo(tmp_path, pkg):
    out = str(tmp_path / "gathered.npz")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    subprocess.check_call(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29547", str(script)],
        env=env, timeout=240)
    got = np.load(out)
    assert len(got.files) == 4 * 7
    n = 130
    tokens = np.stack([1000.0 + np.arange(n), -np.arange(n) / 7.0, np.full(n, float(n))], axis=1)
    assert np.array_equal(got["130_1"], tokens[(np.arange(n) - 1) % n])
