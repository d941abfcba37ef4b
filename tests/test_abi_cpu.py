"""CPU tests (no GPU): the C-ABI library loads and exports every symbol include/cytohip.h declares,
argument validation that needs no device, host-side logic, and a world_size-2 gloo run of the
chunk scheduler."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from cytospace_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "cytohip.h")).read()
    names = sorted(set(re.findall(r"\b(cyto_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 14
    for nme in names:
        assert hasattr(L, nme), f"{nme} declared in cytohip.h but not exported"
    # the block cache's test hook (tests/test_work_buffers_gpu.py) is part of the header, so the loop above covers it
    for nme in ("cyto_trim_device_cache", "cyto_cache_poison", "cyto_cache_poison_fills", "cyto_cache_poison_bytes", "cyto_cache_peek"):
        assert nme in names and hasattr(L, nme), nme
    assert L.cyto_version().decode().startswith("cytohip")
    assert L.cyto_strerror(2).decode() == "cost matrix contains NaN or Inf"


def test_cache_poison_switch_needs_no_device():
    # cyto_cache_poison: a process-wide switch held in atomics; 0...255 on, -1 off, anything else CYTO_ERR_BAD_ARG; nothing is
    # filled (and no device is touched) until a block is handed out
    from cytospace_amd import _lib
    L = _lib.lib()
    f0, b0 = _lib.cache_poison_fills(), _lib.cache_poison_bytes()
    try:
        for bad in (-2, 256, 1000, -(2**31)):
            assert L.cyto_cache_poison(bad) == 1
        for ok in (0, 0x7F, 0x80, 0xFF, -1):
            assert L.cyto_cache_poison(ok) == 0
        _lib.cache_poison(0xFF)
        _lib.cache_poison(None)
        room = np.zeros(8, np.uint8)
        assert L.cyto_cache_peek(0, room.ctypes.data, 0) == 1 and L.cyto_cache_peek(8, None, 0) == 1      # before any device call
    finally:
        L.cyto_cache_poison(-1)
    assert (_lib.cache_poison_fills(), _lib.cache_poison_bytes()) == (f0, b0)
    assert L.cyto_cache_poison_fills.restype is ctypes.c_longlong and L.cyto_cache_poison_bytes.restype is ctypes.c_longlong


def test_build_source_list_is_the_csrc_directory():
    # every csrc/*.hip is compiled into the library, and every entry of the list exists
    from cytospace_amd import build
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(build.SOURCES) == on_disk
    assert len(set(build.SOURCES)) == len(build.SOURCES)


def test_status_to_exception_mapping():
    from cytospace_amd import _lib
    _lib.lib()
    with pytest.raises(ValueError):
        _lib.check(1)
    with pytest.raises(ValueError):
        _lib.check(2)
    with pytest.raises(MemoryError):
        _lib.check(3)
    with pytest.raises(_lib.CytoHipError):
        _lib.check(4)
    _lib.check(0)


def test_no_cpu_fallback_product_fails_loudly_without_device():
    from cytospace_amd import _lib
    from cytospace_amd.lap import lap_solve
    if _lib.device_count() > 0:
        pytest.skip("a device is visible")
    with pytest.raises(Exception):
        lap_solve(np.ones((4, 4), np.float32))


def test_python_argument_validation():
    from cytospace_amd.lap import lap_solve
    with pytest.raises(ValueError):
        lap_solve(np.zeros((3, 4), np.float32))
    with pytest.raises(TypeError):
        lap_solve(np.zeros((3, 3)), dtype=np.int32)
    from cytospace_amd import linear_assignment_solvers as gs
    assert "lapjv_hip" in gs.SOLVER_METHODS
    assert gs.import_solver("lapjv_hip").__name__ == "lapjv_hip"
    with pytest.raises(NotImplementedError):
        gs.import_solver("bogus")
    import pickle
    assert pickle.loads(pickle.dumps(gs.import_solver("lapjv_hip"))) is gs.import_solver("lapjv_hip")  # picklable callable


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cytospace_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f


def test_partition_indices_matches_golden():
    from cytospace_amd.cytospace import partition_indices
    d = np.load(os.path.join(ROOT, "tests", "golden", "gv6_partition.npz"))
    p = partition_indices(np.arange(0, 1800), np.array([500, 1000, 300]), 400, shuffle=False)
    assert np.array_equal([len(x) for x in p], d["ex2_lens"]) and np.array_equal([x[0] for x in p], d["ex2_first"])
    np.random.seed(5)
    p = partition_indices(np.arange(0, 37), split_by_interval_int=10, shuffle=True)
    assert np.array_equal(np.concatenate(p), d["shuf_concat"])


def test_schedule_chunks_lpt():
    from cytospace_amd.cytospace import schedule_chunks
    owner = schedule_chunks([10000, 10000, 10000, 10000, 5000, 5000, 5000, 5000], 4)
    assert sorted(owner[:4]) == [0, 1, 2, 3]            # the four big chunks go to four different devices
    assert len(set(owner)) == 4
    assert schedule_chunks([5, 3], 1) == [0, 0]


_GLOO_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch.distributed as dist
from cytospace_amd.cytospace import schedule_chunks, partition_indices
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
idx = partition_indices(np.arange(2300), split_by_interval_int=500, shuffle=False)
owner = schedule_chunks([len(i) for i in idx], world)
mine = [k for k in range(len(idx)) if owner[k] == rank]
got = [None] * world
dist.all_gather_object(got, mine)
allc = sorted(sum(got, []))
assert allc == list(range(len(idx))), allc          # every chunk solved exactly once
assert all(len(g) > 0 for g in got)
dist.barrier()
if rank == 0:
    print("GLOO_OK", got)
"""


def test_chunk_sharding_world_size_2_gloo(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(_GLOO_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29517", str(script), ROOT],
                       capture_output=True, text=True, timeout=280, env=env)
    assert "GLOO_OK" in r.stdout, r.stdout + r.stderr


def test_gv7_upstream_sampler_and_type_numbers_match_the_reference():
    # host-side functions upstream of apply_linear_assignment (cytospace.py:137-147, 212-301) vs arrays captured from
    # the reference: integer cell numbers per type, and the seeded cell sampler in both of its modes
    import pandas as pd
    from cytospace_amd import cytospace as gcyto
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gv7_upstream.npz"))
    frac_df = pd.DataFrame(d["fractions"], index=["Fraction"], columns=["TYPE_A", "TYPE_B", "TYPE_C"])
    for total in (101, 7):
        got = gcyto.get_cell_type_fraction(total, frac_df.copy())
        assert list(got.index) == ["TYPE_A", "TYPE_B", "TYPE_C"] and int(got.values.sum()) == total
        assert np.array_equal(got.values[:, 0].astype(np.int64), d[f"numbers_{total}"])
    sc = d["sc_counts"]
    G, C = sc.shape
    sc_df = pd.DataFrame(sc, index=[f"g{i}" for i in range(G)], columns=[f"CELL_{i}" for i in range(C)])
    ct_df = pd.DataFrame(d["sc_labels"], index=sc_df.columns, columns=["CellType"])
    need = pd.DataFrame(d["need"], index=["TYPE_A", "TYPE_B", "TYPE_C"], columns=["Fraction"])
    for seed in (1, 4):
        dup = gcyto.sample_single_cells(sc_df, ct_df, need, "duplicates", seed)
        assert np.array_equal(np.array([int(x.split("_")[1]) for x in dup.columns]), d[f"dup_s{seed}_cells"])
        ph = gcyto.sample_single_cells(sc_df, ct_df, need, "place_holders", seed)
        assert list(ph.columns) == list(d[f"ph_s{seed}_names"]) and np.array_equal(ph.to_numpy(), d[f"ph_s{seed}_values"])
    with pytest.raises(ValueError):
        gcyto.sample_single_cells(sc_df, ct_df, need, "bootstrap", 1)
    with pytest.raises(ValueError):
        gcyto.sample_single_cells(sc_df, ct_df, pd.DataFrame([3], index=["TYPE_Z"], columns=["Fraction"]), "duplicates", 1)


def test_c_abi_argument_validation_needs_no_device():
    # the entry points validate their arguments before they touch HIP: status codes only, no device required
    from cytospace_amd import _lib
    L = _lib.lib()
    BAD = 1   # CYTO_ERR_BAD_ARG
    x = np.zeros((4, 4), np.float64)
    assert L.cyto_lap_f32(0, None, 0, 0, None, None, None, None, None, None, 0, None) == BAD
    assert L.cyto_lap_f32(4, x.ctypes.data, 3, 0, None, None, None, None, None, None, 0, None) == BAD      # ld < n
    assert L.cyto_transform(7, 4, 4, x.ctypes.data, 4, 1, 0, 1, x.ctypes.data, 4, 4, 0, None) == BAD       # unknown transform
    assert L.cyto_transform(0, 4, 4, x.ctypes.data, 2, 1, 0, 1, x.ctypes.data, 4, 4, 0, None) == BAD       # ldx < C
    slots = np.ones(4, np.int64)
    assert L.cyto_cost_metric(5, 32, 4, 4, x.ctypes.data, 128, x.ctypes.data, 128, slots.ctypes.data, x.ctypes.data, 4, None, 0, None) == BAD
    assert L.cyto_assign_metric(9, 4, 4, 4, x.ctypes.data, x.ctypes.data, slots.ctypes.data, 1, slots.ctypes.data, None, None, 0) == BAD
    bad_slots = np.array([1, 1, 1, 2], np.int64)                                                            # sum != C
    assert L.cyto_assign_metric(0, 4, 4, 4, x.ctypes.data, x.ctypes.data, bad_slots.ctypes.data, 1, slots.ctypes.data, None, None, 0) == BAD
    h = ctypes.c_void_p()
    assert L.cyto_ctx_create(3, 4, 4, 4, x.ctypes.data, x.ctypes.data, 1, 0, ctypes.byref(h)) == BAD      # unknown metric
    assert L.cyto_ctx_create(0, 4, 0, 4, x.ctypes.data, x.ctypes.data, 1, 0, ctypes.byref(h)) == BAD      # empty matrix
    assert L.cyto_ctx_assign_chunk(None, slots.ctypes.data, 4, None, 0, slots.ctypes.data, slots.ctypes.data, None, None) == BAD
    L.cyto_ctx_destroy(None)                                                                                # no-op
    assert L.cyto_strerror(1).decode() != ""


# ---- the output writers against files the reference itself wrote (tests/golden/gv12_outputs.npz) ----

def _gv12_toy(method):
    import pandas as pd
    rng = np.random.default_rng(12)
    G, C, S = 7, 14, 6
    genes = [f"GENE_g{i}" for i in range(G)]
    cells = [f"CELL_c{i}" for i in range(C)]
    types_ = ["TYPE_B", "TYPE_T", "TYPE_Mono"]
    ctd = pd.DataFrame({"CellType": [types_[i % 3] for i in range(C)]}, index=cells)
    expr = pd.DataFrame(rng.poisson(2.0, (G, C)), index=genes, columns=cells)
    coords = pd.DataFrame({"row": np.arange(S) // 3, "col": np.arange(S) % 3}, index=[f"SPOT_s{i}" for i in range(S)])
    picked = [cells[i] for i in (3, 0, 7, 7, 12, 5, 9, 1, 3, 13, 2)]
    if method == "place_holders":
        extra = [f"CELL_{t[5:]}_new_{k + 1}" for k, t in enumerate(["TYPE_B", "TYPE_Mono"])]
        for e in extra:
            expr[e] = rng.poisson(2.0, G)
        picked = picked[:9] + extra
    spots = [coords.index[i] for i in (0, 0, 1, 3, 3, 3, 4, 1, 0, 4, 3)]
    return picked, expr, coords.loc[spots], ctd, coords


@pytest.mark.parametrize("method", ["duplicates", "place_holders"])
@pytest.mark.parametrize("single", [False, True])
def test_gv12_output_files_equal_the_references(method, single, tmp_path):
    from cytospace_amd.post_processing import save_results, save_unassigned_locations
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gv12_outputs.npz"))
    picked, expr, assigned, ctd, coords = _gv12_toy(method)
    save_results(str(tmp_path), "p_", np.array(picked), expr, assigned, ctd, method, single)
    assert save_unassigned_locations(str(tmp_path), "p_", coords.index, assigned, coords) == 2
    tag = f"{method}_{'sc' if single else 'spot'}"
    want = {k.split("::", 1)[1]: bytes(gold[k].tobytes()) for k in gold.files if k.startswith(tag + "::")}
    got = {}
    for root, _, files in os.walk(str(tmp_path)):
        for f in files:
            got[os.path.relpath(os.path.join(root, f), str(tmp_path))] = open(os.path.join(root, f), "rb").read()
    assert sorted(got) == sorted(want)

    def norm(name, b):          # scipy's MatrixMarket header carries no date, but be robust to comment lines
        return b"\n".join(l for l in b.split(b"\n") if not (name.endswith(".mtx") and l.startswith(b"%") and not l.startswith(b"%%")))
    for name in want:
        assert norm(name, got[name]) == norm(name, want[name]), name


def test_gv13_downsample_equals_the_references():
    # cytospace/common/common.py:149-173 (legacy RandomState draws): same seed, same counts as the reference produced
    import pandas as pd
    from cytospace_amd.common import downsample
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gv13_downsample.npz"))
    df = pd.DataFrame(d["counts"], index=[f"GENE_{i}" for i in range(40)], columns=[f"CELL_{i}" for i in range(9)])
    np.random.seed(int(d["seed"]))
    out = downsample(df, int(d["target"]))
    assert np.array_equal(out.to_numpy(), d["out"])
    assert list(out.index) == list(df.index) and list(out.columns) == list(df.columns)


def test_read_file_matrix_market_and_tables(tmp_path):
    # cytospace/common/common.py:16-82: 10x-style directory (matrix.mtx + genes.tsv + barcodes.tsv) and delimited tables
    import pandas as pd
    import scipy.io
    import scipy.sparse as sp
    from cytospace_amd.common import read_file
    rng = np.random.default_rng(2)
    m = sp.random(12, 7, density=0.3, random_state=3, data_rvs=lambda k: rng.integers(1, 9, k)).tocoo()
    scipy.io.mmwrite(str(tmp_path / "matrix.mtx"), m)
    pd.Series([f"g{i}" for i in range(12)]).to_csv(tmp_path / "genes.tsv", sep="\t", header=False, index=False)
    pd.Series([f"c{i}" for i in range(7)]).to_csv(tmp_path / "barcodes.tsv", sep="\t", header=False, index=False)
    df = read_file(str(tmp_path / "matrix.mtx"))
    assert df.shape == (12, 7) and list(df.index[:2]) == ["g0", "g1"] and list(df.columns[:2]) == ["c0", "c1"]
    assert np.array_equal(df.sparse.to_coo().toarray(), m.toarray())
    dense = read_file(str(tmp_path / "matrix.mtx"), keep_sparse=False)
    assert np.array_equal(dense.to_numpy(), m.toarray())
    t = pd.DataFrame(m.toarray(), index=[f"g{i}" for i in range(12)], columns=[f"c{i}" for i in range(7)])
    t.to_csv(tmp_path / "t.csv")
    t.to_csv(tmp_path / "t.txt", sep="\t")
    for name in ("t.csv", "t.txt"):
        back = read_file(str(tmp_path / name))
        assert np.array_equal(back.to_numpy(), m.toarray()) and list(back.index) == list(t.index)
    with pytest.raises(IOError):
        read_file(str(tmp_path / "missing" / "matrix.mtx"))


def test_batch_return_status_without_a_device(monkeypatch):
    # lap_solve_batch(..., return_status=True): a problem with non-finite costs is a status and a None, not an exception for the
    # call; every other status still raises.  The batch entry point is replaced by a stand-in that writes statuses (no device).
    from cytospace_amd import _lib
    from cytospace_amd.lap import lap_solve_batch, lap_solve_batch_device
    real = _lib.lib()
    plan = {}

    class StandIn:
        def __getattr__(self, name):
            return getattr(real, name)

        def cyto_lap_batch_f32_opts(self, nb, ns, cost, lds, on_device, rowsol, colsol, u, v, totals, infos, status, conc, dev, opts):
            first = 0
            for b in range(nb):
                status[b] = plan["status"][b]
                totals[b] = 10.0 + b
                first = first or status[b]
            return first

    monkeypatch.setattr(_lib, "lib", lambda: StandIn())
    costs = [np.zeros((3, 3), np.float32) for _ in range(4)]
    plan["status"] = [0, 2, 0, 2]
    with pytest.raises(ValueError):
        lap_solve_batch(costs)                                         # the default: the first status raises
    outs, status = lap_solve_batch(costs, return_status=True, return_info=True)
    assert status == [0, 2, 0, 2] and outs[1] is None and outs[3] is None
    assert outs[0]["total"] == 10.0 and outs[2]["total"] == 12.0 and "info" in outs[2] and outs[0]["colsol"].shape == (3,)
    outs, status = lap_solve_batch_device([16, 32], [3, 3], return_status=True)
    assert status == [0, 2] and outs[1] is None and outs[0]["total"] == 10.0
    plan["status"] = [0, 0, 0, 0]
    outs, status = lap_solve_batch(costs, return_status=True)
    assert status == [0, 0, 0, 0] and all(o is not None for o in outs)
    assert [o["total"] for o in lap_solve_batch(costs)] == [10.0, 11.0, 12.0, 13.0]
    for code, exc in ((1, ValueError), (3, MemoryError), (4, _lib.CytoHipError), (5, _lib.CytoHipError)):
        plan["status"] = [0, 2, code, 0]                                  # not a problem's own status: raises either way
        with pytest.raises(exc):
            lap_solve_batch(costs, return_status=True)
    assert lap_solve_batch([]) == [] and lap_solve_batch([], return_status=True) == ([], [])
