"""Shared by test_devgraph_cpu.py and test_gpu_devgraph.py: a sampled block's transpose and
schedules built on the device (pg_csr_transpose_dev / pg_schedule_count_dev /
pg_schedule_build_dev, plagnn.graph.DeviceGraph.from_in_csr, plagnn.graph.DeviceBuiltGraph and
the sampler's block path).

References
  host twins   pg_csr_transpose / pg_schedule_count / pg_schedule_build on the same input are the
               specification: every device array must equal theirs (np.array_equal; integers, no
               tolerance anywhere).
  restatement  independent of both, in numpy: tslot = the stable argsort of col, items = the raw
               list (rows ascending, pieces ascending) under a stable argsort of -(k1 - k0), merges
               stable by -n. Checked against the host twins without a GPU.

Sizes the cases are cut to (pla-gnn_amd/csrc/scan.hpp, graph_dev.hip):
  TILE = 1024             entries per workgroup of a scan and of a radix-sort pass
  TILE_SCAN_PASS = 256    tile totals one pass of the tile scan holds
  ONE_GROUP_CELLS = 8192  cells of a sort's (256 digits x tiles) table that one workgroup scans;
                          above it (more than 32 tiles) the three-kernel scan runs
"""
import functools

import numpy as np
import pytest
import torch

import block_common as bc

TILE = 1024
TILE_SCAN_PASS = 256
ONE_GROUP_CELLS = 8192
CHUNK_PAIRS = [(256, 64), (512, 512), (4, 2), (1, 1)]
NEW_SYMBOLS = ["pg_csr_transpose_dev", "pg_csr_transpose_dev_workspace", "pg_schedule_count_dev",
               "pg_schedule_count_dev_workspace", "pg_schedule_build_dev", "pg_schedule_build_dev_workspace"]


# ------------------------------------------------------------------ cases: (ptr, col, n_src)
def _csr(rows, n_src):
    """In-CSR from a list of rows (each a sequence of source ids)."""
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, col, n_src


def _random(n_dst, n_src, nnz, seed, last_col=True):
    """nnz random entries over n_dst rows (row lengths from a multinomial), one in column n_src - 1."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(n_dst + 1, np.int32)
    ptr[1:] = np.cumsum(rng.multinomial(nnz, np.full(n_dst, 1.0 / n_dst)))
    col = rng.integers(0, n_src, nnz).astype(np.int32)
    if last_col and nnz:
        col[nnz // 2] = n_src - 1
    return ptr, col, n_src


def _rect(ns, nd):
    g = bc.rect(ns, nd)[0]
    return g.fwd.ptr.copy(), g.fwd.col.copy(), ns


def _row_lengths():
    c = 4
    rng = np.random.default_rng(3)
    return _csr([rng.integers(0, 9, d) for d in (0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 1)], 9)


def _hub_column():
    rng = np.random.default_rng(4)
    return _csr([[0, int(rng.integers(1, 50))] for _ in range(3000)], 50)


def _big():
    """More tiles than one pass of the tile scan holds (1025 > TILE_SCAN_PASS), long transposed rows
    (about 1 049 entries per column) and many merges."""
    nnz, n_dst, n_src = TILE * 1024 + 700, 300000, 1000
    rng = np.random.default_rng(6)
    d = np.full(n_dst, 3, np.int64)
    d[:2000] += 70  # rows split at the small chunks and at 64
    d[5] += 600  # and one split at 512
    rest = nnz - int(d.sum())
    d[2000:2000 + rest] += 1
    assert d.sum() == nnz
    ptr = np.zeros(n_dst + 1, np.int32)
    ptr[1:] = np.cumsum(d)
    col = rng.integers(0, n_src, nnz).astype(np.int32)
    col[7] = n_src - 1
    return ptr, col, n_src


CASES = {
    "rect_37x11": lambda: _rect(37, 11),
    "rect_11x37": lambda: _rect(11, 37),
    "no_dst": lambda: _csr([], 5),
    "no_entries": lambda: _csr([[]] * 5, 3),
    "no_src": lambda: _csr([[]] * 4, 0),
    "nothing": lambda: _csr([], 0),
    "empty_tail": lambda: _csr([[1, 0], [2], [0, 0, 1], [], [], []], 7),
    "row_lengths_c4": _row_lengths,
    "duplicates": lambda: _csr([[3, 1], [2, 2, 2, 2, 2, 0], [2]], 4),
    "hub_column": _hub_column,
    "one_column": lambda: _csr([[0, 0], [0], []], 1),
    **{f"digits_{n}": functools.partial(_random, 400, n, 5000, n) for n in (256, 257, 65536, 65537, 70000)},
    **{f"nnz_{n}": functools.partial(_random, 300, 300, n, n) for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)},
    **{f"rows_{n}": functools.partial(_random, n, 40, 3 * n, n) for n in (TILE - 1, TILE, TILE + 1)},
    "scan_switch": lambda: _random(900, 900, ONE_GROUP_CELLS // 256 * TILE + 1, 8),
    "big": _big,
    "row_70000": lambda: _csr([[1], np.random.default_rng(7).integers(0, 30, 70000), [2, 29]], 30),
}
BIG_CASES = ("big",)  # the only input above 100 000 entries


@functools.lru_cache(maxsize=None)
def case(name):
    ptr, col, n_src = CASES[name]()
    assert ptr.dtype == col.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == len(col)
    assert name in BIG_CASES or len(col) <= 100000
    return ptr, col, n_src


def _p(a):
    return a.ctypes.data


# ------------------------------------------------------------------ host twins
@functools.lru_cache(maxsize=None)
def host_transpose(name):
    from plagnn._lib import call

    ptr, col, n_src = case(name)
    nnz = len(col)
    tptr = np.full(n_src + 1, -1, np.int32)
    tcol, tslot, tpos = (np.zeros(max(nnz, 1), np.int32) for _ in range(3))
    colp = col if nnz else np.zeros(1, np.int32)
    call("pg_csr_transpose", _p(ptr), _p(colp), len(ptr) - 1, n_src, nnz, _p(tptr), _p(tcol), _p(tslot), _p(tpos))
    return {"tptr": tptr, "tcol": tcol[:nnz], "tslot": tslot[:nnz], "tpos": tpos[:nnz]}


def host_schedule(ptr, chunk):
    from plagnn.graph import _schedule

    items, n_items, merges, n_merges, n_slots, max_deg = _schedule(np.ascontiguousarray(ptr), chunk)
    d = np.diff(ptr)
    counts = [n_items, n_merges, n_slots, max_deg, int(d.min()) if len(d) else 0, 0]
    return {"counts": counts, "items": items[:4 * n_items], "merges": merges[:4 * n_merges]}


@functools.lru_cache(maxsize=None)
def host_result(name, chunk, chunk_bwd):
    t = host_transpose(name)
    return {**t, "fwd": host_schedule(case(name)[0], chunk), "bwd": host_schedule(t["tptr"], chunk_bwd)}


# ------------------------------------------------------------------ numpy restatement
def numpy_transpose(ptr, col, n_src):
    order = np.argsort(col, kind="stable").astype(np.int32)
    row = np.repeat(np.arange(len(ptr) - 1, dtype=np.int32), np.diff(ptr))
    tptr = np.zeros(n_src + 1, np.int32)
    tptr[1:] = np.cumsum(np.bincount(col, minlength=n_src)) if n_src else 0
    return {"tptr": tptr, "tcol": row[order], "tslot": order, "tpos": order - ptr[row[order]]}


def numpy_schedule(ptr, chunk):
    ptr = ptr.astype(np.int64)
    d = np.diff(ptr)
    n_rows = len(d)
    split = d > chunk
    n = np.where(split, -(-d // chunk), 1)
    first = np.concatenate([[0], np.cumsum(n)])
    slot0 = np.concatenate([[0], np.cumsum(np.where(split, n, 0))])
    row = np.repeat(np.arange(n_rows), n)
    j = np.arange(first[-1]) - first[row]
    k0 = ptr[row] + j * chunk
    k1 = np.minimum(ptr[row + 1], k0 + chunk)
    raw = np.stack([row, k0, k1, np.where(split[row], slot0[row] + j, -1)], 1)
    items = raw[np.argsort(-(k1 - k0), kind="stable")]
    mr = np.nonzero(split)[0]
    mraw = np.stack([mr, slot0[mr], n[mr], np.zeros_like(mr)], 1)
    merges = mraw[np.argsort(-n[mr], kind="stable")]
    counts = [len(items), len(mr), int(slot0[-1]), int(d.max()) if n_rows else 0, int(d.min()) if n_rows else 0, 0]
    return {"counts": counts, "items": items.astype(np.int32).reshape(-1), "merges": merges.astype(np.int32).reshape(-1)}


def same(got, want, what):
    for k in want:
        if isinstance(want[k], dict):
            same(got[k], want[k], f"{what} {k}")
        elif isinstance(want[k], (list, int)):
            assert got[k] == want[k], f"{what}: {k} = {got[k]}, expected {want[k]}"
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), f"{what}: {k} differs"


def check_restatement(name, chunk, chunk_bwd):
    """The numpy restatement agrees with the host functions (no GPU)."""
    ptr, col, n_src = case(name)
    want = host_result(name, chunk, chunk_bwd)
    t = numpy_transpose(ptr, col, n_src)
    got = {**t, "fwd": numpy_schedule(ptr, chunk), "bwd": numpy_schedule(t["tptr"], chunk_bwd)}
    same(got, want, f"{name} numpy restatement against the host functions")


# ------------------------------------------------------------------ the device entry points, raw
class DevRun:
    """One run of the three entry points on `dev` into outputs and workspaces pre-filled with 0xFF
    bytes; the counts are read back between count and build, as the shim does."""

    def __init__(self, dev, ptr, col, n_src, chunk, chunk_bwd, build=True):
        from plagnn import _lib

        self.lib, self.dev, self._lib = _lib.lib(), torch.device(dev), _lib
        self.ptr, self.col = torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev)
        self.n_rows, self.n_src, self.nnz = len(ptr) - 1, n_src, len(col)
        self.tptr = self.ff(n_src + 1)
        self.tcol, self.tslot, self.tpos, self.status = self.ff(self.nnz), self.ff(self.nnz), self.ff(self.nnz), self.ff(1)
        self.transpose()
        self.fcounts = self.count(self.ptr, chunk)
        self.bcounts = self.count(self.tptr, chunk_bwd)
        self.out = {"tptr": self.np(self.tptr), "tcol": self.np(self.tcol), "tslot": self.np(self.tslot),
                    "tpos": self.np(self.tpos), "status": int(self.status.item())}
        if build:
            self.out["fwd"] = self.build(self.ptr, chunk, self.fcounts)
            self.out["bwd"] = self.build(self.tptr, chunk_bwd, self.bcounts)

    def ff(self, n, dtype=torch.int32):
        return torch.full((max(int(n), 1),), -1, dtype=dtype, device=self.dev)[:int(n)] if n else \
            torch.full((1,), -1, dtype=dtype, device=self.dev)[:0]

    def ws(self, nbytes):
        return torch.full((max(int(nbytes), 256),), 255, dtype=torch.uint8, device=self.dev)

    @staticmethod
    def np(t):
        return t.cpu().numpy()

    def stream(self):
        return self._lib.stream_handle(self.dev)

    def transpose(self, ws=None):
        L, p = self.lib, self._lib.ptr
        ws = self.ws(L.pg_csr_transpose_dev_workspace(self.n_rows, self.n_src, self.nnz)) if ws is None else ws
        self._lib.call("pg_csr_transpose_dev", p(self.ptr), p(self.col), self.n_rows, self.n_src, self.nnz, p(self.tptr),
                       p(self.tcol), p(self.tslot), p(self.tpos), p(self.status), p(ws), ws.numel(), self.stream())

    def count(self, ptr, chunk):
        L, p = self.lib, self._lib.ptr
        counts = self.ff(6, torch.int64)
        ws = self.ws(L.pg_schedule_count_dev_workspace(ptr.numel() - 1))
        self._lib.call("pg_schedule_count_dev", p(ptr), ptr.numel() - 1, chunk, p(counts), p(ws), ws.numel(), self.stream())
        return counts.tolist()

    def build(self, ptr, chunk, counts, items=None, merges=None, ws=None):
        L, p = self.lib, self._lib.ptr
        n_items, n_merges, _, max_deg = counts[:4]
        items = self.ff(4 * n_items) if items is None else items
        merges = self.ff(4 * n_merges) if merges is None else merges
        ws = self.ws(L.pg_schedule_build_dev_workspace(ptr.numel() - 1, n_items, n_merges)) if ws is None else ws
        self._lib.call("pg_schedule_build_dev", p(ptr), ptr.numel() - 1, chunk, n_items, n_merges, max_deg, p(items),
                       p(merges), p(ws), ws.numel(), self.stream())
        return {"counts": list(counts), "items": self.np(items), "merges": self.np(merges)}


def check_kernels(dev, name, chunk, chunk_bwd):
    """Two runs into 0xFF-filled buffers: identical, equal to the host functions and to numpy."""
    ptr, col, n_src = case(name)
    want = host_result(name, chunk, chunk_bwd)
    a = DevRun(dev, ptr, col, n_src, chunk, chunk_bwd).out
    b = DevRun(dev, ptr, col, n_src, chunk, chunk_bwd).out
    assert a["status"] == 0 and b["status"] == 0
    same(a, want, f"{name} chunks ({chunk}, {chunk_bwd}) against the host functions")
    same(b, a, f"{name} chunks ({chunk}, {chunk_bwd}): the second run against the first")
    t = numpy_transpose(ptr, col, n_src)
    same(a, {**t, "fwd": numpy_schedule(ptr, chunk), "bwd": numpy_schedule(t["tptr"], chunk_bwd)},
         f"{name} chunks ({chunk}, {chunk_bwd}) against the numpy restatement")


def check_arg_kind(dev):
    """One row of 70 000 entries: max_deg >= 0xFFFF, so the records are int32."""
    from plagnn import _lib
    from plagnn.graph import DeviceGraph

    ptr, col, n_src = case("row_70000")
    dg = DeviceGraph.from_in_csr(torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), n_src)
    assert dg.fwd.max_deg == 70000 and dg.arg_kind == _lib.PG_ARG_I32 and dg.arg_dtype == torch.int32
    ptr, col, n_src = case("rect_37x11")
    dg = DeviceGraph.from_in_csr(torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), n_src)
    assert dg.arg_kind == _lib.PG_ARG_U16 and dg.arg_dtype == torch.int16


BAD_INPUTS = {
    "col_equals_n_cols": (np.array([0, 2, 3], np.int32), np.array([1, 4, 0], np.int32), 4),
    "negative_col": (np.array([0, 2, 3], np.int32), np.array([1, -1, 0], np.int32), 4),
    "ptr_not_monotone": (np.array([0, 3, 2, 5], np.int32), np.array([1, 0, 2, 3, 1], np.int32), 4),
}


def check_bad_input(dev, which):
    """The status is set and from_in_csr raises; every kernel bounds-checks before it indexes, so
    the process simply goes on (the next test runs in it)."""
    from plagnn.graph import DeviceGraph

    ptr, col, n_src = BAD_INPUTS[which]
    run = DevRun(dev, ptr, col, n_src, 4, 2, build=False)
    if which == "ptr_not_monotone":
        assert run.fcounts[5] < 0 and run.out["status"] == 0
    else:
        assert run.out["status"] < 0 and run.fcounts[5] == 0
    with pytest.raises(ValueError):
        DeviceGraph.from_in_csr(torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), n_src, 4, 2)
    good = case("duplicates")
    DeviceGraph.from_in_csr(torch.from_numpy(good[0]).to(dev), torch.from_numpy(good[1]).to(dev), good[2])


def check_capture(dev):
    """pg_csr_transpose_dev + pg_schedule_build_dev captured on one stream, replayed twice into
    cleared outputs: the replays equal the eager result."""
    name, chunk, chunk_bwd = "rect_37x11", 256, 64
    ptr, col, n_src = case(name)
    eager = DevRun(dev, ptr, col, n_src, chunk, chunk_bwd)
    outs = [eager.tptr, eager.tcol, eager.tslot, eager.tpos, eager.status]
    ni, nm = eager.fcounts[0], eager.fcounts[1]
    items, merges = eager.ff(4 * ni), eager.ff(4 * nm)
    ws = eager.ws(eager.lib.pg_schedule_build_dev_workspace(eager.n_rows, ni, nm))
    ws_t = eager.ws(eager.lib.pg_csr_transpose_dev_workspace(eager.n_rows, n_src, eager.nnz))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # the calls below take torch's current stream: the capturing one
        eager.transpose(ws_t)
        eager._lib.call("pg_schedule_build_dev", eager._lib.ptr(eager.ptr), eager.n_rows, chunk, ni, nm,
                        eager.fcounts[3], eager._lib.ptr(items), eager._lib.ptr(merges), eager._lib.ptr(ws), ws.numel(),
                        eager.stream())
    want = host_result(name, chunk, chunk_bwd)
    for _ in range(2):
        for t in outs + [items, merges]:
            t.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        got = {"tptr": eager.np(eager.tptr), "tcol": eager.np(eager.tcol), "tslot": eager.np(eager.tslot),
               "tpos": eager.np(eager.tpos), "items": eager.np(items), "merges": eager.np(merges)}
        same(got, {**{k: want[k] for k in ("tptr", "tcol", "tslot", "tpos")}, "items": want["fwd"]["items"],
                   "merges": want["fwd"]["merges"]}, "replay against the host functions")
        same(got, {**{k: eager.out[k] for k in ("tptr", "tcol", "tslot", "tpos")}, "items": eager.out["fwd"]["items"],
                   "merges": eager.out["fwd"]["merges"]}, "replay against the eager run")
        assert int(eager.status.item()) == 0


# ------------------------------------------------------------------ graph.py
CSR_FIELDS = ("ptr", "col", "eslot", "epos", "items", "merges")
CSR_SCALARS = ("n_rows", "n_cols", "nnz", "n_items", "n_merges", "n_slots", "max_deg", "chunk")


def same_device_graph(a, b, what):
    assert (a.num_src, a.num_dst, a.num_edges, a.arg_kind, a.arg_dtype) == \
           (b.num_src, b.num_dst, b.num_edges, b.arg_kind, b.arg_dtype), what
    assert a.eid.dtype == b.eid.dtype and torch.equal(a.eid.cpu(), b.eid.cpu()), f"{what}: eid"
    for side in ("fwd", "bwd"):
        x, y = getattr(a, side), getattr(b, side)
        for f in CSR_SCALARS:
            assert getattr(x, f) == getattr(y, f), f"{what}: {side}.{f} = {getattr(x, f)}, expected {getattr(y, f)}"
        for f in CSR_FIELDS:
            s, t = getattr(x, f), getattr(y, f)
            assert (s is None) == (t is None), f"{what}: {side}.{f}"
            if s is not None:
                assert s.dtype == t.dtype and s.shape == t.shape and np.array_equal(s.cpu().numpy(), t.cpu().numpy()), \
                    f"{what}: {side}.{f} differs"


def check_from_in_csr(dev, name, chunk=256, chunk_bwd=None):
    """DeviceGraph.from_in_csr on `dev` equals CSRGraph.from_in_csr(...).on(dev), field by field."""
    import plagnn
    from plagnn.graph import DeviceGraph

    ptr, col, n_src = case(name)
    want = plagnn.CSRGraph.from_in_csr(ptr, col, n_src, chunk, chunk_bwd).on(dev)
    got = DeviceGraph.from_in_csr(torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), n_src, chunk, chunk_bwd)
    assert got.device.type == torch.device(dev).type
    same_device_graph(got, want, f"from_in_csr {name} on {dev}")
    assert np.array_equal(got.in_degrees().cpu().numpy(), np.diff(ptr))
    assert np.array_equal(got.out_degrees().cpu().numpy(), np.bincount(col, minlength=n_src))


def check_zero_in_degree_host():
    import plagnn

    for name in ("rect_37x11", "no_dst", "no_entries", "empty_tail", "hub_column", "one_column"):
        ptr, col, n_src = case(name)
        g = plagnn.CSRGraph.from_in_csr(ptr, col, n_src)
        assert g.has_zero_in_degree() is bool((g.in_degrees() == 0).any()), name


def check_zero_in_degree_device(dev):
    from plagnn.graph import DeviceBuiltGraph

    for name in ("rect_37x11", "no_dst", "no_entries", "empty_tail", "hub_column", "one_column"):
        ptr, col, n_src = case(name)
        o = DeviceBuiltGraph(torch.from_numpy(ptr).to(dev), torch.from_numpy(col).to(dev), n_src)
        assert o.has_zero_in_degree() is bool((np.diff(ptr) == 0).any()), name
        assert o.host is None and (o.num_src, o.num_dst, o.num_edges) == (n_src, len(ptr) - 1, len(col))
        assert np.array_equal(o.in_degrees(), np.diff(ptr)) and o.host is not None, "in_degrees() builds the host graph"


def check_exports():
    from plagnn import _lib

    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.pg_version() == 13


# ------------------------------------------------------------------ the sampler's block path
def hub_parent(dev):
    """bc.sampler_graph()'s parent (the graph with the hub rows) as a dgl graph, edges in id order."""
    import dgl

    g, k = bc.sampler_graph()
    dst_slot = np.repeat(np.arange(g.num_dst, dtype=np.int64), np.diff(g.fwd.ptr))
    src, dst = np.empty(g.num_edges, np.int64), np.empty(g.num_edges, np.int64)
    src[g.eid], dst[g.eid] = g.fwd.col, dst_slot
    return dgl.graph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=g.num_dst).to(dev), k


def sample_both(dev, g, fanouts, seeds):
    """The same blocks through the host build and the device build."""
    import dgl
    from dgl.dataloading import NeighborSampler
    from plagnn import graph as eg

    res = []
    old = eg.DEVICE_BUILD
    try:
        for flag in (False, True):
            eg.DEVICE_BUILD = flag
            dgl.seed(17)
            res.append(NeighborSampler(fanouts).sample_blocks(g, seeds))
    finally:
        eg.DEVICE_BUILD = old
    return res


def check_paths_equal(dev, which):
    import dgl
    import dgl.nn.pytorch as dnn
    from plagnn.graph import CSRGraph, DeviceBuiltGraph

    if which == "parent":
        g, fanouts = bc.parent_graph(dev), [3, 4]
        seeds = torch.from_numpy(np.random.default_rng(1).permutation(g.num_nodes())[:40].copy())
    else:
        (g, k), fanouts = hub_parent(dev), [5, 70]
        seeds = torch.cat([torch.arange(k), torch.tensor([650, 699, 20])])
    (inp_h, out_h, bl_h), (inp_d, out_d, bl_d) = sample_both(dev, g, fanouts, seeds)
    assert torch.equal(inp_h, inp_d) and torch.equal(out_h, out_d) and len(bl_h) == len(bl_d) == 2
    for i, (h, d) in enumerate(zip(bl_h, bl_d)):
        assert isinstance(h._csr_cache["host"], CSRGraph) and isinstance(d._csr_cache["host"], DeviceBuiltGraph)
        same_device_graph(d._device_graph(dev), h._device_graph(dev), f"{which} block {i}")
        assert d._csr_cache["host"].host is None
        for x, y in zip(h.edges(), d.edges()):
            assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu())
        assert torch.equal(h.srcdata[dgl.NID], d.srcdata[dgl.NID]) and torch.equal(h.edata[dgl.EID], d.edata[dgl.EID])
    if which == "hubs":  # the hub rows reach the fanout
        assert bl_d[1]._device_graph(dev).fwd.max_deg == 70 and bl_d[0]._device_graph(dev).fwd.max_deg == 5
    fin = 12
    x = bc.gc._randn(np.random.default_rng(2), g.num_nodes(), fin)
    torch.manual_seed(3)
    l1, l2 = dnn.SAGEConv(fin, 8, "pool").to(dev), dnn.SAGEConv(8, 6, "pool").to(dev)
    res = []
    for inp, blocks in ((inp_h, bl_h), (inp_d, bl_d)):
        for p in list(l1.parameters()) + list(l2.parameters()):
            p.grad = None
        xd = bc._leaf(x, dev)
        h = torch.relu(l1(blocks[0], xd[inp.to(dev)]))
        h = l2(blocks[1], h)
        (h * h).sum().backward()
        res.append([h.detach(), xd.grad] + [p.grad.clone() for p in list(l1.parameters()) + list(l2.parameters())])
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), f"{which}: tensor {i} of the two paths differs"


def check_no_host_graph(dev):
    """The default switch on a HIP device: sampling and one forward and backward of four layers
    build no host CSRGraph; b.to('cpu') + update_all builds it lazily and gives the device result."""
    import dgl
    import dgl.function as fn
    import dgl.nn.pytorch as dnn
    from dgl.dataloading import NeighborSampler
    from plagnn import graph as eg
    from plagnn.graph import DeviceBuiltGraph

    assert eg.DEVICE_BUILD is True
    g = bc.parent_graph(dev)
    dgl.seed(2)
    seeds = torch.arange(30)
    inp, out, blocks = NeighborSampler([3, 4]).sample_blocks(g, seeds)
    owners = [b._csr_cache["host"] for b in blocks]
    assert all(isinstance(o, DeviceBuiltGraph) for o in owners)
    assert all(b._src.device.type == "cuda" and b._dst.device.type == "cuda" for b in blocks)
    x = bc.gc._randn(np.random.default_rng(5), g.num_nodes(), 8)
    torch.manual_seed(4)
    for make in (lambda: dnn.SAGEConv(8, 8, "pool"), lambda: dnn.GATConv(8, 4, 2), lambda: dnn.GATv2Conv(8, 4, 2),
                 lambda: dnn.GraphConv(8, 8, norm="right")):
        l1, l2 = make().to(dev), make().to(dev)
        xd = bc._leaf(x, dev)
        h = torch.relu(l1(blocks[0], xd[inp.to(dev)])).flatten(1)
        h = l2(blocks[1], h).flatten(1)
        assert h.shape[0] == len(seeds)
        h.sum().backward()
        assert xd.grad is not None and all(p.grad is not None for p in l1.parameters())
    assert all(o.host is None for o in owners), "a layer asked for host arrays"
    b = blocks[1]
    hsrc = bc.gc._randn(np.random.default_rng(6), b.num_src_nodes(), 5)
    b.srcdata["h"] = hsrc.to(dev)
    b.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
    on_dev = b.dstdata["o"].cpu()
    assert owners[1].host is None
    c = b.to("cpu")
    assert c.srcdata["h"].device.type == "cpu"
    c.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
    assert owners[1].host is not None, "the CPU device needs the host graph"
    assert torch.equal(c.dstdata["o"], on_dev)


def check_empty_seeds(dev):
    import dgl
    import dgl.function as fn
    from dgl.dataloading import NeighborSampler

    src, dst = torch.tensor([0, 1, 2, 2]), torch.tensor([1, 2, 0, 1])
    g = dgl.graph((src, dst), num_nodes=6).to(dev)  # nodes 3, 4, 5 have no in-edges
    for seeds, n in ((torch.zeros(0, dtype=torch.int64), 0), (torch.tensor([4, 3, 5]), 3)):
        inp, out, blocks = NeighborSampler([2, 2]).sample_blocks(g, seeds)
        assert len(inp) == n and len(out) == n and len(blocks) == 2
        for b in blocks:
            assert (b.num_src_nodes(), b.num_dst_nodes(), b.num_edges()) == (n, n, 0)
            dg = b._device_graph(dev)
            assert (dg.num_src, dg.num_dst, dg.num_edges, dg.fwd.n_items, dg.bwd.n_items, dg.fwd.n_merges) == (n, n, 0, n, n, 0)
            assert b._engine_graph().has_zero_in_degree() is (n > 0)
            if n:  # rows without entries aggregate to zero
                b.srcdata["h"] = torch.ones(n, 3, device=dev)
                b.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
                assert tuple(b.dstdata["o"].shape) == (n, 3) and not b.dstdata["o"].any()
