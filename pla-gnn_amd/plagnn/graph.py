"""Graph storage for the message-passing engine.

Host side: the COO edge list (self-loops already appended, code/utils.py:44-45) becomes
an in-CSR (DGL's CSC: rows = destinations, each row in ascending edge id) and its
transpose (rows = sources, destinations ascending, with the in-CSR slot of every edge),
plus the longest-first work schedules the kernels consume. All of it is built by the
C-ABI host entry points (pg_csr_from_coo / pg_csr_transpose / pg_schedule_*).

Device side: one ``DeviceGraph`` per torch device, uploaded once and cached; int32 ids
throughout (DGL uses int64), the compact per-row argmax positions are u16 whenever the
largest in-degree allows (else int32).

A sampled block's in-CSR is born on the device: ``DeviceGraph.from_in_csr`` builds its transpose
and both schedules there (pg_csr_transpose_dev / pg_schedule_count_dev / pg_schedule_build_dev,
the twins of the host calls, equal to them bit for bit) with one small read-back of the counts,
and ``DeviceBuiltGraph`` stands in for the host ``CSRGraph`` until something asks for host arrays.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import PgCsr, call

# in-CSR entries per forward work item before a row is split (CSRGraph(chunk=...))
DEFAULT_CHUNK = 256
# out-CSR entries per backward work item, its work is data-dependent (CSRGraph(chunk_bwd=...);
# None = by graph size). Measured with the dense pull (scripts/bwd_bench.py, per call): S0
# (24 041 nodes) F = 256: 68.0 / 66.0 / 72.1 / 101.6 us at 64 / 128 / 256 / 512 (hub
# sources serialise on one wave past 128); RMAT x16 (384 656 nodes) F = 512 bf16: 1504 /
# 1375 / 1308 / 1275 us: finer items pay off only while the graph alone does not fill the
# chip.
DEFAULT_CHUNK_BWD = None


CHUNK_BWD_OVERRIDE: Optional[int] = None  # tuning experiments (bench.py --chunk-bwd)
# graphs from this many edges (self-loops included) get transposed max-backward descriptors
TRANS_MIN_EDGES = 1 << 22
# sampled blocks (dgl.dataloading) build their transpose and schedules on the HIP device they
# were sampled on; False keeps the host build (CSRGraph.from_in_csr + upload) for A/B runs
DEVICE_BUILD = True


def default_chunk_bwd(num_nodes: int) -> int:
    if CHUNK_BWD_OVERRIDE:
        return CHUNK_BWD_OVERRIDE
    return 64 if num_nodes <= 65536 else 512


def _square_nodes(num_src: int, num_dst: int) -> int:
    """num_nodes of a square graph; a rectangular one has num_src and num_dst instead."""
    if num_src != num_dst:
        raise ValueError(f"num_nodes of a rectangular graph ({num_src} sources, {num_dst} destinations): "
                         "use num_src / num_dst")
    return num_dst


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _schedule(ptr: np.ndarray, chunk: int):
    n_rows = len(ptr) - 1
    n_items = ctypes.c_int64()
    n_merges = ctypes.c_int64()
    n_slots = ctypes.c_int64()
    max_deg = ctypes.c_int32()
    call("pg_schedule_count", _np_ptr(ptr), n_rows, chunk, ctypes.byref(n_items),
         ctypes.byref(n_merges), ctypes.byref(n_slots), ctypes.byref(max_deg))
    items = np.zeros(max(1, n_items.value) * 4, np.int32)
    merges = np.zeros(max(1, n_merges.value) * 4, np.int32)
    call("pg_schedule_build", _np_ptr(ptr), n_rows, chunk, _np_ptr(items), _np_ptr(merges))
    return items, n_items.value, merges, n_merges.value, n_slots.value, max_deg.value


class HostCsr:
    """One CSR direction with its schedule, in host memory (numpy int32)."""

    def __init__(self, ptr, col, eslot, n_cols: int, chunk: int, epos=None):
        self.ptr, self.col, self.eslot, self.epos = ptr, col, eslot, epos
        self.n_rows = len(ptr) - 1
        self.n_cols = int(n_cols)
        self.nnz = int(len(col))
        self.chunk = int(chunk)
        (self.items, self.n_items, self.merges, self.n_merges, self.n_slots,
         self.max_deg) = _schedule(ptr, chunk)


class DeviceCsr:
    """A HostCsr uploaded to one device; ``struct()`` gives the pg_csr_t view."""

    def __init__(self, h: HostCsr, device: torch.device):
        def up(a):
            return None if a is None else torch.from_numpy(a).to(device)

        self.device = device
        self.ptr, self.col, self.eslot, self.epos = up(h.ptr), up(h.col), up(h.eslot), up(h.epos)

        self.items, self.merges = up(h.items), up(h.merges)
        self.n_rows, self.n_cols, self.nnz = h.n_rows, h.n_cols, h.nnz
        self.n_items, self.n_merges, self.n_slots = h.n_items, h.n_merges, h.n_slots
        self.max_deg, self.chunk = h.max_deg, h.chunk

    @classmethod
    def from_tensors(cls, device: torch.device, ptr, col, eslot, epos, items, merges, n_cols: int, n_items: int,
                     n_merges: int, n_slots: int, max_deg: int, chunk: int) -> "DeviceCsr":
        """The same object from tensors that already live on `device` (int32; eslot / epos may
        be None), with the counts the schedule was built with."""
        c = cls.__new__(cls)
        c.device = device
        c.ptr, c.col, c.eslot, c.epos, c.items, c.merges = ptr, col, eslot, epos, items, merges
        c.n_rows, c.n_cols, c.nnz = int(ptr.numel()) - 1, int(n_cols), int(col.numel())
        c.n_items, c.n_merges, c.n_slots = int(n_items), int(n_merges), int(n_slots)
        c.max_deg, c.chunk = int(max_deg), int(chunk)
        return c

    def struct(self, ew: Optional[torch.Tensor] = None) -> PgCsr:
        """The pg_csr_t view (cached per edge-weight pointer: it holds raw pointers only)."""
        key = _lib.ptr(ew)
        cache = self.__dict__.setdefault("_structs", {})
        s = cache.get(key)
        if s is None:
            s = cache[key] = self._make_struct(ew)
        return s

    def _make_struct(self, ew: Optional[torch.Tensor]) -> PgCsr:
        s = PgCsr()
        s.n_rows, s.n_cols, s.nnz = self.n_rows, self.n_cols, self.nnz
        s.ptr = _lib.ptr(self.ptr)
        s.col = _lib.ptr(self.col)
        s.eslot = _lib.ptr(self.eslot)
        s.epos = _lib.ptr(self.epos)
        s.ew = _lib.ptr(ew)
        s.items = _lib.ptr(self.items)
        s.n_items = self.n_items
        s.merges = _lib.ptr(self.merges) if self.n_merges > 0 else 0
        s.n_merges = self.n_merges
        s.n_slots = self.n_slots
        s.max_deg = self.max_deg
        s.chunk = self.chunk
        return s


class CSRGraph:
    """In-CSR + out-CSR of a directed graph given as COO (src -> dst), host resident. Square
    (``CSRGraph(src, dst, num_nodes)``: sources and destinations are one node set) or
    rectangular (``CSRGraph.from_in_csr``: a bipartite block of num_src sources and num_dst
    destinations)."""

    def __init__(self, src, dst, num_nodes: int, chunk: int = DEFAULT_CHUNK,
                 chunk_bwd: Optional[int] = DEFAULT_CHUNK_BWD, bwd_trans: Optional[bool] = None):
        src = np.ascontiguousarray(np.asarray(src, dtype=np.int64))
        dst = np.ascontiguousarray(np.asarray(dst, dtype=np.int64))
        if src.shape != dst.shape or src.ndim != 1:
            raise ValueError("src and dst must be 1-D arrays of equal length")
        n = int(num_nodes)
        E = len(src)
        ptr = np.zeros(n + 1, np.int32)
        col = np.zeros(max(E, 1), np.int32)
        eid = np.zeros(max(E, 1), np.int32)
        call("pg_csr_from_coo", _np_ptr(src), _np_ptr(dst), E, n, n, _np_ptr(ptr), _np_ptr(col),
             _np_ptr(eid))
        self._finish(ptr, col[:E], eid[:E], n, n, chunk, chunk_bwd, bwd_trans)

    @classmethod
    def from_coo_rect(cls, src, dst, num_src: int, num_dst: int, chunk: int = DEFAULT_CHUNK,
                      chunk_bwd: Optional[int] = DEFAULT_CHUNK_BWD) -> "CSRGraph":
        """A rectangular graph from COO (src in [0, num_src), dst in [0, num_dst)): the stable
        sort of pg_csr_from_coo, as the square constructor (dgl.create_block)."""
        src = np.ascontiguousarray(np.asarray(src, dtype=np.int64))
        dst = np.ascontiguousarray(np.asarray(dst, dtype=np.int64))
        if src.shape != dst.shape or src.ndim != 1:
            raise ValueError("src and dst must be 1-D arrays of equal length")
        E = len(src)
        ptr = np.zeros(int(num_dst) + 1, np.int32)
        col = np.zeros(max(E, 1), np.int32)
        eid = np.zeros(max(E, 1), np.int32)
        call("pg_csr_from_coo", _np_ptr(src), _np_ptr(dst), E, int(num_src), int(num_dst), _np_ptr(ptr),
             _np_ptr(col), _np_ptr(eid))
        g = cls.__new__(cls)
        g._finish(ptr, col[:E], eid[:E], int(num_src), int(num_dst), chunk, chunk_bwd, False)
        return g

    @classmethod
    def from_in_csr(cls, ptr, col, num_src: int, chunk: int = DEFAULT_CHUNK,
                    chunk_bwd: Optional[int] = DEFAULT_CHUNK_BWD) -> "CSRGraph":
        """A graph from a finished in-CSR (rows = the len(ptr) - 1 destinations, col = source ids
        below num_src, every row in the order its entries are to be reduced in): edge id = slot,
        no COO sort. The transpose and both schedules come from the same host calls as the
        square constructor's. A sampled block is built this way."""
        ptr = np.ascontiguousarray(np.asarray(ptr, dtype=np.int32))
        col = np.ascontiguousarray(np.asarray(col, dtype=np.int32))
        if ptr.ndim != 1 or col.ndim != 1 or len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != len(col):
            raise ValueError("from_in_csr: ptr must start at 0 and end at len(col)")
        if len(ptr) > 1 and (np.diff(ptr) < 0).any():
            raise ValueError("from_in_csr: ptr is not monotone")
        g = cls.__new__(cls)
        g._finish(ptr, col, np.arange(len(col), dtype=np.int32), int(num_src), len(ptr) - 1, chunk, chunk_bwd,
                  False)
        return g

    def _finish(self, ptr, col, eid, num_src: int, num_dst: int, chunk, chunk_bwd, bwd_trans):
        E = len(col)
        tptr = np.zeros(num_src + 1, np.int32)
        tcol = np.zeros(max(E, 1), np.int32)
        tslot = np.zeros(max(E, 1), np.int32)
        tpos = np.zeros(max(E, 1), np.int32)
        colp = col if E > 0 else np.zeros(1, np.int32)
        call("pg_csr_transpose", _np_ptr(ptr), _np_ptr(colp), num_dst, num_src, E, _np_ptr(tptr), _np_ptr(tcol),
             _np_ptr(tslot), _np_ptr(tpos))
        self.num_src, self.num_dst = num_src, num_dst
        self.num_edges = E
        self.eid = eid  # in-CSR slot -> edge id
        # the in-CSR slots' transposed indices (pg_csr_t.epos of the in-CSR): with them the
        # max backward stores each live edge's list descriptor where the pull reads it in
        # order (coalesced) instead of at the slot (one random read per edge), at the price
        # of clearing the descriptor array and scattered descriptor stores. Measured per step:
        # RMAT x16 (19.6 M edges) 3.28 -> 2.90 ms, S0 (1.23 M edges, its descriptors stay in
        # the caches) 0.232 -> 0.238 ms: on by default from TRANS_MIN_EDGES edges
        if bwd_trans is None:
            bwd_trans = E >= TRANS_MIN_EDGES
        einv = None
        if bwd_trans and E > 0:
            einv = np.empty(E, np.int32)
            einv[tslot[:E]] = np.arange(E, dtype=np.int32)
        self.bwd_trans = einv is not None
        self.fwd = HostCsr(ptr, col, None, num_src, chunk, epos=einv)
        if chunk_bwd is None:
            chunk_bwd = default_chunk_bwd(max(num_src, num_dst))
        self.bwd = HostCsr(tptr, tcol[:E], tslot[:E], num_dst, chunk_bwd, epos=tpos[:E])
        # argmax records hold positions inside in-CSR rows: u16 while every row is shorter
        # than 0xFFFF entries (0xFFFF = no winner)
        self.arg_kind = _lib.PG_ARG_U16 if self.fwd.max_deg < 0xFFFF else _lib.PG_ARG_I32
        self._dev: Dict[str, "DeviceGraph"] = {}

    @property
    def num_nodes(self) -> int:
        return _square_nodes(self.num_src, self.num_dst)

    def on(self, device) -> "DeviceGraph":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = str(device)
        if key not in self._dev:
            self._dev[key] = DeviceGraph(self, device)
        return self._dev[key]

    def in_degrees(self) -> np.ndarray:
        return np.diff(self.fwd.ptr)

    def out_degrees(self) -> np.ndarray:
        return np.diff(self.bwd.ptr)

    def has_zero_in_degree(self) -> bool:
        return bool((self.in_degrees() == 0).any())


def _dev_ws(nbytes: int, device) -> torch.Tensor:
    from .ops import _workspace  # deferred: ops imports this module

    return _workspace(max(int(nbytes), 256), device)


def _schedule_count_dev(ptr: torch.Tensor, chunk: int) -> torch.Tensor:
    """int64[6] on ptr's device (pg_schedule_count_dev): n_items, n_merges, n_slots, max_deg,
    min_deg, status. Nothing is read back here."""
    n_rows = ptr.numel() - 1
    counts = torch.empty(6, dtype=torch.int64, device=ptr.device)
    ws_n = _lib.lib().pg_schedule_count_dev_workspace(n_rows)
    ws = _dev_ws(ws_n, ptr.device)
    call("pg_schedule_count_dev", _lib.ptr(ptr), n_rows, chunk, _lib.ptr(counts), _lib.ptr(ws), ws.numel(),
         _lib.stream_handle(ptr.device))
    return counts


def _schedule_build_dev(ptr: torch.Tensor, chunk: int, n_items: int, n_merges: int, max_deg: int):
    """(items, merges) on ptr's device (pg_schedule_build_dev), sized as HostCsr's."""
    n_rows = ptr.numel() - 1
    items = torch.zeros(max(1, n_items) * 4, dtype=torch.int32, device=ptr.device)
    merges = torch.zeros(max(1, n_merges) * 4, dtype=torch.int32, device=ptr.device)
    ws_n = _lib.lib().pg_schedule_build_dev_workspace(n_rows, n_items, n_merges)
    ws = _dev_ws(ws_n, ptr.device)
    call("pg_schedule_build_dev", _lib.ptr(ptr), n_rows, chunk, n_items, n_merges, max_deg, _lib.ptr(items),
         _lib.ptr(merges), _lib.ptr(ws), ws.numel(), _lib.stream_handle(ptr.device))
    return items, merges


def _transpose_dev(ptr: torch.Tensor, col: torch.Tensor, n_cols: int):
    """(tptr, tcol, tslot, tpos, status) on ptr's device (pg_csr_transpose_dev)."""
    dev = ptr.device
    n_rows, nnz = ptr.numel() - 1, col.numel()
    tptr = torch.empty(n_cols + 1, dtype=torch.int32, device=dev)
    tcol, tslot, tpos = (torch.empty(nnz, dtype=torch.int32, device=dev) for _ in range(3))
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws_n = _lib.lib().pg_csr_transpose_dev_workspace(n_rows, n_cols, nnz)
    ws = _dev_ws(ws_n, dev)
    call("pg_csr_transpose_dev", _lib.ptr(ptr), _lib.ptr(col), n_rows, n_cols, nnz, _lib.ptr(tptr), _lib.ptr(tcol),
         _lib.ptr(tslot), _lib.ptr(tpos), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    return tptr, tcol, tslot, tpos, status


class DeviceGraph:
    def __init__(self, g: CSRGraph, device: torch.device):
        self.device = device
        self.num_src, self.num_dst = g.num_src, g.num_dst
        self.num_edges = g.num_edges
        self.arg_kind = g.arg_kind
        self.arg_dtype = torch.int16 if g.arg_kind == _lib.PG_ARG_U16 else torch.int32
        self.fwd = DeviceCsr(g.fwd, device)
        self.bwd = DeviceCsr(g.bwd, device)
        self.eid = torch.from_numpy(g.eid.astype(np.int64)).to(device)

    @classmethod
    def from_in_csr(cls, ptr: torch.Tensor, col: torch.Tensor, num_src: int, chunk: int = DEFAULT_CHUNK,
                    chunk_bwd: Optional[int] = DEFAULT_CHUNK_BWD) -> "DeviceGraph":
        """CSRGraph.from_in_csr(ptr, col, num_src).on(device) for an in-CSR that lives on a device
        (int32 tensors): on a HIP device the transpose and both schedules are built there by
        the device twins of the host calls, with one read-back (both directions' counts and the
        status) and no copy of an index array; edge id = slot. ValueError for a column outside
        [0, num_src) or a ptr that is not monotone from 0 to len(col)."""
        if ptr.dtype != torch.int32 or col.dtype != torch.int32 or ptr.dim() != 1 or col.dim() != 1 \
                or ptr.numel() < 1 or ptr.device != col.device:
            raise TypeError("from_in_csr: ptr and col must be 1-D int32 tensors on one device")
        dev, num_src = ptr.device, int(num_src)
        if dev.type != "cuda":
            return CSRGraph.from_in_csr(ptr.numpy(), col.numpy(), num_src, chunk, chunk_bwd).on("cpu")
        ptr, col = ptr.contiguous(), col.contiguous()
        num_dst, E = ptr.numel() - 1, col.numel()
        if num_src < 0:
            raise ValueError("from_in_csr: negative num_src")
        if chunk_bwd is None:
            chunk_bwd = default_chunk_bwd(max(num_src, num_dst))
        cf = _schedule_count_dev(ptr, chunk)
        tptr, tcol, tslot, tpos, status = _transpose_dev(ptr, col, num_src)
        cb = _schedule_count_dev(tptr, chunk_bwd)
        back = torch.cat([cf, cb, status.to(torch.int64)]).tolist()  # the one read-back
        (fi, fm, fs, fmax, fmin, fst), (bi, bm, bs, bmax, _, bst), st = back[:6], back[6:12], back[12]
        if st or fst or bst:
            raise ValueError("from_in_csr: " + ("a column lies outside [0, num_src)" if st == -2 else
                                                "ptr must start at 0, end at len(col) and be monotone"
                                                if st or fst == -1 else "the schedule exceeds int32"))
        fitems, fmerges = _schedule_build_dev(ptr, chunk, fi, fm, fmax)
        bitems, bmerges = _schedule_build_dev(tptr, chunk_bwd, bi, bm, bmax)
        g = cls.__new__(cls)
        g.device = dev
        g.num_src, g.num_dst, g.num_edges = num_src, num_dst, E
        g.arg_kind = _lib.PG_ARG_U16 if fmax < 0xFFFF else _lib.PG_ARG_I32
        g.arg_dtype = torch.int16 if g.arg_kind == _lib.PG_ARG_U16 else torch.int32
        g.fwd = DeviceCsr.from_tensors(dev, ptr, col, None, None, fitems, fmerges, num_src, fi, fm, fs, fmax, chunk)
        g.bwd = DeviceCsr.from_tensors(dev, tptr, tcol, tslot, tpos, bitems, bmerges, num_dst, bi, bm, bs, bmax,
                                       chunk_bwd)
        g.eid = torch.arange(E, dtype=torch.int64, device=dev)
        g.min_in_degree = fmin
        return g

    @property
    def num_nodes(self) -> int:
        return _square_nodes(self.num_src, self.num_dst)

    def in_degrees(self) -> torch.Tensor:
        """int32 in-degrees on the device (the differences of the in-CSR's ptr), computed once."""
        if "_in_degrees" not in self.__dict__:
            self._in_degrees = self.fwd.ptr.diff()
        return self._in_degrees

    def out_degrees(self) -> torch.Tensor:
        if "_out_degrees" not in self.__dict__:
            self._out_degrees = self.bwd.ptr.diff()
        return self._out_degrees

    @property
    def is_cuda(self) -> bool:
        return self.device.type == "cuda"

    def edge_map(self, transpose: bool = False) -> torch.Tensor:
        """int32 edge id of every entry of the in-CSR (transpose: of the out-CSR, eid[eslot]):
        pg_gspmm / pg_gsddmm's `eidx`, with which edge tensors are read and written in edge-id
        order. Built once per device graph."""
        maps = self.__dict__.setdefault("_edge_maps", {})
        if transpose not in maps:
            eid = self.eid.to(torch.int32)
            maps[transpose] = eid[self.bwd.eslot.long()].contiguous() if transpose else eid.contiguous()
        return maps[transpose]

    def exclusion_bits(self) -> torch.Tensor:
        """The graph's exclusion bit set (ops.sample_neighbors(exclude=)): int32 words on the device,
        bit e & 31 of word e >> 5 for edge id e, allocated zeroed on first use. A batch sets its
        ids (ops.edge_bits_update), samples, and clears the same ids: between batches it is zero."""
        if "_exclusion_bits" not in self.__dict__:
            self._exclusion_bits = torch.zeros(max(1, (self.num_edges + 31) // 32), dtype=torch.int32,
                                               device=self.device)
        return self._exclusion_bits

    def edge_weight_slots(self, edge_weight: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Edge weights given per edge id (DGL order) -> in-CSR slot order, f32 contiguous:
        one weight per edge as a 1-D tensor, H > 1 weights per edge ((E, H, ...)) as (E, H)."""
        if edge_weight is None:
            return None
        if edge_weight.dim() >= 2 and edge_weight.shape[0] == self.num_edges \
                and edge_weight.numel() != self.num_edges:
            w = edge_weight.reshape(self.num_edges, -1)
            return w.to(device=self.device, dtype=torch.float32).index_select(0, self.eid).contiguous()
        w = edge_weight.reshape(-1)
        if w.numel() != self.num_edges:
            raise ValueError(f"edge_weight has {w.numel()} entries, graph has {self.num_edges} edges")
        return w.to(device=self.device, dtype=torch.float32).index_select(0, self.eid).contiguous()


class DeviceBuiltGraph:
    """Owner of a block whose engine graph was built on the device (DeviceGraph.from_in_csr): what
    the dgl shim asks of a CSRGraph, answered without host arrays where it can be. `.on(its own
    device)` is the device-built graph and `has_zero_in_degree()` comes from the count's minimum;
    anything that needs host arrays (another device, in_degrees() / out_degrees() as numpy,
    .fwd / .bwd / .eid) downloads ptr and col once and builds a CSRGraph.from_in_csr, kept in
    `host` (None until then)."""

    def __init__(self, ptr: torch.Tensor, col: torch.Tensor, num_src: int, chunk: int = DEFAULT_CHUNK,
                 chunk_bwd: Optional[int] = DEFAULT_CHUNK_BWD):
        self._chunk, self._chunk_bwd = chunk, chunk_bwd
        self.device_graph = DeviceGraph.from_in_csr(ptr, col, num_src, chunk, chunk_bwd)
        self.device = self.device_graph.device
        self.num_src, self.num_dst = self.device_graph.num_src, self.device_graph.num_dst
        self.num_edges = self.device_graph.num_edges
        self.arg_kind = self.device_graph.arg_kind
        self.host: Optional[CSRGraph] = None

    def host_graph(self) -> CSRGraph:
        if self.host is None:
            f = self.device_graph.fwd
            self.host = CSRGraph.from_in_csr(f.ptr.cpu().numpy(), f.col.cpu().numpy(), self.num_src, self._chunk,
                                             self._chunk_bwd)
        return self.host

    @property
    def num_nodes(self) -> int:
        return _square_nodes(self.num_src, self.num_dst)

    def on(self, device) -> DeviceGraph:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self.device_graph
        return self.host_graph().on(device)

    def has_zero_in_degree(self) -> bool:
        return self.num_dst > 0 and self.device_graph.min_in_degree == 0

    def in_degrees(self) -> np.ndarray:
        return self.host_graph().in_degrees()

    def out_degrees(self) -> np.ndarray:
        return self.host_graph().out_degrees()

    @property
    def fwd(self) -> HostCsr:
        return self.host_graph().fwd

    @property
    def bwd(self) -> HostCsr:
        return self.host_graph().bwd

    @property
    def eid(self) -> np.ndarray:
        return self.host_graph().eid
