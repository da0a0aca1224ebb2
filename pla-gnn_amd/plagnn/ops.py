"""Tensor-level operations over the C-ABI, and their autograd wrappers.

Every GPU operation here is a call into libplagnn.so on torch's current stream; there is
no fallback to another implementation. Tensors on the CPU device (the reference's
``-d cpu``, code/main_normal.py:30) go to the library's ``*_cpu`` entry points for the
message passing and to torch-CPU for the dense algebra, as DGL's CPU backend does.
"""
from __future__ import annotations

import weakref
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import call, ptr
from .graph import DeviceGraph

LEAKY_SLOPE = 0.01  # F.leaky_relu default (code/model.py:21-27)


def round4(n: int) -> int:
    return (n + 3) // 4 * 4


def _ld(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a row-major 2-D tensor with unit column stride")
    return t.stride(0)


def _stream(t: torch.Tensor):
    return _lib.stream_handle(t.device)


_scratch = {}


def _workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Library scratch for one call: one buffer per (device, stream), grown on demand and
    reused by every later call on that stream (stream order makes the reuse safe), so the
    drop-in path's autograd functions allocate nothing per call. During HIP-graph capture a
    call gets a fresh buffer from the graph's private pool instead: a cached buffer would
    be shared between the graph's replays and eager calls that can run beside them."""
    if nbytes <= 0:
        return None
    device = torch.device(device)
    if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
        return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


def _check_device(dg: DeviceGraph, *ts):
    for t in ts:
        if t is not None and t.device != dg.device:
            raise ValueError(f"tensor on {t.device}, graph on {dg.device}")
        if t is not None and t.dtype not in (torch.float32, torch.bfloat16, torch.int16, torch.int32,
                                             torch.int64):
            raise TypeError(f"unsupported dtype {t.dtype}")


# ------------------------------------------------------------------ message passing
def spmm_max(dg: DeviceGraph, X: torch.Tensor, ew_slots: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, argpos: Optional[torch.Tensor] = None,
             dead_none: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """out[v] = max over in-edges of X[u] (* w), argpos = winning in-row position.
    DGL update_all(copy_u|u_mul_e, max) (code/model.py:20,22,24). `dead_none`
    (PG_ARG_DEAD_NONE, GPU): a zero maximum records no winner."""
    if X.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("spmm_max: float32 or bfloat16 features expected")
    bf = X.dtype == torch.bfloat16
    _check_device(dg, X, ew_slots)
    n, F = dg.num_dst, X.shape[1]
    if X.shape[0] != dg.num_src:
        raise ValueError(f"spmm_max: X has {X.shape[0]} rows, graph has {dg.num_src} source nodes")
    if out is None:
        out = torch.empty(n, F, dtype=X.dtype, device=X.device)
    if argpos is None:
        argpos = torch.empty(n, F, dtype=dg.arg_dtype, device=X.device)
    g = dg.fwd.struct(ew_slots)
    if bf and not dg.is_cuda:
        raise TypeError("spmm_max: bfloat16 storage runs on the GPU only")
    if dg.is_cuda:
        ws_n = _lib.lib().pg_spmm_max_fwd_workspace(g, F, dg.arg_kind)
        ws = _workspace(ws_n, X.device)
        kind = dg.arg_kind | (_lib.PG_ARG_DEAD_NONE if dead_none else 0)
        call("pg_spmm_max_fwd_bf16" if bf else "pg_spmm_max_fwd", g, ptr(X), _ld(X), F, ptr(out), _ld(out), ptr(argpos), _ld(argpos),
             kind, ptr(ws), ws_n, _stream(X))
    else:
        call("pg_spmm_max_fwd_cpu", g, ptr(X), _ld(X), F, ptr(out), _ld(out), ptr(argpos),
             _ld(argpos), dg.arg_kind)
    return out, argpos


def spmm_max_backward(dg: DeviceGraph, argpos: torch.Tensor, dout: torch.Tensor,
                      ew_slots: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                      dx: Optional[torch.Tensor] = None, fwd_out: Optional[torch.Tensor] = None,
                      dead_none: bool = False) -> torch.Tensor:
    """dX of the max aggregation (DGL GSpMM.backward: scatter_add_ through argX),
    gathered per source in ascending destination order; optional fused relu' mask
    (mask[u,f] > 0). With `fwd_out` (the forward's output; needs mask = the forward's
    input) entries whose maximum is 0 are skipped: they contribute nothing (the mask is
    still applied). `dead_none`: the records come from spmm_max(..., dead_none=True) (the
    same skip made by the forward; needs mask = a relu output >= 0, which is then implied
    and not read)."""
    _check_device(dg, argpos, dout, ew_slots, mask)
    bf = dout.dtype == torch.bfloat16
    if bf and ((mask is not None and mask.dtype != torch.bfloat16) or not dg.is_cuda):
        raise TypeError("spmm_max_backward: bfloat16 storage (GPU) needs a bfloat16 mask")
    n, F = dg.num_src, dout.shape[1]
    if dx is None:
        dx = torch.empty(n, F, dtype=dout.dtype, device=dout.device)
    g = dg.fwd.struct(ew_slots)
    gt = dg.bwd.struct(None)
    ldm = _ld(mask) if mask is not None else 0
    if dg.is_cuda:
        ws_n = _lib.lib().pg_spmm_max_bwd_workspace(gt, F)
        ws = _workspace(ws_n, dout.device)
        ldf = _ld(fwd_out) if fwd_out is not None else 0
        kind = dg.arg_kind | (_lib.PG_ARG_DEAD_NONE if dead_none else 0)
        call("pg_spmm_max_bwd_bf16" if bf else "pg_spmm_max_bwd", g, gt, ptr(argpos), _ld(argpos), kind, ptr(dout), _ld(dout),
             F, ptr(mask), ldm, ptr(fwd_out), ldf, ptr(dx), _ld(dx), ptr(ws), ws_n, _stream(dout))
    else:
        call("pg_spmm_max_bwd_cpu", g, gt, ptr(argpos), _ld(argpos), dg.arg_kind, ptr(dout),
             _ld(dout), F, ptr(mask), ldm, ptr(dx), _ld(dx))
    return dx


def spmm_max_backward_scatter(dg: DeviceGraph, argpos: torch.Tensor, dout: torch.Tensor,
                              ew_slots: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DGL-form backward with float atomics (non-deterministic summation order)."""
    if not dg.is_cuda:
        raise ValueError("scatter backward is a GPU-only entry point")
    F = dout.shape[1]
    dx = torch.empty(dg.num_src, F, dtype=torch.float32, device=dout.device)
    call("pg_spmm_max_bwd_scatter", dg.fwd.struct(ew_slots), ptr(argpos), _ld(argpos), dg.arg_kind,
         ptr(dout), _ld(dout), F, ptr(dx), _ld(dx), dg.num_src, _stream(dout))
    return dx


def spmm_sum(dg: DeviceGraph, X: torch.Tensor, mean: bool = False,
             ew_slots: Optional[torch.Tensor] = None, transpose: bool = False,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sum/mean aggregation (copy_u|u_mul_e, sum|mean). With transpose=True it runs on the
    out-CSR: the backward of the forward aggregation (mean -> per-term 1/deg(dst))."""
    _check_device(dg, X, ew_slots)
    F = X.shape[1]
    n_out, n_in = (dg.num_src, dg.num_dst) if transpose else (dg.num_dst, dg.num_src)
    if X.shape[0] != n_in:
        raise ValueError(f"spmm_sum: X has {X.shape[0]} rows, {n_in} expected")
    if out is None:
        out = torch.empty(n_out, F, dtype=torch.float32, device=X.device)
    csr = dg.bwd if transpose else dg.fwd
    g = csr.struct(ew_slots)
    norm_mode = (2 if transpose else 1) if mean else 0
    norm_ptr = dg.fwd.ptr if (mean and transpose) else None
    if dg.is_cuda:
        ws_n = _lib.lib().pg_spmm_sum_workspace(g, F)
        ws = _workspace(ws_n, X.device)
        call("pg_spmm_sum", g, ptr(X), _ld(X), F, norm_mode, ptr(norm_ptr), ptr(out), _ld(out),
             ptr(ws), ws_n, _stream(X))
    else:
        call("pg_spmm_sum_cpu", g, ptr(X), _ld(X), F, norm_mode, ptr(norm_ptr), ptr(out), _ld(out))
    return out


def sddmm_dot(dg: DeviceGraph, D: torch.Tensor, X: torch.Tensor, mean: bool = False,
              argpos: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-edge dot products de[k] = sum_f D[dst_k, f] * X[src_k, f] in in-CSR slot order
    (pg_sddmm_dot): the gradient of a sum (`mean`: mean) aggregation w.r.t. its u_mul_e
    weights, with D = dout. With `argpos` (a max aggregation's records, plain or dead-none)
    only the features edge k won are summed: the max aggregation's weight gradient."""
    _check_device(dg, D, X, argpos)
    if D.dtype != torch.float32 or X.dtype != torch.float32:
        raise TypeError("sddmm_dot: float32 operands expected")
    n, F = dg.num_dst, D.shape[1]
    if D.shape[0] != n or tuple(X.shape) != (dg.num_src, F):
        raise ValueError(f"sddmm_dot: operands {tuple(D.shape)}, {tuple(X.shape)} on a graph of {dg.num_src} "
                         f"source and {n} destination nodes")
    if argpos is not None and (argpos.dtype != dg.arg_dtype or tuple(argpos.shape) != (n, F)):
        raise ValueError("sddmm_dot: argpos does not match the graph's record type or the operands' shape")
    de = torch.empty(dg.num_edges, dtype=torch.float32, device=D.device)
    g = dg.fwd.struct(None)
    lda = _ld(argpos) if argpos is not None else 0
    args = (g, ptr(D), _ld(D), ptr(X), _ld(X), F, int(mean), ptr(argpos), lda, dg.arg_kind, ptr(de))
    if dg.is_cuda:
        call("pg_sddmm_dot", *args, _stream(D))
    else:
        call("pg_sddmm_dot_cpu", *args)
    return de


def _edge_heads(dg: DeviceGraph, name: str, *ts: torch.Tensor) -> int:
    """The head count of (E, H) float32 edge tensors in slot order (one count for all)."""
    H = ts[0].shape[1] if ts[0].dim() == 2 else -1
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: float32 edge features expected")
        if t.dim() != 2 or t.shape[0] != dg.num_edges or t.shape[1] != H:
            raise ValueError(f"{name}: edge features {tuple(t.shape)} on a graph of {dg.num_edges} edges, "
                             f"({dg.num_edges}, {H}) expected")
    return H


def edge_softmax(dg: DeviceGraph, scores: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Softmax of the (E, H) scores over the in-edges of each destination, per head, in
    in-CSR slot order (pg_edge_softmax_fwd; dgl.ops.edge_softmax with norm_by='dst')."""
    _check_device(dg, scores, out)
    if out is None:
        out = torch.empty(tuple(scores.shape), dtype=torch.float32, device=scores.device)
    H = _edge_heads(dg, "edge_softmax", scores, out)
    args = (dg.fwd.struct(None), ptr(scores), _ld(scores), H, ptr(out), _ld(out))
    if dg.is_cuda:
        call("pg_edge_softmax_fwd", *args, _stream(scores))
    else:
        call("pg_edge_softmax_fwd_cpu", *args)
    return out


def edge_softmax_backward(dg: DeviceGraph, a: torch.Tensor, da: torch.Tensor,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ds = a * (da - sum over the row of a * da) for a = edge_softmax(s) (pg_edge_softmax_bwd)."""
    _check_device(dg, a, da, out)
    if out is None:
        out = torch.empty(tuple(a.shape), dtype=torch.float32, device=a.device)
    H = _edge_heads(dg, "edge_softmax_backward", a, da, out)
    args = (dg.fwd.struct(None), ptr(a), _ld(a), ptr(da), _ld(da), H, ptr(out), _ld(out))
    if dg.is_cuda:
        call("pg_edge_softmax_bwd", *args, _stream(a))
    else:
        call("pg_edge_softmax_bwd_cpu", *args)
    return out


def _head_width(name: str, X: torch.Tensor, n: int, H: int) -> int:
    if X.dtype != torch.float32:
        raise TypeError(f"{name}: float32 features expected")
    if X.dim() != 2 or X.shape[0] != n or H < 1 or X.shape[1] % H != 0 or X.shape[1] == 0:
        raise ValueError(f"{name}: features {tuple(X.shape)} do not split into {H} heads on {n} nodes")
    return X.shape[1] // H


def spmm_sum_heads(dg: DeviceGraph, A: torch.Tensor, X: torch.Tensor, H: int, transpose: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[v, h*Fh + j] = sum over in-edges k of A[k, h] * X[src_k, h*Fh + j] with (E, H)
    weights in slot order (pg_spmm_sum_heads; update_all(u_mul_e, sum) on (N, H, Fh) features).
    transpose=True runs on the out-CSR: the feature gradient of the forward aggregation."""
    _check_device(dg, A, X, out)
    if _edge_heads(dg, "spmm_sum_heads", A) != H:
        raise ValueError(f"spmm_sum_heads: weights {tuple(A.shape)} for {H} heads")
    n_out, n_in = (dg.num_src, dg.num_dst) if transpose else (dg.num_dst, dg.num_src)
    Fh = _head_width("spmm_sum_heads", X, n_in, H)
    if out is None:
        out = torch.empty(n_out, H * Fh, dtype=torch.float32, device=X.device)
    g = (dg.bwd if transpose else dg.fwd).struct(None)
    args = (g, ptr(A), _ld(A), H, ptr(X), _ld(X), Fh, ptr(out), _ld(out))
    if dg.is_cuda:
        ws_n = _lib.lib().pg_spmm_sum_workspace(g, H * Fh)
        ws = _workspace(ws_n, X.device)
        call("pg_spmm_sum_heads", *args, ptr(ws), ws_n, _stream(X))
    else:
        call("pg_spmm_sum_heads_cpu", *args)
    return out


def sddmm_dot_heads(dg: DeviceGraph, D: torch.Tensor, X: torch.Tensor, H: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-edge, per-head dot products de[k, h] = sum_j D[dst_k, h*Fh + j] * X[src_k, h*Fh + j],
    (E, H) in slot order (pg_sddmm_dot_heads): the gradient of spmm_sum_heads w.r.t. its
    weights (D = dout), and apply_edges(u_dot_v) on (N, H, Fh) operands."""
    _check_device(dg, D, X, out)
    Fh = _head_width("sddmm_dot_heads", D, dg.num_dst, H)
    if tuple(X.shape) != (dg.num_src, D.shape[1]) or X.dtype != torch.float32:
        raise ValueError(f"sddmm_dot_heads: operands {tuple(D.shape)}, {tuple(X.shape)}")
    de = torch.empty(dg.num_edges, H, dtype=torch.float32, device=D.device) if out is None else out
    if _edge_heads(dg, "sddmm_dot_heads", de) != H:
        raise ValueError(f"sddmm_dot_heads: output {tuple(de.shape)} for {H} heads")
    args = (dg.fwd.struct(None), ptr(D), _ld(D), ptr(X), _ld(X), H, Fh, ptr(de), max(_ld(de), H))
    if dg.is_cuda:
        call("pg_sddmm_dot_heads", *args, _stream(D))
    else:
        call("pg_sddmm_dot_heads_cpu", *args)
    return de


def _gatv2_args(dg: DeviceGraph, name: str, xl: torch.Tensor, xr: torch.Tensor, attn: torch.Tensor, H: int) -> int:
    """Checked operands of the GATv2 score calls: (N, H*Fh) projections and H*Fh attention
    weights, float32 and contiguous; returns Fh."""
    _check_device(dg, xl, xr, attn)
    Fh = _head_width(name, xl, dg.num_src, H)
    if tuple(xr.shape) != (dg.num_dst, xl.shape[1]) or xr.dtype != torch.float32:
        raise ValueError(f"{name}: operands {tuple(xl.shape)}, {tuple(xr.shape)}")
    if attn.dtype != torch.float32 or attn.numel() != H * Fh or not attn.is_contiguous():
        raise ValueError(f"{name}: attn {tuple(attn.shape)} for {H} heads of {Fh}")
    return Fh


def gatv2_score(dg: DeviceGraph, xl: torch.Tensor, xr: torch.Tensor, attn: torch.Tensor, H: int,
                slope: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GATv2 attention scores s[k, h] = sum_d attn[h, d] * leaky_relu(xl[src_k, h, d] +
    xr[dst_k, h, d]), (E, H) in slot order (pg_gatv2_score): one fused pass, no (E, H, Fh)
    tensor."""
    Fh = _gatv2_args(dg, "gatv2_score", xl, xr, attn, H)
    s = torch.empty(dg.num_edges, H, dtype=torch.float32, device=xl.device) if out is None else out
    if _edge_heads(dg, "gatv2_score", s) != H:
        raise ValueError(f"gatv2_score: output {tuple(s.shape)} for {H} heads")
    args = (dg.fwd.struct(None), ptr(xl), _ld(xl), ptr(xr), _ld(xr), ptr(attn), H, Fh, float(slope), ptr(s),
            max(_ld(s), H))
    if dg.is_cuda:
        call("pg_gatv2_score", *args, _stream(xl))
    else:
        call("pg_gatv2_score_cpu", *args)
    return s


def gatv2_backward_pass(dg: DeviceGraph, ds: torch.Tensor, xl: torch.Tensor, xr: torch.Tensor,
                        attn: torch.Tensor, H: int, slope: float, transpose: bool, want_dx: bool,
                        dattn: Optional[torch.Tensor] = None, dx: Optional[torch.Tensor] = None
                        ) -> Optional[torch.Tensor]:
    """One pg_gatv2_bwd pass: over the in-CSR it returns dxr, over the transposed CSR
    (`transpose`, node operands swapped) dxl (into `dx` when given), or None without
    `want_dx`; `dattn` (H*Fh), when given, is filled by the same pass."""
    Fh = _gatv2_args(dg, "gatv2_backward_pass", xl, xr, attn, H)
    _check_device(dg, ds, dattn)
    if _edge_heads(dg, "gatv2_backward_pass", ds) != H:
        raise ValueError(f"gatv2_backward_pass: ds {tuple(ds.shape)} for {H} heads")
    if dattn is not None and (dattn.dtype != torch.float32 or dattn.numel() != H * Fh or not dattn.is_contiguous()):
        raise ValueError(f"gatv2_backward_pass: dattn {tuple(dattn.shape)} for {H} heads of {Fh}")
    own, gat = (xl, xr) if transpose else (xr, xl)
    if not want_dx:
        dx = None
    elif dx is None:
        dx = torch.empty(own.shape[0], H * Fh, dtype=torch.float32, device=xl.device)
    elif tuple(dx.shape) != tuple(own.shape) or dx.dtype != torch.float32 or dx.device != xl.device:
        raise ValueError(f"gatv2_backward_pass: dx {tuple(dx.shape)} for operands {tuple(xl.shape)}")
    g = (dg.bwd if transpose else dg.fwd).struct(None)
    args = (g, ptr(ds), max(_ld(ds), H), ptr(own), _ld(own), ptr(gat), _ld(gat), ptr(attn), H, Fh,
            float(slope), ptr(dx), _ld(dx) if want_dx else 0, ptr(dattn))
    if dg.is_cuda:
        ws_n = _lib.lib().pg_gatv2_bwd_workspace(g, H, Fh, int(dattn is not None))
        ws = _workspace(ws_n, xl.device)
        call("pg_gatv2_bwd", *args, ptr(ws), ws_n, _stream(xl))
    else:
        call("pg_gatv2_bwd_cpu", *args)
    return dx


def gatv2_score_backward(dg: DeviceGraph, ds: torch.Tensor, xl: torch.Tensor, xr: torch.Tensor,
                         attn: torch.Tensor, H: int, slope: float, need_xl: bool = True, need_xr: bool = True,
                         need_attn: bool = True):
    """(dxl, dxr, dattn) of gatv2_score for the (E, H) score gradient `ds` in slot order, each
    None unless asked for. dxr is one pass over the in-CSR, dxl the same kernel over the
    transposed CSR; dattn rides on the first pass that runs (a pass of its own when neither
    node gradient is wanted)."""
    dattn = torch.empty(attn.numel(), dtype=torch.float32, device=attn.device) if need_attn else None
    dxl = dxr = None
    da = dattn
    if need_xr or (need_attn and not need_xl):
        dxr = gatv2_backward_pass(dg, ds, xl, xr, attn, H, slope, False, need_xr, da)
        da = None
    if need_xl:
        dxl = gatv2_backward_pass(dg, ds, xl, xr, attn, H, slope, True, True, da)
    return dxl, dxr, dattn


def _gop_args(dg: DeviceGraph, name: str, op: str, lhs, rhs, lhs_target: str, rhs_target: str, targets: str,
              transpose: bool = False):
    """Checked operands of gspmm / gsddmm: (op code, lhs, rhs, F); an operand the operator
    does not read becomes None. 'u' rows are the sources and 'v' rows the destinations of the
    in-CSR; on the transposed CSR the two swap."""
    if op not in _lib.PG_OP:
        raise ValueError(f"{name}: unknown operator {op!r}")
    if op == "copy_rhs":
        lhs = None
    if op == "copy_lhs":
        rhs = None
    F = None
    for t, tgt, side in ((lhs, lhs_target, "lhs"), (rhs, rhs_target, "rhs")):
        if t is None:
            if (side == "lhs") != (op == "copy_rhs"):
                raise ValueError(f"{name}: {op} needs its {side} operand")
            continue
        if tgt not in targets:
            raise ValueError(f"{name}: {side} target {tgt!r}, one of {tuple(targets)} expected")
        n_u, n_v = (dg.num_dst, dg.num_src) if transpose else (dg.num_src, dg.num_dst)
        rows = dg.num_edges if tgt == "e" else (n_u if tgt == "u" else n_v)
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: float32 operands expected")
        if t.dim() != 2 or t.shape[0] != rows or (F is not None and t.shape[1] != F):
            raise ValueError(f"{name}: {side} operand {tuple(t.shape)} at target {tgt!r} on a graph of "
                             f"{dg.num_src} x {dg.num_dst} nodes and {dg.num_edges} edges")
        F = t.shape[1]
    _check_device(dg, lhs, rhs)
    return _lib.PG_OP[op], lhs, rhs, F


def _edge_index(dg: DeviceGraph, eidx, transpose: bool) -> Optional[torch.Tensor]:
    """`eidx` of pg_gspmm / pg_gsddmm: "eid" = edge tensors in edge-id order (the cached map),
    None = in-CSR slot order, or an int32 tensor with one edge row index per CSR entry."""
    if isinstance(eidx, str):
        if eidx != "eid":
            raise ValueError(f"eidx: 'eid', None or an int32 tensor expected, not {eidx!r}")
        return dg.edge_map(transpose)
    if eidx is not None and (eidx.dtype != torch.int32 or eidx.numel() != dg.num_edges
                             or eidx.device != dg.device or not eidx.is_contiguous()):
        raise ValueError("eidx: a contiguous int32 tensor with one entry per edge on the graph's device expected")
    return eidx


def _arg_kind(csr, arg_kind: Optional[int]) -> int:
    if arg_kind is None:
        arg_kind = _lib.PG_ARG_U16 if csr.max_deg < 0xFFFF else _lib.PG_ARG_I32
    if arg_kind not in (_lib.PG_ARG_U16, _lib.PG_ARG_I32):
        raise ValueError(f"arg_kind {arg_kind}")
    return arg_kind


def _arg_dtype(arg_kind: int):
    return torch.int16 if arg_kind == _lib.PG_ARG_U16 else torch.int32


def gspmm(dg: DeviceGraph, op: str, reduce: str, lhs: Optional[torch.Tensor], rhs: Optional[torch.Tensor],
          lhs_target: str = "u", rhs_target: str = "e", transpose: bool = False, eidx="eid",
          out: Optional[torch.Tensor] = None, argpos: Optional[torch.Tensor] = None,
          arg_kind: Optional[int] = None, want_arg: bool = True):
    """out[v] = reduce over the in-edges k of v of op(lhs[t_l(k)], rhs[t_r(k)]) (pg_gspmm): op
    in add / sub / mul / div / copy_lhs / copy_rhs, reduce in sum / mean / max / min, targets
    'u' (the source row) or 'e' (the edge row; `eidx`: see _edge_index). transpose=True runs on
    the out-CSR, where 'u' is the destination of each out-edge: the source-side gradients.
    Returns out for sum / mean, (out, argpos) for max / min (argpos None with want_arg=False)."""
    name = "gspmm"
    code, lhs, rhs, F = _gop_args(dg, name, op, lhs, rhs, lhs_target, rhs_target, "ue", transpose)
    if reduce not in ("sum", "mean", "max", "min"):
        raise ValueError(f"{name}: unknown reducer {reduce!r}")
    red = _lib.PG_RED["sum" if reduce == "mean" else reduce]
    csr = dg.bwd if transpose else dg.fwd
    g = csr.struct(None)
    emap = _edge_index(dg, eidx, transpose)
    n = dg.num_src if transpose else dg.num_dst
    dev = (lhs if lhs is not None else rhs).device
    if out is None:
        out = torch.empty(n, F, dtype=torch.float32, device=dev)
    cmp_ = reduce in ("max", "min")
    kind = _arg_kind(csr, arg_kind)
    if cmp_ and want_arg and argpos is None:
        argpos = torch.empty(n, F, dtype=_arg_dtype(kind), device=dev)
    if not cmp_:
        argpos = None
    _check_device(dg, out, argpos)
    if tuple(out.shape) != (n, F) or (argpos is not None and (tuple(argpos.shape) != (n, F)
                                                             or argpos.dtype != _arg_dtype(kind))):
        raise ValueError(f"{name}: output buffers do not match ({n}, {F}) / the record kind")
    args = (g, code, red, ptr(lhs), _ld(lhs) if lhs is not None else 0, _lib.PG_TGT[lhs_target],
            ptr(rhs), _ld(rhs) if rhs is not None else 0, _lib.PG_TGT[rhs_target], ptr(emap), F,
            int(reduce == "mean"), ptr(out), _ld(out), ptr(argpos), _ld(argpos) if argpos is not None else 0, kind)
    if dg.is_cuda:
        ws_n = _lib.lib().pg_gspmm_workspace(g, F, red, kind)
        ws = _workspace(ws_n, dev)
        call("pg_gspmm", *args, ptr(ws), ws_n, _stream(out))
    else:
        call("pg_gspmm_cpu", *args)
    return (out, argpos) if cmp_ else out


def gsddmm(dg: DeviceGraph, op: str, lhs: Optional[torch.Tensor], rhs: Optional[torch.Tensor],
           lhs_target: str = "u", rhs_target: str = "v", transpose: bool = False, eidx="eid",
           out: Optional[torch.Tensor] = None, argpos: Optional[torch.Tensor] = None,
           arg_kind: Optional[int] = None) -> torch.Tensor:
    """out[e] = op(lhs[t_l(e)], rhs[t_r(e)]) per edge (pg_gsddmm), (E, F) in the order `eidx`
    gives ("eid": edge-id order); targets 'u' (source), 'v' (destination), 'e'. With `argpos`
    (a max / min reduce's records) the value only where the edge won, +0 elsewhere."""
    name = "gsddmm"
    code, lhs, rhs, F = _gop_args(dg, name, op, lhs, rhs, lhs_target, rhs_target, "uve", transpose)
    csr = dg.bwd if transpose else dg.fwd
    emap = _edge_index(dg, eidx, transpose)
    dev = (lhs if lhs is not None else rhs).device
    if out is None:
        out = torch.empty(dg.num_edges, F, dtype=torch.float32, device=dev)
    kind = _arg_kind(csr, arg_kind)
    _check_device(dg, out, argpos)
    if tuple(out.shape) != (dg.num_edges, F) or out.dtype != torch.float32:
        raise ValueError(f"{name}: output {tuple(out.shape)}, ({dg.num_edges}, {F}) float32 expected")
    if argpos is not None and (tuple(argpos.shape) != (csr.n_rows, F) or argpos.dtype != _arg_dtype(kind)):
        raise ValueError(f"{name}: argpos does not match ({csr.n_rows}, {F}) / the record kind")
    args = (csr.struct(None), code, ptr(lhs), _ld(lhs) if lhs is not None else 0, _lib.PG_TGT[lhs_target],
            ptr(rhs), _ld(rhs) if rhs is not None else 0, _lib.PG_TGT[rhs_target], ptr(emap), F,
            ptr(out), _ld(out) if out.numel() else max(F, 1), ptr(argpos),
            _ld(argpos) if argpos is not None else 0, kind)
    if dg.is_cuda:
        call("pg_gsddmm", *args, _stream(out))
    else:
        call("pg_gsddmm_cpu", *args)
    return out


def segment_sum(dg: DeviceGraph, de_slots: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """Sums of (E, T) edge values in slot order over the in-edges of each node (transpose: the
    out-edges), (N, T): spmm_sum_heads with Fh = 1 and X = 1, at most 64 columns per call."""
    E, T = de_slots.shape
    n_out, n_in = (dg.num_src, dg.num_dst) if transpose else (dg.num_dst, dg.num_src)
    out = torch.empty(n_out, T, dtype=torch.float32, device=de_slots.device)
    for c0 in range(0, T, 64):
        Hc = min(64, T - c0)
        ones = torch.ones(n_in, Hc, dtype=torch.float32, device=de_slots.device)
        spmm_sum_heads(dg, de_slots[:, c0:c0 + Hc], ones, Hc, transpose=transpose, out=out[:, c0:c0 + Hc])
    return out


def argpos_to_src(dg: DeviceGraph, argpos: torch.Tensor) -> torch.Tensor:
    """DGL's argX (int64 source ids; -1 where a row has no in-edge)."""
    n, F = argpos.shape
    argx = torch.empty(n, F, dtype=torch.int64, device=argpos.device)
    g = dg.fwd.struct(None)
    if dg.is_cuda:
        call("pg_argpos_to_src", g, ptr(argpos), _ld(argpos), dg.arg_kind, F, ptr(argx), F,
             _stream(argpos))
    else:
        call("pg_argpos_to_src_cpu", g, ptr(argpos), _ld(argpos), dg.arg_kind, F, ptr(argx), F)
    return argx


# ------------------------------------------------------------------ sampling
def _ids32(t, device, name: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 1:
        raise TypeError(f"{name}: a 1-D int32 / int64 id tensor expected")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _excl_bits(dg: DeviceGraph, bits: torch.Tensor, name: str) -> torch.Tensor:
    if bits.dtype != torch.int32 or bits.dim() != 1 or not bits.is_contiguous() or bits.device != dg.device \
            or bits.numel() < (dg.num_edges + 31) // 32:
        raise TypeError(f"{name}: the exclusion bit set is a contiguous int32 tensor of ceil(num_edges / 32) "
                        "words on the graph's device (DeviceGraph.exclusion_bits())")
    return bits


def edge_bits_update(bits: torch.Tensor, n_edge_ids: int, eids, set: bool = True, check: bool = True) -> None:
    """Set (or clear) the bits of edge ids `eids` in `bits` (pg_edge_bits_update): bit e & 31 of
    word e >> 5 stands for edge id e; int32 words, in place, on bits' device. Duplicates are fine.
    An id outside [0, n_edge_ids) is skipped; with `check` it raises ValueError after the update
    (one device-to-host read of the status), without it nothing is read back."""
    n_edge_ids = int(n_edge_ids)
    if bits.dtype != torch.int32 or bits.dim() != 1 or not bits.is_contiguous() \
            or bits.numel() < (n_edge_ids + 31) // 32:
        raise TypeError("edge_bits_update: bits must be a contiguous int32 tensor of ceil(n_edge_ids / 32) words")
    eids = _ids32(eids, bits.device, "edge_bits_update")
    status = torch.zeros(1, dtype=torch.int32, device=bits.device) if check else None
    args = (ptr(bits), n_edge_ids, ptr(eids), eids.numel(), 1 if set else 0, ptr(status))
    if bits.device.type == "cuda":
        call("pg_edge_bits_update", *args, _stream(bits))
    else:
        call("pg_edge_bits_update_cpu", *args)
    if check and int(status[0]) != 0:
        raise ValueError(f"edge_bits_update: edge ids outside [0, {n_edge_ids})")


def sample_neighbors(dg: DeviceGraph, seeds, fanout: int, seed: int, exclude: Optional[torch.Tensor] = None):
    """Up to `fanout` in-edges of every seed node, without replacement (pg_sample_count +
    pg_sample_fill): (ptr, col, eid) of the sampled in-CSR, int32 on the graph's device, row i
    for seeds[i], col = parent source ids, eid = parent edge ids ascending in each row.
    fanout < 0 keeps whole rows. The result is a function of (graph, seeds, fanout, seed)
    only. One device-to-host read lies between the two calls: the entry count, and with it
    whether a seed lies outside the graph (ValueError; the count kernel itself takes such a seed
    as a row without entries).

    exclude: a bit set over the graph's edge ids (DeviceGraph.exclusion_bits(), filled by
    edge_bits_update). The result is then that of the graph with those edges deleted and the
    edge ids kept (pg_sample_count_excl + pg_sample_fill_excl): a row still receives `fanout`
    neighbours from the edges that remain. None calls the plain entry points."""
    seeds = _ids32(seeds, dg.device, "sample_neighbors")
    n = seeds.numel()
    fanout, seed = int(fanout), int(seed) & 0xFFFFFFFFFFFFFFFF
    g = dg.fwd.struct(None)
    emap = dg.edge_map()
    out_ptr = torch.empty(n + 1, dtype=torch.int32, device=dg.device)
    if exclude is not None:
        return _sample_neighbors_excl(dg, g, emap, seeds, fanout, seed, _excl_bits(dg, exclude, "sample_neighbors"),
                                      out_ptr)
    if dg.is_cuda:
        ws_n = _lib.lib().pg_sample_count_workspace(n)
        ws = _workspace(ws_n, dg.device)
        call("pg_sample_count", g, ptr(seeds), n, fanout, ptr(out_ptr), ptr(ws), ws_n, _stream(out_ptr))
    else:
        call("pg_sample_count_cpu", g, ptr(seeds), n, fanout, ptr(out_ptr))
    bad = ((seeds < 0) | (seeds >= dg.num_dst)).any().to(torch.int32).reshape(1)
    total, bad = torch.cat([out_ptr[n:], bad]).tolist()  # one read-back for both
    if bad:
        raise ValueError(f"sample_neighbors: seed ids outside [0, {dg.num_dst})")
    col = torch.empty(total, dtype=torch.int32, device=dg.device)
    eid = torch.empty(total, dtype=torch.int32, device=dg.device)
    args = (g, ptr(emap), ptr(seeds), n, fanout, seed, ptr(out_ptr), ptr(col), ptr(eid))
    if total:
        if dg.is_cuda:
            call("pg_sample_fill", *args, _stream(out_ptr))
        else:
            call("pg_sample_fill_cpu", *args)
    return out_ptr, col, eid


def _sample_neighbors_excl(dg, g, emap, seeds, fanout, seed, bits, out_ptr):
    n = seeds.numel()
    if dg.is_cuda:
        ws_n = _lib.lib().pg_sample_count_excl_workspace(n)
        ws = _workspace(ws_n, dg.device)
        call("pg_sample_count_excl", g, ptr(emap), ptr(seeds), n, fanout, ptr(bits), ptr(out_ptr), ptr(ws), ws_n,
             _stream(out_ptr))
    else:
        call("pg_sample_count_excl_cpu", g, ptr(emap), ptr(seeds), n, fanout, ptr(bits), ptr(out_ptr))
    bad = ((seeds < 0) | (seeds >= dg.num_dst)).any().to(torch.int32).reshape(1)
    total, bad = torch.cat([out_ptr[n:], bad]).tolist()  # one read-back for both
    if bad:
        raise ValueError(f"sample_neighbors: seed ids outside [0, {dg.num_dst})")
    col = torch.empty(total, dtype=torch.int32, device=dg.device)
    eid = torch.empty(total, dtype=torch.int32, device=dg.device)
    args = (g, ptr(emap), ptr(seeds), n, fanout, seed, ptr(bits), ptr(out_ptr), ptr(col), ptr(eid))
    if total:
        if dg.is_cuda:
            call("pg_sample_fill_excl", *args, _stream(out_ptr))
        else:
            call("pg_sample_fill_excl_cpu", *args)
    return out_ptr, col, eid


def edge_lookup(dg: DeviceGraph, u, v) -> torch.Tensor:
    """int32 edge id of every pair u[i] -> v[i] (pg_edge_lookup): the smallest id when the graph
    holds the edge more than once, -1 when it does not hold it or an end lies outside the graph.
    On the graph's device; nothing is read back."""
    u = _ids32(u, dg.device, "edge_lookup")
    v = _ids32(v, dg.device, "edge_lookup")
    if u.numel() != v.numel():
        raise ValueError("edge_lookup: u and v lengths differ")
    out = torch.empty(u.numel(), dtype=torch.int32, device=dg.device)
    args = (dg.fwd.struct(None), ptr(dg.edge_map()), ptr(u), ptr(v), u.numel(), ptr(out))
    if dg.is_cuda:
        call("pg_edge_lookup", *args, _stream(out))
    else:
        call("pg_edge_lookup_cpu", *args)
    return out


def negative_sample(dg: DeviceGraph, pos_src, pos_id, n_pos: int, k: int, seed: int, tries: int = 32,
                    reject_edge: bool = False, reject_self: bool = False):
    """k negative pairs per positive edge (pg_negative_sample): (neg_src, neg_dst, n_fail), int32
    on the graph's device, slot (i, j) at i * k + j. The source is pos_src[i] (None: drawn over
    the graph's sources), the destination is drawn over its destinations; up to `tries` attempts
    per slot, the first that is no edge (reject_edge) and no self-pair (reject_self) wins. A slot
    without one holds -1 in both outputs and counts in n_fail (a 1-element tensor: nothing is
    read back here). The draws depend on (seed, pos_id[i] (None: i), j, attempt) only."""
    n_pos, k = int(n_pos), int(k)
    if pos_src is not None:
        pos_src = _ids32(pos_src, dg.device, "negative_sample")
    if pos_id is not None:
        pos_id = _ids32(pos_id, dg.device, "negative_sample")
    for t in (pos_src, pos_id):
        if t is not None and t.numel() != n_pos:
            raise ValueError("negative_sample: pos_src / pos_id must hold n_pos ids")
    n_out = max(n_pos, 0) * max(k, 0)
    neg_src = torch.empty(n_out, dtype=torch.int32, device=dg.device)
    neg_dst = torch.empty(n_out, dtype=torch.int32, device=dg.device)
    n_fail = torch.empty(1, dtype=torch.int32, device=dg.device)
    flags = (_lib.PG_NEG_REJECT_EDGE if reject_edge else 0) | (_lib.PG_NEG_REJECT_SELF if reject_self else 0)
    args = (dg.fwd.struct(None), ptr(pos_src), ptr(pos_id), n_pos, k, int(tries), flags,
            int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(neg_src), ptr(neg_dst), ptr(n_fail))
    if dg.is_cuda:
        call("pg_negative_sample", *args, _stream(neg_src))
    else:
        call("pg_negative_sample_cpu", *args)
    return neg_src, neg_dst, n_fail


def block_compact(dst_ids, col, n_parent: int):
    """(src_ids, col_local) of a block (pg_block_compact): src_ids = dst_ids followed by every
    other parent id of `col` in the order of its first appearance there, col_local[k] = the
    position of col[k] in src_ids; int32 on col's device. Duplicate dst_ids: ValueError. One
    device-to-host read (the source count)."""
    col = torch.as_tensor(col)
    dev = col.device
    col = _ids32(col, dev, "block_compact")
    dst_ids = _ids32(dst_ids, dev, "block_compact")
    n_dst, nnz, n_parent = dst_ids.numel(), col.numel(), int(n_parent)
    src_ids = torch.empty(n_dst + nnz, dtype=torch.int32, device=dev)
    col_local = torch.empty(nnz, dtype=torch.int32, device=dev)
    n_src = torch.empty(1, dtype=torch.int32, device=dev)
    args = (ptr(dst_ids), n_dst, ptr(col), nnz, n_parent, ptr(src_ids), ptr(col_local), ptr(n_src))
    if dev.type == "cuda":
        ws_n = _lib.lib().pg_block_compact_workspace(n_dst, nnz, n_parent)
        ws = _workspace(ws_n, dev)
        call("pg_block_compact", *args, ptr(ws), ws_n, _stream(col_local))
    else:
        call("pg_block_compact_cpu", *args)
    n = int(n_src[0])
    if n == -1:
        raise ValueError("block_compact: dst_ids holds a duplicate")
    if n < 0:
        raise ValueError(f"block_compact: an id lies outside [0, {n_parent})")
    return src_ids[:n], col_local


# ------------------------------------------------------------------ dense
def _split_k(M: int, N: int, K: int) -> int:
    """K-split for long-K products (weight gradients): the library's recommendation
    (pg_gemm_f32_split_k: ~3 workgroups per CU, slices of >= 96 K entries)."""
    return int(_lib.lib().pg_gemm_f32_split_k(M, N, K))


def gemm(A: torch.Tensor, B: torch.Tensor, transa: bool = False, transb: bool = False,
         out: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 0.0,
         bias: Optional[torch.Tensor] = None, act: int = _lib.PG_ACT_NONE,
         slope: float = LEAKY_SLOPE, split_k: Optional[int] = None,
         dact: Optional[torch.Tensor] = None, rowsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """C = alpha*op(A)@op(B) + beta*C (+bias, act): f32 GEMM on the GPU (three-piece bf16 MFMA
    products where the operands are aligned, the f32 MFMA kernel otherwise; f32 accuracy) or
    torch-CPU (CPU device). With `dact` (an activation output) the result is instead
    multiplied by act'(dact): the fused activation backward. With `rowsum`, also
    rowsum[m] = sum_k op(A)[m][k] (bias gradients of a weight-gradient product)."""
    M = A.shape[1] if transa else A.shape[0]
    K = A.shape[0] if transa else A.shape[1]
    Kb = B.shape[1] if transb else B.shape[0]
    N = B.shape[0] if transb else B.shape[1]
    if K != Kb:
        raise ValueError(f"gemm: inner dims {K} vs {Kb}")
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm: beta != 0 needs out")
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    if A.device.type != "cuda":
        a = A.t() if transa else A
        b = B.t() if transb else B
        r = alpha * (a @ b)
        if beta != 0.0:
            r = r + beta * out
        if bias is not None:
            r = r + bias
        if dact is not None:
            r = torch.where(dact > 0, r, r * slope if act == _lib.PG_ACT_LEAKY else r * 0)
        elif act == _lib.PG_ACT_RELU:
            r = torch.relu(r)
        elif act == _lib.PG_ACT_LEAKY:
            r = torch.nn.functional.leaky_relu(r, slope)
        out.copy_(r)
        if rowsum is not None:
            rowsum.copy_((A.t() if transa else A).sum(1))
        return out
    if split_k is None:
        split_k = 1 if (bias is not None or act != _lib.PG_ACT_NONE or dact is not None
                        or beta not in (0.0, 1.0)) else _split_k(M, N, K)
    ws_n = _lib.lib().pg_gemm_f32_workspace(M, N, K, split_k)
    ws = _workspace(ws_n, A.device)
    ep = _lib.epilogue(bias, act, slope, dact, rowsum)
    call("pg_gemm_f32", int(transa), int(transb), M, N, K, alpha, ptr(A), _ld(A), ptr(B), _ld(B),
         beta, ptr(out), _ld(out), ep, split_k, ptr(ws), ws_n, _stream(A))
    return out


PG_ERR_UNSUPPORTED = -2


def gemm_cat(A1: torch.Tensor, A2: torch.Tensor, B1: torch.Tensor, B2: torch.Tensor, transb: bool = False,
             out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
             act: int = _lib.PG_ACT_NONE) -> Optional[torch.Tensor]:
    """C = [A1 | A2] @ op([B1 ; B2]) (+ bias, leaky_relu) without building either
    concatenation (pg_gemm_f32_cat, GPU). Returns None when the library does not take these
    operands (PG_ERR_UNSUPPORTED: the caller concatenates instead)."""
    M, K1 = A1.shape
    K2 = A2.shape[1]
    N = B1.shape[0] if transb else B1.shape[1]
    if A2.shape[0] != M or (B1.shape[1] if transb else B1.shape[0]) != K1 or \
            (B2.shape[1] if transb else B2.shape[0]) != K2 or (B2.shape[0] if transb else B2.shape[1]) != N:
        raise ValueError("gemm_cat: shapes do not concatenate")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A1.device)
    ep = _lib.epilogue(bias, act, LEAKY_SLOPE)
    rc = _lib.lib().pg_gemm_f32_cat(int(transb), M, N, K1, K2, 1.0, ptr(A1), _ld(A1), ptr(A2), _ld(A2), ptr(B1),
                                    _ld(B1), ptr(B2), _ld(B2), 0.0, ptr(out), _ld(out), ep, _stream(A1))
    if rc == PG_ERR_UNSUPPORTED:
        return None
    _lib.check(rc, "pg_gemm_f32_cat")
    return out


def gemm_group(parts) -> None:
    """Several split-K products in one launch + one combine (pg_gemm_f32_group): each part
    (A, B, C, transa, transb, beta, rowsum) computes C = op(A) op(B) (+ C when beta = 1) and
    rowsum = the row sums of op(A) when given. The weight gradients of a layer's backward."""
    if not parts:
        return
    dev = parts[0][0].device
    if dev.type != "cuda":
        for A, B, C, ta, tb, beta, rs in parts:
            gemm(A, B, transa=ta, transb=tb, out=C, beta=beta, rowsum=rs)
        return
    arr = (_lib.PgGemmPart * len(parts))()
    for q, (A, B, C, ta, tb, beta, rs) in zip(arr, parts):
        q.transa, q.transb = int(ta), int(tb)
        q.M = A.shape[1] if ta else A.shape[0]
        q.K = A.shape[0] if ta else A.shape[1]
        q.N = B.shape[0] if tb else B.shape[1]
        q.A, q.lda, q.B, q.ldb = ptr(A), _ld(A), ptr(B), _ld(B)
        q.beta, q.C, q.ldc, q.rowsum = beta, ptr(C), _ld(C), ptr(rs)
    ws_n = _lib.lib().pg_gemm_f32_group_workspace(arr, len(parts))
    ws = _workspace(ws_n, dev)
    call("pg_gemm_f32_group", arr, len(parts), ptr(ws), ws_n, _stream(parts[0][0]))


def gemm_bf16(A: torch.Tensor, B: torch.Tensor, transa: bool = False, transb: bool = False,
              out: Optional[torch.Tensor] = None, out_dtype=torch.float32, alpha: float = 1.0,
              beta: float = 0.0, bias: Optional[torch.Tensor] = None, act: int = _lib.PG_ACT_NONE,
              slope: float = LEAKY_SLOPE, split_k: Optional[int] = None,
              dact: Optional[torch.Tensor] = None, rowsum: Optional[torch.Tensor] = None
              ) -> torch.Tensor:
    """pg_gemm_bf16: bfloat16 operands, f32 accumulate on v_mfma_f32_32x32x16_bf16, output
    float32 or bfloat16 (`out` / `out_dtype`), the same epilogues as gemm() (bias f32, dact
    bfloat16, rowsum f32)."""
    if A.dtype != torch.bfloat16 or B.dtype != torch.bfloat16 or A.device.type != "cuda":
        raise TypeError("gemm_bf16: bfloat16 operands on a HIP device expected")
    M = A.shape[1] if transa else A.shape[0]
    K = A.shape[0] if transa else A.shape[1]
    Kb = B.shape[1] if transb else B.shape[0]
    N = B.shape[0] if transb else B.shape[1]
    if K != Kb:
        raise ValueError(f"gemm_bf16: inner dims {K} vs {Kb}")
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm_bf16: beta != 0 needs out")
        out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("gemm_bf16: float32 or bfloat16 output")
    if dact is not None and dact.dtype != torch.bfloat16:
        raise TypeError("gemm_bf16: dact must be bfloat16")
    obf = out.dtype == torch.bfloat16
    if split_k is None:
        split_k = 1 if (obf or bias is not None or act != _lib.PG_ACT_NONE or dact is not None
                        or beta not in (0.0, 1.0)) else int(_lib.lib().pg_gemm_bf16_split_k(M, N, K))
    ws_n = _lib.lib().pg_gemm_bf16_workspace(M, N, K, split_k)
    ws = _workspace(ws_n, A.device)
    ep = _lib.epilogue(bias, act, slope, dact, rowsum)
    call("pg_gemm_bf16", int(transa), int(transb), M, N, K, alpha, ptr(A), _ld(A), ptr(B), _ld(B),
         beta, ptr(out), _ld(out), _lib.PG_DTYPE_BF16 if obf else _lib.PG_DTYPE_F32, ep, split_k,
         ptr(ws), ws_n, _stream(A))
    return out


def cast_bf16(src: torch.Tensor, index: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16(src[index]) (round to nearest even; index < 0 gives 0) with pg_cast_f32_bf16."""
    if src.dtype != torch.float32 or not src.is_contiguous():
        raise TypeError("cast_bf16: contiguous float32 source expected")
    n = index.numel() if index is not None else src.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.bfloat16, device=src.device)
    if index is not None and index.dtype != torch.int32:
        raise TypeError("cast_bf16: int32 index expected")
    call("pg_cast_f32_bf16", ptr(src), ptr(index), n, ptr(out), _stream(src))
    return out


def pad2d_group(parts) -> None:
    """dst[:rows, :cols] = src, the rest of dst zero, for each (src, dst) pair of 2-D f32
    tensors (unit column stride): one pg_pad2d_group launch per PG_PAD2D_MAX parts on the
    GPU, torch on the CPU."""
    parts = [(s.contiguous(), d) for s, d in parts]
    if not parts:
        return
    if parts[0][1].device.type != "cuda":
        for src, dst in parts:
            dst.zero_()
            dst[:src.shape[0], :src.shape[1]].copy_(src)
        return
    for i in range(0, len(parts), _lib.PG_PAD2D_MAX):
        chunk = parts[i:i + _lib.PG_PAD2D_MAX]
        arr = (_lib.PgPad2d * len(chunk))()
        for k, (src, dst) in enumerate(chunk):
            if dst.stride(1) != 1 or src.dtype != torch.float32 or dst.dtype != torch.float32:
                raise ValueError("pad2d_group: f32 operands with unit column stride expected")
            arr[k] = _lib.PgPad2d(ptr(src), _ld(src), src.shape[0], src.shape[1], ptr(dst), dst.stride(0),
                                  dst.shape[0], dst.shape[1])
        call("pg_pad2d_group", arr, len(chunk), _stream(chunk[0][1]))


def col_sum(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False
            ) -> torch.Tensor:
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    if x.device.type != "cuda":
        s = x.sum(0)
        out.copy_(out + s if accumulate else s)
        return out
    ws_n = _lib.lib().pg_col_sum_workspace(rows, cols)
    ws = _workspace(ws_n, x.device)
    call("pg_col_sum", ptr(x), _ld(x), rows, cols, ptr(out), int(accumulate), ptr(ws), ws_n,
         _stream(x))
    return out


# ------------------------------------------------------------------ autograd
class MaxAggregate(torch.autograd.Function):
    """update_all(copy_u('h','m') | u_mul_e, max('m','neigh')) with the DGL backward; the
    weights' gradient (u_mul_e) is the per-edge product over the features the edge won."""

    @staticmethod
    def forward(ctx, X, dg, ew_slots):
        X = X.contiguous()
        out, argpos = spmm_max(dg, X, ew_slots)
        ctx.dg = dg
        ctx.need_ew = ew_slots is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(argpos, ew_slots, X if ctx.need_ew else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        argpos, ew_slots, X = ctx.saved_tensors
        dout = dout.contiguous()
        dx = spmm_max_backward(ctx.dg, argpos, dout, ew_slots) if ctx.needs_input_grad[0] else None
        d_ew = sddmm_dot(ctx.dg, dout, X, argpos=argpos) if ctx.need_ew else None
        return dx, None, d_ew


class SumAggregate(torch.autograd.Function):
    """update_all(copy_u | u_mul_e, sum | mean); backward on the transposed CSR, the
    weights' gradient (u_mul_e) as per-edge dot products of dout and X."""

    @staticmethod
    def forward(ctx, X, dg, ew_slots, mean):
        X = X.contiguous()
        ctx.dg, ctx.mean = dg, mean
        ctx.need_ew = ew_slots is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(ew_slots, X if ctx.need_ew else None)
        return spmm_sum(dg, X, mean, ew_slots)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        ew_slots, X = ctx.saved_tensors
        dout = dout.contiguous()
        dx = spmm_sum(ctx.dg, dout, ctx.mean, ew_slots, transpose=True) if ctx.needs_input_grad[0] else None
        d_ew = sddmm_dot(ctx.dg, dout, X, mean=ctx.mean) if ctx.need_ew else None
        return dx, None, d_ew, None


class EdgeDot(torch.autograd.Function):
    """apply_edges(u_dot_v(lhs, rhs, out)): de[k] = sum_f lhs[src_k, f] * rhs[dst_k, f] in
    in-CSR slot order (pg_sddmm_dot); the input gradients are weighted sum aggregations
    with the incoming edge gradient as the weights."""

    @staticmethod
    def forward(ctx, lhs, rhs, dg):
        lhs, rhs = lhs.contiguous(), rhs.contiguous()
        ctx.dg = dg
        ctx.save_for_backward(lhs, rhs)
        return sddmm_dot(dg, rhs, lhs)

    @staticmethod
    @once_differentiable
    def backward(ctx, de):
        lhs, rhs = ctx.saved_tensors
        de = de.contiguous()
        d_lhs = spmm_sum(ctx.dg, rhs, ew_slots=de, transpose=True) if ctx.needs_input_grad[0] else None
        d_rhs = spmm_sum(ctx.dg, lhs, ew_slots=de) if ctx.needs_input_grad[1] else None
        return d_lhs, d_rhs, None


class EdgeSoftmax(torch.autograd.Function):
    """edge_softmax over (E, H) scores in slot order; the backward is one
    edge_softmax_backward call on the saved output."""

    @staticmethod
    def forward(ctx, scores_slots, dg):
        a = edge_softmax(dg, scores_slots.contiguous())
        ctx.dg = dg
        ctx.save_for_backward(a)
        return a

    @staticmethod
    @once_differentiable
    def backward(ctx, da):
        (a,) = ctx.saved_tensors
        return edge_softmax_backward(ctx.dg, a, da.contiguous()), None


class SumAggregateHeads(torch.autograd.Function):
    """update_all(u_mul_e, sum) on (N, H*Fh) features with (E, H) weights in slot order
    (GATConv's aggregation): dX on the transposed CSR, dA as per-head dot products of dout and
    X, each only when needed."""

    @staticmethod
    def forward(ctx, X, dg, A_slots, H):
        X, A_slots = X.contiguous(), A_slots.contiguous()
        ctx.dg, ctx.H = dg, H
        ctx.save_for_backward(A_slots if ctx.needs_input_grad[0] else None,
                              X if ctx.needs_input_grad[2] else None)
        return spmm_sum_heads(dg, A_slots, X, H)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        A_slots, X = ctx.saved_tensors
        dout = dout.contiguous()
        dx = spmm_sum_heads(ctx.dg, A_slots, dout, ctx.H, transpose=True) if ctx.needs_input_grad[0] else None
        dA = sddmm_dot_heads(ctx.dg, dout, X, ctx.H) if ctx.needs_input_grad[2] else None
        return dx, None, dA, None


class EdgeDotHeads(torch.autograd.Function):
    """apply_edges(u_dot_v) on (N, H*Fh) operands: de[k, h] = <lhs[src_k, head h], rhs[dst_k,
    head h]>, (E, H) in slot order; the input gradients are per-head weighted sums with the
    incoming edge gradient as the weights (EdgeDot's backward, per head)."""

    @staticmethod
    def forward(ctx, lhs, rhs, dg, H):
        lhs, rhs = lhs.contiguous(), rhs.contiguous()
        ctx.dg, ctx.H = dg, H
        ctx.save_for_backward(lhs, rhs)
        return sddmm_dot_heads(dg, rhs, lhs, H)

    @staticmethod
    @once_differentiable
    def backward(ctx, de):
        lhs, rhs = ctx.saved_tensors
        de = de.contiguous()
        d_lhs = spmm_sum_heads(ctx.dg, de, rhs, ctx.H, transpose=True) if ctx.needs_input_grad[0] else None
        d_rhs = spmm_sum_heads(ctx.dg, de, lhs, ctx.H) if ctx.needs_input_grad[1] else None
        return d_lhs, d_rhs, None, None


class GATv2Score(torch.autograd.Function):
    """GATv2 attention scores (gatv2_score) of (N, H*Fh) source and destination projections,
    (E, H) in slot order, so they feed EdgeSoftmax and SumAggregateHeads with no reorder.
    Saves xl, xr and attn only: the backward recomputes the pre-activations from the node rows
    and runs only the passes `needs_input_grad` asks for."""

    @staticmethod
    def forward(ctx, xl, xr, attn, dg, H, slope):
        xl, xr = xl.contiguous(), xr.contiguous()
        flat = attn.contiguous().reshape(-1)
        ctx.dg, ctx.H, ctx.slope, ctx.attn_shape = dg, H, float(slope), attn.shape
        ctx.save_for_backward(xl, xr, flat)
        return gatv2_score(dg, xl, xr, flat, H, slope)

    @staticmethod
    @once_differentiable
    def backward(ctx, ds):
        xl, xr, flat = ctx.saved_tensors
        need = ctx.needs_input_grad
        dxl, dxr, dattn = gatv2_score_backward(ctx.dg, ds.contiguous(), xl, xr, flat, ctx.H, ctx.slope,
                                               need_xl=need[0], need_xr=need[1], need_attn=need[2])
        if dattn is not None:
            dattn = dattn.reshape(ctx.attn_shape)
        return dxl, dxr, dattn, None, None, None


class EdgeAdd(torch.autograd.Function):
    """apply_edges(u_add_v): out[e] = lhs[src_e] + rhs[dst_e] for (N, T) operands, (E, T) in
    edge-id order. The forward is two gathers; the backward's segment sums over the in-edges
    (d_rhs) and the out-edges (d_lhs) run on the engine in a fixed order (segment_sum), not
    as an index_add_ over repeated indices."""

    @staticmethod
    def forward(ctx, lhs, rhs, dg, src, dst):
        ctx.dg = dg
        return lhs.index_select(0, src) + rhs.index_select(0, dst)

    @staticmethod
    @once_differentiable
    def backward(ctx, de):
        de_slots = de.index_select(0, ctx.dg.eid).contiguous()
        d_lhs = segment_sum(ctx.dg, de_slots, transpose=True) if ctx.needs_input_grad[0] else None
        d_rhs = segment_sum(ctx.dg, de_slots) if ctx.needs_input_grad[1] else None
        return d_lhs, d_rhs, None, None, None


def _local_grad(op: str, side: str):
    """(kind, sign) of dz/dx for z = op(lhs, rhs) and x the operand on `side`, y its partner:
    'one' (sign), 'partner' (y), 'inv' (1 / y), 'den' (-y / x^2); None: z does not depend on x."""
    if op == "add":
        return "one", 1.0
    if op == "sub":
        return "one", 1.0 if side == "lhs" else -1.0
    if op == "mul":
        return "partner", 1.0
    if op == "div":
        return ("inv", 1.0) if side == "lhs" else ("den", 1.0)
    if (op, side) in (("copy_lhs", "lhs"), ("copy_rhs", "rhs")):
        return "one", 1.0
    return None


def _finish_grad(kind: str, sign: float, s: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    if kind == "den":
        return -s / (x * x)
    return s if sign == 1.0 else -s


def _edge_term(dg, kind: str, d, d_target: str, y, y_target: str, argpos=None, arg_kind=None):
    """(E, F) in edge-id order: d[t_d(e)] times the partner factor of `kind` (without a 'den'
    operand's own -1 / x^2), through pg_gsddmm; masked by `argpos` when given."""
    if kind == "one":
        return gsddmm(dg, "copy_lhs", d, None, d_target, "e", argpos=argpos, arg_kind=arg_kind)
    return gsddmm(dg, "div" if kind == "inv" else "mul", d, y, d_target, y_target, argpos=argpos,
                  arg_kind=arg_kind)


class GSpMM(torch.autograd.Function):
    """out[v] = reduce over in-edges of op(lhs, rhs) with one operand at 'u' ((N, F)) and one at
    'e' ((E, F), edge-id order), or a copy of either (pg_gspmm). Backward, only where needed:
    sum / mean: a 'u' operand's gradient is pg_gspmm on the transposed CSR with dout as the
    gathered operand, an 'e' operand's one pg_gsddmm with dout at 'v'; max / min: the masked
    pg_gsddmm gives the winners' gradient per edge, an 'e' operand takes it, a 'u' operand its
    sum over the out-edges (pg_gspmm copy_rhs on the transposed CSR)."""

    @staticmethod
    def forward(ctx, dg, op, reduce, lhs, rhs, lhs_target, rhs_target):
        lhs = lhs.contiguous() if lhs is not None and op != "copy_rhs" else None
        rhs = rhs.contiguous() if rhs is not None and op != "copy_lhs" else None
        if lhs is not None and rhs is not None and {lhs_target, rhs_target} != {"u", "e"}:
            raise NotImplementedError("GSpMM: a binary message takes one operand at 'u' and one at 'e'")
        ctx.dg, ctx.op, ctx.reduce, ctx.targets = dg, op, reduce, (lhs_target, rhs_target)
        argpos = None
        if reduce in ("max", "min"):
            need = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
            out, argpos = gspmm(dg, op, reduce, lhs, rhs, lhs_target, rhs_target, want_arg=need)
        else:
            out = gspmm(dg, op, reduce, lhs, rhs, lhs_target, rhs_target)
        ctx.save_for_backward(lhs, rhs, argpos)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lhs, rhs, argpos = ctx.saved_tensors
        dg, op = ctx.dg, ctx.op
        d = dout.contiguous()
        if ctx.reduce == "mean":
            d = d / dg.fwd.ptr.diff().clamp(min=1).to(d.dtype)[:, None]
        cmp_ = ctx.reduce in ("max", "min")
        grads = [None, None]
        for i, side in enumerate(("lhs", "rhs")):
            x, y = (lhs, rhs) if i == 0 else (rhs, lhs)
            loc = _local_grad(op, side)
            if x is None or loc is None or not ctx.needs_input_grad[3 + i]:
                continue
            kind, sign = loc
            xt, yt = ctx.targets[i], ctx.targets[1 - i]
            if xt == "e":
                s = _edge_term(dg, kind, d, "v", y, yt, argpos)
            elif cmp_:
                t = _edge_term(dg, kind, d, "v", y, yt, argpos)
                s = gspmm(dg, "copy_rhs", "sum", None, t, "u", "e", transpose=True)
            elif kind == "one":
                s = gspmm(dg, "copy_lhs", "sum", d, None, "u", "e", transpose=True)
            else:
                s = gspmm(dg, "div" if kind == "inv" else "mul", "sum", d, y, "u", "e", transpose=True)
            grads[i] = _finish_grad(kind, sign, s, x)
        return None, None, None, grads[0], grads[1], None, None


class GSDDMM(torch.autograd.Function):
    """out[e] = op(lhs[t_l(e)], rhs[t_r(e)]), (E, F) in edge-id order, two different targets of
    'u', 'v', 'e' (pg_gsddmm). Backward: a node operand's gradient is pg_gspmm (mul | div |
    copy_rhs, sum) with the upstream edge gradient as the 'e' operand, on the in-CSR for an
    operand at 'v' and on the transposed CSR for one at 'u'; an edge operand's gradient is
    another pg_gsddmm."""

    @staticmethod
    def forward(ctx, dg, op, lhs, rhs, lhs_target, rhs_target):
        lhs = lhs.contiguous() if lhs is not None and op != "copy_rhs" else None
        rhs = rhs.contiguous() if rhs is not None and op != "copy_lhs" else None
        if lhs is not None and rhs is not None and lhs_target == rhs_target:
            raise NotImplementedError("GSDDMM: the two operands sit at different targets")
        ctx.dg, ctx.op, ctx.targets = dg, op, (lhs_target, rhs_target)
        ctx.save_for_backward(lhs, rhs)
        return gsddmm(dg, op, lhs, rhs, lhs_target, rhs_target)

    @staticmethod
    @once_differentiable
    def backward(ctx, de):
        lhs, rhs = ctx.saved_tensors
        dg, op = ctx.dg, ctx.op
        de = de.contiguous()
        grads = [None, None]
        for i, side in enumerate(("lhs", "rhs")):
            x, y = (lhs, rhs) if i == 0 else (rhs, lhs)
            loc = _local_grad(op, side)
            if x is None or loc is None or not ctx.needs_input_grad[2 + i]:
                continue
            kind, sign = loc
            xt, yt = ctx.targets[i], ctx.targets[1 - i]
            if xt == "e":
                s = de if kind == "one" else _edge_term(dg, kind, de, "e", y, yt)
            else:
                tr = xt == "u"  # rows of the CSR = x's side; its 'u' target = the other node side
                if kind == "one":
                    s = gspmm(dg, "copy_rhs", "sum", None, de, "u", "e", transpose=tr)
                elif yt == "e":
                    s = gspmm(dg, "copy_rhs", "sum", None, de / y if kind == "inv" else de * y, "u", "e",
                              transpose=tr)
                elif kind == "inv":
                    s = gspmm(dg, "div", "sum", de, y, "e", "u", transpose=tr)
                else:
                    s = gspmm(dg, "mul", "sum", y, de, "u", "e", transpose=tr)
            grads[i] = _finish_grad(kind, sign, s, x)
        return None, None, grads[0], grads[1], None, None


def _padded(n: int, F: int, device) -> torch.Tensor:
    """(n, F) view of an (n, round4(F)) buffer whose pad columns are zero."""
    Fp = round4(F)
    buf = torch.empty(n, Fp, dtype=torch.float32, device=device)
    if Fp > F:
        buf[:, F:].zero_()
    return buf


def sage_width(F: int, align: int = 4) -> int:
    """TrainEngine's SAGE input width: a multiple of 64 when that costs <= 2 % more columns
    (503 -> 512: whole SpMM feature tiles, the three-piece GEMM's aligned operands), else a
    multiple of `align` (the engine's WIDTH_ALIGN). Pads are zero and stay zero."""
    r64 = -(-F // 64) * 64
    return r64 if r64 <= 1.02 * F else -(-F // align) * align


# layer inputs that take no gradient (the features: the same tensor every epoch) keep their
# padded [H | M] buffer: {key: [HM, weakref(h), version, busy]}. A hit needs the SAME tensor
# object (identity through the weak reference, not only its address: a freed input's memory
# is handed to the next same-size allocation, which starts at the same version) with an
# unchanged version. A buffer whose forward saved it for a backward that has not run yet is
# busy (its M half must not be overwritten): another forward then gets a fresh buffer.
_HM_CACHE: dict = {}


def _hm_buffer(h: torch.Tensor, Fp: int, keep: bool):
    """([H | M] (N x 2Fp, H and its zero pad in the left half) for a SAGE layer's input h,
    the cache key it was marked busy under or None)."""
    N, Fin = h.shape
    key = (h.data_ptr(), tuple(h.shape), str(h.device), Fp) if not h.requires_grad else None
    if key is not None:
        hit = _HM_CACHE.get(key)
        if hit is not None and hit[1]() is h and hit[2] == h._version and not hit[3]:
            hit[3] = keep
            return hit[0], (key if keep else None)
    HM = torch.empty(N, 2 * Fp, dtype=torch.float32, device=h.device)
    HM[:, :Fin].copy_(h)
    if Fp > Fin:
        HM[:, Fin:Fp].zero_()
    if key is not None and (key not in _HM_CACHE or not _HM_CACHE[key][3]):
        if len(_HM_CACHE) > 8:
            _HM_CACHE.clear()
        _HM_CACHE[key] = [HM, weakref.ref(h), h._version, keep]
        return HM, (key if keep else None)
    return HM, None


def _hm_release(key) -> None:
    hit = _HM_CACHE.get(key) if key is not None else None
    if hit is not None:
        hit[3] = False


class SagePool(torch.autograd.Function):
    """One DGL 0.8.2 SAGEConv(in, out, 'pool') layer, forward and backward, on the
    engine's kernels (code/model.py:13-15):
        P = relu(h @ Wpool^T + bpool); M = max-aggregate(P); Y = h @ Wself^T + M @ Wneigh^T + b

    On a HIP device it runs TrainEngine's layouts: the input padded to sage_width (503 ->
    512, so the layer-1 products run the three-piece GEMM), fc_self + fc_neigh as ONE
    K = 2F product [H | M] [Wself | Wneigh]^T, dead-none max records (the backward reads no
    relu' mask), the weight gradients of fc_self and fc_neigh as one product dY^T [H | M],
    and the input gradient as one stacked product [dY | dP] [Wself ; Wpool]. On the CPU
    device: the plain composition (DGL's CPU backend role).

    Edge weights that require grad get their gradient from sddmm_dot's max form (dM and P
    over the argmax records); the HIP paths then record plain argmax and apply the relu'
    mask from P. With frozen weights every path makes the calls described above."""

    @staticmethod
    def forward(ctx, h, w_pool, b_pool, w_self, w_neigh, bias, dg, ew_slots):
        h = h.contiguous()
        ctx.dg = dg
        ctx.has_bias = bias is not None
        # a weight gradient needs plain argmax records: a dead-none record drops the entries
        # whose maximum is 0, and an edge with w = 0, P > 0 there has d/dw = dM * P != 0
        ctx.need_ew = ew_slots is not None and ctx.needs_input_grad[7]
        if h.device.type == "cuda":
            return SagePool._forward_gpu(ctx, h, w_pool, b_pool, w_self, w_neigh, bias, dg, ew_slots)
        N, Fin = h.shape
        Fp = round4(Fin)
        Pb = _padded(N, Fin, h.device)
        gemm(h, w_pool, transb=True, out=Pb[:, :Fin], bias=b_pool, act=_lib.PG_ACT_RELU)
        Mb = torch.empty(N, Fp, dtype=torch.float32, device=h.device)
        argpos = torch.empty(N, Fp, dtype=dg.arg_dtype, device=h.device)
        spmm_max(dg, Pb, ew_slots, out=Mb, argpos=argpos)
        Y = gemm(h, w_self, transb=True)
        gemm(Mb[:, :Fin], w_neigh, transb=True, out=Y, beta=1.0, bias=bias)
        ctx.gpu = False
        ctx.save_for_backward(h, w_pool, w_self, w_neigh, Pb, Mb, argpos, ew_slots)
        return Y

    @staticmethod
    def _forward_gpu(ctx, h, w_pool, b_pool, w_self, w_neigh, bias, dg, ew_slots):
        N, Fin = h.shape
        Fp = sage_width(Fin)
        if Fp == Fin:
            out = SagePool._forward_gpu_cat(ctx, h, w_pool, b_pool, w_self, w_neigh, bias, dg, ew_slots)
            if out is not None:
                return out
        ctx.cat = False
        fpad = Fp - Fin
        keep = torch.is_grad_enabled() and (any(ctx.needs_input_grad[:6]) or ctx.need_ew)
        HM, ctx.hm_key = _hm_buffer(h, Fp, keep)
        # the padded weight images in one launch (pg_pad2d_group)
        Fo = w_self.shape[0]
        Wpool = torch.empty(Fp, Fp, dtype=torch.float32, device=h.device)
        bpool = torch.empty(Fp, dtype=torch.float32, device=h.device)
        Wcat = torch.empty(Fo, 2 * Fp, dtype=torch.float32, device=h.device)
        pad2d_group([(w_pool, Wpool), (b_pool.view(1, -1), bpool.view(1, -1)), (w_self, Wcat[:, :Fp]),
                     (w_neigh, Wcat[:, Fp:])])
        P = torch.empty(N, Fp, dtype=torch.float32, device=h.device)
        gemm(HM[:, :Fp], Wpool, transb=True, out=P, bias=bpool, act=_lib.PG_ACT_RELU)
        argpos = torch.empty(N, Fp, dtype=dg.arg_dtype, device=h.device)
        spmm_max(dg, P, ew_slots, out=HM[:, Fp:], argpos=argpos, dead_none=not ctx.need_ew)
        Y = gemm(HM, Wcat, transb=True, bias=bias)
        ctx.gpu = True
        ctx.save_for_backward(HM, P, argpos, Wpool, Wcat, ew_slots)
        ctx.fin = Fin
        return Y

    @staticmethod
    def _forward_gpu_cat(ctx, h, w_pool, b_pool, w_self, w_neigh, bias, dg, ew_slots):
        """A layer whose input needs no padding (4-aligned width): H is the caller's tensor
        and M its own buffer, fc_self + fc_neigh one product over the two K pieces
        ([H | M] [Wself | Wneigh]^T, pg_gemm_f32_cat), no [H | M] copy and no weight
        concatenation; where the library does not take the operands (a misaligned h or
        bias, an odd output width), the same product on the two concatenations, reusing P, M
        and argpos (the aggregation is not redone)."""
        N, Fin = h.shape
        w_pool, w_self, w_neigh = w_pool.contiguous(), w_self.contiguous(), w_neigh.contiguous()
        P = torch.empty(N, Fin, dtype=torch.float32, device=h.device)
        gemm(h, w_pool, transb=True, out=P, bias=b_pool.contiguous(), act=_lib.PG_ACT_RELU)
        M = torch.empty(N, Fin, dtype=torch.float32, device=h.device)
        argpos = torch.empty(N, Fin, dtype=dg.arg_dtype, device=h.device)
        spmm_max(dg, P, ew_slots, out=M, argpos=argpos, dead_none=not ctx.need_ew)
        Y = gemm_cat(h, M, w_self, w_neigh, transb=True, bias=bias)
        if Y is None:
            Y = gemm(torch.cat([h, M], 1), torch.cat([w_self, w_neigh], 1), transb=True, bias=bias)
        ctx.gpu = ctx.cat = True
        ctx.save_for_backward(h, M, P, argpos, w_pool, w_self, w_neigh, ew_slots)
        ctx.fin = Fin
        ctx.hm_key = None
        return Y

    @staticmethod
    def _backward_gpu_cat(ctx, dY):
        h, M, P, argpos, w_pool, w_self, w_neigh, ew_slots = ctx.saved_tensors
        dg, Fin = ctx.dg, ctx.fin
        dY = dY.contiguous()
        N, Fo = dY.shape
        need_h, need_wp, need_bp, need_ws, need_wn, need_b = ctx.needs_input_grad[:6]
        d_b = torch.empty(Fo, dtype=torch.float32, device=dY.device) if (need_b and ctx.has_bias) else None
        wgrads = []  # the layer's weight gradients, one grouped launch after the max backward
        d_ws = torch.empty(Fo, Fin, dtype=torch.float32, device=dY.device) if need_ws else None
        d_wn = torch.empty(Fo, Fin, dtype=torch.float32, device=dY.device) if need_wn else None
        if d_ws is not None:
            wgrads.append((dY, h, d_ws, True, False, 0.0, d_b))
        if d_wn is not None:
            wgrads.append((dY, M, d_wn, True, False, 0.0, d_b if d_ws is None else None))
        if d_b is not None and not wgrads:
            d_b = col_sum(dY)
        dM = gemm(dY, w_neigh)
        dP = torch.empty(N, Fin, dtype=torch.float32, device=dY.device)
        spmm_max_backward(dg, argpos, dM, ew_slots, mask=P, dx=dP, dead_none=not ctx.need_ew)
        d_ew = sddmm_dot(dg, dM, P, argpos=argpos) if ctx.need_ew else None
        d_bp = torch.empty(Fin, dtype=torch.float32, device=dY.device) if need_bp else None
        d_wp = None
        if need_wp:
            d_wp = torch.empty(Fin, Fin, dtype=torch.float32, device=dY.device)
            wgrads.append((dP, h, d_wp, True, False, 0.0, d_bp))
        elif d_bp is not None:
            d_bp = col_sum(dP)
        gemm_group(wgrads)
        d_h = None
        if need_h:  # [dY | dP] [Wself ; Wpool] over the two K pieces
            d_h = gemm_cat(dY, dP, w_self, w_pool)
            if d_h is None:
                d_h = gemm(torch.cat([dY, dP], 1), torch.cat([w_self, w_pool], 0))
        return d_h, d_wp, d_bp, d_ws, d_wn, d_b, None, d_ew

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        if ctx.gpu and ctx.cat:
            return SagePool._backward_gpu_cat(ctx, dY)
        if ctx.gpu:
            return SagePool._backward_gpu(ctx, dY)
        h, w_pool, w_self, w_neigh, Pb, Mb, argpos, ew_slots = ctx.saved_tensors
        dg = ctx.dg
        dY = dY.contiguous()
        N, Fin = h.shape
        need_h, need_wp, need_bp, need_ws, need_wn, need_b = ctx.needs_input_grad[:6]
        d_b = torch.empty(dY.shape[1], dtype=torch.float32, device=dY.device) \
            if (need_b and ctx.has_bias) else None
        d_ws = gemm(dY, h, transa=True, rowsum=d_b) if need_ws else None
        d_wn = gemm(dY, Mb[:, :Fin], transa=True) if need_wn else None
        if d_b is not None and not need_ws:
            d_b = col_sum(dY)
        dMb = _padded(N, Fin, h.device)
        gemm(dY, w_neigh, out=dMb[:, :Fin])
        dPb = torch.empty_like(Pb)
        spmm_max_backward(dg, argpos, dMb, ew_slots, mask=Pb, dx=dPb)
        d_ew = sddmm_dot(dg, dMb, Pb, argpos=argpos) if ctx.need_ew else None
        dP = dPb[:, :Fin]
        d_bp = torch.empty(Fin, dtype=torch.float32, device=dY.device) if need_bp else None
        d_wp = gemm(dP, h, transa=True, rowsum=d_bp) if need_wp else None
        if d_bp is not None and not need_wp:
            d_bp = col_sum(dP)
        d_h = None
        if need_h:
            d_h = gemm(dY, w_self)
            gemm(dP, w_pool, out=d_h, beta=1.0)
        return d_h, d_wp, d_bp, d_ws, d_wn, d_b, None, d_ew

    @staticmethod
    def _backward_gpu(ctx, dY):
        HM, P, argpos, Wpool, Wcat, ew_slots = ctx.saved_tensors
        dg, Fin = ctx.dg, ctx.fin
        try:
            return SagePool._backward_gpu_body(ctx, dY, HM, P, argpos, Wpool, Wcat, ew_slots, dg, Fin)
        finally:
            _hm_release(ctx.hm_key)

    @staticmethod
    def _backward_gpu_body(ctx, dY, HM, P, argpos, Wpool, Wcat, ew_slots, dg, Fin):
        N, Fp = P.shape
        Fo = dY.shape[1]
        need_h, need_wp, need_bp, need_ws, need_wn, need_b = ctx.needs_input_grad[:6]
        # [dY | dP]: dY copied in, dP written by the max backward (only for the stacked
        # input-gradient product: the first layer's input, the features, takes none)
        if need_h:
            DYP = torch.empty(N, Fo + Fp, dtype=torch.float32, device=dY.device)
            DYP[:, :Fo].copy_(dY)
            dY = DYP[:, :Fo]
        else:
            dY = dY.contiguous()
            DYP = None
        d_b = torch.empty(Fo, dtype=torch.float32, device=dY.device) if (need_b and ctx.has_bias) else None
        d_ws = d_wn = None
        wgrads = []  # the layer's weight gradients, one grouped launch after the max backward
        if need_ws or need_wn:
            d_wcat = torch.empty(Fo, 2 * Fp, dtype=torch.float32, device=dY.device)
            wgrads.append((dY, HM, d_wcat, True, False, 0.0, d_b))  # [d Wself | d Wneigh]
            d_ws, d_wn = d_wcat[:, :Fin], d_wcat[:, Fp:Fp + Fin]
        elif d_b is not None:
            d_b = col_sum(dY)
        dM = gemm(dY, Wcat[:, Fp:])
        # dead-none records: the relu' mask of P is implied (P is not read); plain records
        # (a weight gradient is wanted): the mask is applied from P
        dP = DYP[:, Fo:] if DYP is not None else torch.empty(N, Fp, dtype=torch.float32, device=dY.device)
        spmm_max_backward(dg, argpos, dM, ew_slots, mask=P, dx=dP, dead_none=not ctx.need_ew)
        d_ew = sddmm_dot(dg, dM, P, argpos=argpos) if ctx.need_ew else None
        d_bp_p = torch.empty(Fp, dtype=torch.float32, device=dY.device) if need_bp else None
        d_wp = d_bp = None
        if need_wp:
            d_wp_p = torch.empty(Fp, Fp, dtype=torch.float32, device=dY.device)
            wgrads.append((dP, HM[:, :Fp], d_wp_p, True, False, 0.0, d_bp_p))
            d_wp = d_wp_p[:Fin, :Fin]
        elif d_bp_p is not None:
            d_bp_p = col_sum(dP)
        gemm_group(wgrads)
        if d_bp_p is not None:
            d_bp = d_bp_p[:Fin]
        d_h = None
        if need_h:  # one stacked product [dY | dP] [Wself ; Wpool]
            Wstack = torch.cat([Wcat[:, :Fp], Wpool], 0)
            d_h = gemm(DYP, Wstack)[:, :Fin]
        return d_h, d_wp, d_bp, d_ws, d_wn, d_b, None, d_ew
