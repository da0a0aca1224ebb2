"""One case per dispatch leaf of the three GEMM families (csrc/gemm.hip, gemm_x3.hip,
gemm_bf16.hip): every tile each pick rule can return, every (transa, transb), every fused
epilogue, the loader forms, split-K, the K-concatenated and row-list forms and the grouped
launches, each at the smallest shape that selects it. A kernel the dispatch can reach and
that was not built, or a dispatch that lands on another kernel than the rule names, fails
here (PG_ERR_INVALID, or a changed digest in the listing below).

Bars (float64 references, the ones tests/test_gpu_kernels.py and test_gpu_bf16.py use):
  f32 entry points   |C - ref| <= 1e-6 sum_k |a b|
  bf16 entry point   |C - ref| <= 2e-6 sqrt(K) sum_k |a b|, + 2^-8 |ref| for a bf16 output
  fused epilogues    the same bars, nothing added (bias, beta = 1 and the activations
                     included); the reference's slope is the float32 nearest 0.01, as in the
                     kernels.
  row sums           f32: 2e-7 sqrt(slices) ||row||_2 + 2e-7 |sum| (float64 accumulation, one
                     float32 rounding per slice); bf16: 2e-6 sqrt(K) sum_k |a|

How each shape selects its tile (tiles(bm, bn) = ceil(M / bm) ceil(N / bn)):
  f32 MFMA kernels, pick_tile (reached by writing C through a view with ldc = N + 1, which
  the three-piece kernel does not take; split products by an operand or workspace 4 B off):
    (70, 68, 40)       N <= 128                                            -> 64 x 64
    (30700, 132, 36)   128 < N <= 512, K <= 1024, tiles(128, 64) = 240 * 3 = 720 >= 720
                                                                           -> 128 x 64
    (70, 516, 36)      N > 512, tiles(128, 128) = 1 * 5 < 768              -> 64 x 128
    (19585, 516, 36)   N > 512, tiles(128, 128) = 154 * 5 = 770 >= 768     -> 128 x 128
    split              always kSplitBM x kSplitBN                          -> 64 x 64
  three-piece kernels, pick_tile_x3:
    (72, 68, 40)       tiles(128, 128) = 1, tiles(128, 64) = 2             -> 64 x 64
    (32644, 68, 36)    tiles(128, 128) = 256 < 512, tiles(128, 64) = 256 * 2 = 512
                                                                           -> 128 x 64
    (21764, 260, 36)   tiles(128, 128) = 171 * 3 = 513 >= 512              -> 128 x 128
    split              bm = M > 64 ? 128 : 64, bn = N > 64 ? 128 : 64: M, N in {40, 72}
                       give the four tiles
  bf16 kernels, pick_tile:
    (72, 72, 72)       tiles(128, 64) = 2                                  -> 64 x 64
    (65416, 64, 72)    N <= 64, tiles(128, 64) = 512 * 1 >= 512            -> 128 x 64
    (21768, 264, 72)   K < 384, N > 64, tiles(128, 128) = 171 * 3 = 513    -> 128 x 128
    (32520, 264, 392)  N >= 256, K >= 384, tiles(256, 256) = 128 * 2 = 256 -> 256 x 256
                       (A B^T without row sums: the ping-pong kernel; otherwise the generic one)
    split              M, N >= 256 -> 256 x 256 (264, 264), else 64 x 64 (72, 72)

`python tests/test_gpu_gemm_paths.py` prints `case-id sha256(output bytes)` for every case:
two builds that run the same kernels on the same slices in the same order print the same
listing. The whole file (103 cases) takes about 5 s on an MI355X.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = float(np.float32(0.01))
TT = [(False, False), (False, True), (True, False), (True, True)]
EPIS = ["none", "relu", "leaky", "drelu", "dleaky"]


def _tt(ta, tb):
    return ("t" if ta else "n") + ("t" if tb else "n")


# ------------------------------------------------------------------ inputs and references
_cache = {}


def _data(fam, M, N, K):
    """op(A) (M x K), op(B) (K x N) from default_rng(shape), their float64 product and
    sum |a b|; bf16 families round the operands first. One shape is kept (cases are ordered
    by shape)."""
    key = (fam == "bf16", M, N, K)
    if key not in _cache:
        _cache.clear()
        rng = np.random.default_rng(M * 1000003 + N * 1009 + K)
        a = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal((K, N)).astype(np.float32))
        extra = torch.from_numpy(rng.standard_normal((M + 1, N)).astype(np.float32))  # C0 / dact, bias
        if fam == "bf16":
            a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
        a64, b64 = a.double(), b.double()
        _cache[key] = (a, b, extra, a64 @ b64, a64.abs() @ b64.abs())
    return _cache[key]


def _dev(t, off=0):
    """Device copy of t; off = 1 puts it one element past a 16-B boundary."""
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _operands(a, b, ta, tb, offa=0, offb=0):
    return _dev(a.t().contiguous() if ta else a, offa), _dev(b.t().contiguous() if tb else b, offb)


def _epilogue(epi, M, N, extra, bf16):
    """(bias, dact, C0, act, reference transform) of a fused epilogue."""
    from plagnn import _lib

    bias = extra[M] if epi in ("relu", "leaky") else None
    y = extra[:M] if epi in ("drelu", "dleaky") else None
    c0 = extra[:M].flip(0).contiguous() if epi == "dleaky" else None  # beta = 1 with the fused leaky'
    act = {"none": _lib.PG_ACT_NONE, "relu": _lib.PG_ACT_RELU, "drelu": _lib.PG_ACT_RELU}.get(epi, _lib.PG_ACT_LEAKY)
    if bf16 and y is not None:
        y = y.to(torch.bfloat16)

    def ref_fn(r):
        if c0 is not None:
            r = r + c0.double()
        if bias is not None:
            r = r + bias.double()
        if epi == "relu":
            return r.clamp_min(0)
        if epi == "leaky":
            return torch.where(r > 0, r, r * SLOPE)
        if epi == "drelu":
            return torch.where(y.double() > 0, r, torch.zeros_like(r))
        if epi == "dleaky":
            return torch.where(y.double() > 0, r, r * SLOPE)
        return r

    return bias, y, c0, act, ref_fn


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ runners: -> (outputs, check)
def _run_f32(M, N, K, ta, tb, epi="none", split_k=1, ldc_pad=0, offa=0, offb=0, ws_off=0):
    """pg_gemm_f32. ldc_pad = 1, offa / offb = 1 or ws_off = 4 take the three-piece path
    away (x3_ok: 16-B aligned operands, ldc % 4 == 0, a 16-B aligned workspace)."""
    from plagnn import _lib
    from plagnn._lib import call, ptr

    a, b, extra, ref, mag = _data("f32", M, N, K)
    A, B = _operands(a, b, ta, tb, offa, offb)
    bias, y, c0, act, ref_fn = _epilogue(epi, M, N, extra, False)
    buf = torch.full((M, N + ldc_pad), float("nan"), device=DEV)
    C = buf[:, :N]
    if c0 is not None:
        C.copy_(c0)
    bias_d, y_d = (None if bias is None else _dev(bias)), (None if y is None else _dev(y))
    rs = torch.full((M,), float("nan"), device=DEV) if split_k > 1 else None
    ws_n = int(_lib.lib().pg_gemm_f32_workspace(M, N, K, split_k))
    ws = torch.empty(ws_n + 16, dtype=torch.uint8, device=DEV)
    ep = _lib.epilogue(bias_d, act, SLOPE, y_d, rs)
    call("pg_gemm_f32", int(ta), int(tb), M, N, K, 1.0, ptr(A), A.stride(0), ptr(B), B.stride(0),
         1.0 if c0 is not None else 0.0, ptr(C), C.stride(0), ep, split_k, ptr(ws) + ws_off, ws_n, _stream())
    torch.cuda.synchronize()

    def check():
        got = C.cpu().double()
        assert bool(((got - ref_fn(ref)).abs() <= 1e-6 * mag).all())
        if ldc_pad:
            assert bool(torch.isnan(buf[:, N:]).all())
        if rs is not None:
            a64 = a.double()
            rs64 = a64.sum(1)
            bound = 2e-7 * split_k ** 0.5 * a64.pow(2).sum(1).sqrt() + 2e-7 * rs64.abs()
            assert bool(((rs.cpu().double() - rs64).abs() <= bound).all())

    return [C] + ([rs] if rs is not None else []), check


def _run_cat(M, N, K, tb, epi):
    """pg_gemm_f32_cat: K split at K1 = 24 (a 16-k step straddles it)."""
    from plagnn import _lib
    from plagnn._lib import call, ptr

    a, b, extra, ref, mag = _data("f32", M, N, K)
    K1 = 24
    A1, A2 = _dev(a[:, :K1].contiguous()), _dev(a[:, K1:].contiguous())
    B1 = _dev(b[:K1].t().contiguous() if tb else b[:K1].contiguous())
    B2 = _dev(b[K1:].t().contiguous() if tb else b[K1:].contiguous())
    bias, _, _, act, ref_fn = _epilogue(epi, M, N, extra, False)
    C = torch.full((M, N), float("nan"), device=DEV)
    ep = _lib.epilogue(None if bias is None else _dev(bias), act, SLOPE)
    call("pg_gemm_f32_cat", int(tb), M, N, K1, K - K1, 1.0, ptr(A1), A1.stride(0), ptr(A2), A2.stride(0), ptr(B1),
         B1.stride(0), ptr(B2), B2.stride(0), 0.0, ptr(C), C.stride(0), ep, _stream())
    torch.cuda.synchronize()

    def check():
        assert bool(((C.cpu().double() - ref_fn(ref)).abs() <= 1e-6 * mag).all())

    return [C], check


def _run_rows(M, N, K, tb):
    """pg_gemm_f32_rows: the M listed rows (they select the tile) of an A of M + 9 rows."""
    from plagnn import _lib
    from plagnn._lib import call, ptr

    a, b, extra, ref, mag = _data("f32", M, N, K)
    m_full = M + 9
    rng = np.random.default_rng(M + N)
    rows = np.sort(rng.choice(m_full, M, replace=False)).astype(np.int32)
    full = torch.zeros(m_full, K)
    full[torch.from_numpy(rows).long()] = a
    A, B = _operands(full, b, False, tb)
    rows_d = torch.from_numpy(rows).to(DEV)
    C = torch.full((m_full, N), float("nan"), device=DEV)
    call("pg_gemm_f32_rows", int(tb), m_full, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.stride(0),
         ptr(rows_d), M, _stream())
    torch.cuda.synchronize()

    def check():
        got = C.cpu()
        listed = torch.zeros(m_full, dtype=torch.bool)
        listed[torch.from_numpy(rows).long()] = True
        assert bool(((got[listed].double() - ref).abs() <= 1e-6 * mag).all())
        assert bool(torch.isnan(got[~listed]).all())

    return [C], check


_GROUP_SHAPES = {"f32": [(72, 68, 400), (40, 132, 300), (260, 72, 500)],
                 # (264, 264) and (264, 520) are members of the bf16 group (256 x 256 tiles waste
                 # < 4x their area), (72, 72) runs alone after it
                 "bf16": [(264, 264, 400), (264, 520, 600), (72, 72, 400)]}


def _run_group(fam, ta, tb):
    from plagnn import _lib
    from plagnn._lib import call, ptr

    shapes = _GROUP_SHAPES[fam]
    parts = (_lib.PgGemmPart * len(shapes))()
    keep = []
    for i, (q, (M, N, K)) in enumerate(zip(parts, shapes)):
        rng = np.random.default_rng(M * 1000003 + N * 1009 + K + 17)
        a = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32))
        b = torch.from_numpy(rng.standard_normal((K, N)).astype(np.float32))
        c0 = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32))
        if fam == "bf16":
            a, b = a.to(torch.bfloat16), b.to(torch.bfloat16)
        A, B = _operands(a, b, ta, tb)
        beta = 1.0 if i == 1 else 0.0
        C, rs = _dev(c0), torch.full((M,), float("nan"), device=DEV)
        q.transa, q.transb, q.M, q.N, q.K = int(ta), int(tb), M, N, K
        q.A, q.lda, q.B, q.ldb = ptr(A), A.stride(0), ptr(B), B.stride(0)
        q.beta, q.C, q.ldc, q.rowsum = beta, ptr(C), C.stride(0), ptr(rs)
        keep.append((a, b, c0, beta, A, B, C, rs))
    n = len(shapes)
    L = _lib.lib()
    ws_n = int((L.pg_gemm_f32_group_workspace if fam == "f32" else L.pg_gemm_bf16_group_workspace)(parts, n))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    call(f"pg_gemm_{fam}_group", parts, n, ptr(ws), ws_n, _stream())
    torch.cuda.synchronize()

    def check():
        for (a, b, c0, beta, _, _, C, rs) in keep:
            a64, b64 = a.double(), b.double()
            K = a.shape[1]
            ref, mag = a64 @ b64 + beta * c0.double(), a64.abs() @ b64.abs()
            rs64 = a64.sum(1)
            if fam == "f32":
                bound = 1e-6 * mag
                rs_bound = 2e-7 * 256 ** 0.5 * a64.pow(2).sum(1).sqrt() + 2e-7 * rs64.abs()
            else:
                bound = 2e-6 * np.sqrt(K) * mag
                rs_bound = 2e-6 * np.sqrt(K) * a64.abs().sum(1)
            assert bool(((C.cpu().double() - ref).abs() <= bound).all())
            assert bool(((rs.cpu().double() - rs64).abs() <= rs_bound).all())

    return [t for k in keep for t in (k[6], k[7])], check


def _run_bf16(M, N, K, ta, tb, epi="none", obf=False, split_k=1, rowsum=False):
    from plagnn import _lib
    from plagnn._lib import call, ptr

    a, b, extra, ref, mag = _data("bf16", M, N, K)
    A, B = _operands(a, b, ta, tb)
    if obf:  # a bf16 C holds bf16 values before the call too
        extra = extra.to(torch.bfloat16).float()
    bias, y, c0, act, ref_fn = _epilogue(epi, M, N, extra, True)
    C =torch.full((M, N), float("nan"), dtype=torch.bfloat16 if obf else torch.float32, device=DEV)
    if c0 is not None:
        C.copy_(c0)
    bias_d, y_d = (None if bias is None else _dev(bias)), (None if y is None else _dev(y))
    rs = torch.full((M,), float("nan"), device=DEV) if rowsum else None
    ws_n = int(_lib.lib().pg_gemm_bf16_workspace(M, N, K, split_k))
    ws = torch.empty(max(ws_n, 16), dtype=torch.uint8, device=DEV)
    ep = _lib.epilogue(bias_d, act, SLOPE, y_d, rs)
    call("pg_gemm_bf16", int(ta), int(tb), M, N, K, 1.0, ptr(A), A.stride(0), ptr(B), B.stride(0),
         1.0 if c0 is not None else 0.0, ptr(C), C.stride(0), _lib.PG_DTYPE_BF16 if obf else _lib.PG_DTYPE_F32, ep,
         split_k, ptr(ws), ws_n, _stream())
    torch.cuda.synchronize()

    def check():
        r = ref_fn(ref)
        bound = 2e-6 * np.sqrt(K) * mag + 1e-30
        if obf:
            bound = bound + 2.0 ** -8 * r.abs()
        assert bool(((C.cpu().double() - r).abs() <= bound).all())
        if rs is not None:
            a64 = a.double()
            assert bool(((rs.cpu().double() - a64.sum(1)).abs() <= 2e-6 * np.sqrt(K) * a64.abs().sum(1)).all())

    return [C] + ([rs] if rs is not None else []), check


# ------------------------------------------------------------------ the cases
F32_TILES = [("64x64", (70, 68, 40)), ("128x64", (30700, 132, 36)), ("64x128", (70, 516, 36)),
             ("128x128", (19585, 516, 36))]
X3_TILES = [("64x64", (72, 68, 40)), ("128x64", (32644, 68, 36)), ("128x128", (21764, 260, 36))]
BF16_TILES = [("64x64", (72, 72, 72)), ("128x64", (65416, 64, 72)), ("128x128", (21768, 264, 72)),
              ("256x256", (32520, 264, 392))]


def _cases():
    """(id, runner, kwargs), ordered so that consecutive cases share a shape."""
    out = []

    def add(cid, fn, **kw):
        out.append((cid, fn, kw))

    # f32 MFMA kernels: all five epilogues on 64 x 64, one (rotated) on each other tile
    for e in EPIS:
        add(f"f32-64x64-{e}", _run_f32, M=70, N=68, K=40, ta=False, tb=False, epi=e, ldc_pad=1)
    # split products: A 4 B off (register loader for A), and a workspace 4 B off (LDS-DMA kernel)
    add("f32-split-offa", _run_f32, M=70, N=68, K=300, ta=False, tb=False, split_k=3, offa=1)
    add("f32-split-wsoff", _run_f32, M=70, N=68, K=300, ta=False, tb=False, split_k=3, ws_off=4)
    for (name, (M, N, K)), e in zip(F32_TILES[1:], EPIS[1:]):
        add(f"f32-{name}-{e}", _run_f32, M=M, N=N, K=K, ta=False, tb=False, epi=e, ldc_pad=1)
    # every transposition x the four loader forms (va, vb: 16-B loads of A / of B), 64 x 64
    for ta, tb in TT:
        for offa in (0, 1):
            for offb in (0, 1):
                add(f"f32-{_tt(ta, tb)}-va{1 - offa}-vb{1 - offb}", _run_f32, M=72, N=68, K=40, ta=ta, tb=tb,
                    ldc_pad=1, offa=offa, offb=offb)
    # three-piece kernels
    for ta, tb in TT:
        add(f"x3-64x64-{_tt(ta, tb)}", _run_f32, M=72, N=68, K=40, ta=ta, tb=tb)
    for e in EPIS[1:]:
        add(f"x3-64x64-{e}", _run_f32, M=72, N=68, K=40, ta=False, tb=False, epi=e)
    for tb in (False, True):
        for e in ("none", "leaky"):
            add(f"x3-cat-64x64-{_tt(False, tb)}-{e}", _run_cat, M=72, N=68, K=40, tb=tb, epi=e)
        add(f"x3-rows-64x64-{_tt(False, tb)}", _run_rows, M=72, N=68, K=40, tb=tb)
    for (name, (M, N, K)), e in zip(X3_TILES[1:], EPIS[1:]):
        add(f"x3-{name}-{e}", _run_f32, M=M, N=N, K=K, ta=False, tb=False, epi=e)
        for tb in (False, True):
            for ce in ("none", "leaky"):
                add(f"x3-cat-{name}-{_tt(False, tb)}-{ce}", _run_cat, M=M, N=N, K=K, tb=tb, epi=ce)
            add(f"x3-rows-{name}-{_tt(False, tb)}", _run_rows, M=M, N=N, K=K, tb=tb)
    for M in (40, 72):
        for N in (40, 72):
            for ta, tb in TT:
                add(f"x3-split-{M}x{N}-{_tt(ta, tb)}", _run_f32, M=M, N=N, K=400, ta=ta, tb=tb, split_k=3)
    for ta, tb in TT:
        add(f"x3-group-{_tt(ta, tb)}", _run_group, fam="f32", ta=ta, tb=tb)
    # bf16 kernels
    for ta, tb in TT:
        for obf in (False, True):
            add(f"bf16-64x64-{_tt(ta, tb)}-{'bf16' if obf else 'f32'}", _run_bf16, M=72, N=72, K=72, ta=ta, tb=tb,
                obf=obf)
    for e in EPIS[1:]:
        add(f"bf16-64x64-{e}", _run_bf16, M=72, N=72, K=72, ta=False, tb=False, epi=e, obf=e in ("relu", "dleaky"))
    for (name, (M, N, K)), e in zip(BF16_TILES[1:], EPIS[1:]):
        add(f"bf16-{name}-{e}", _run_bf16, M=M, N=N, K=K, ta=True, tb=False, epi=e, obf=e == "leaky")
    M, N, K = BF16_TILES[3][1]
    add("bf16-256x256-nt-pingpong", _run_bf16, M=M, N=N, K=K, ta=False, tb=True)
    add("bf16-256x256-nt-rowsum", _run_bf16, M=M, N=N, K=K, ta=False, tb=True, rowsum=True)
    for M in (264, 72):
        for ta, tb in TT:
            add(f"bf16-split-{M}-{_tt(ta, tb)}", _run_bf16, M=M, N=M, K=400, ta=ta, tb=tb, split_k=3, rowsum=True)
    for ta, tb in TT:
        add(f"bf16-group-{_tt(ta, tb)}", _run_group, fam="bf16", ta=ta, tb=tb)
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_path(case):
    _, fn, kw = case
    _, check = fn(**kw)
    check()


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "pla-gnn_amd"))
    for cid, fn, kw in CASES:
        outs, _ = fn(**kw)
        print(cid, _sha(*outs), flush=True)
