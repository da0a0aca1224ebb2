"""The max backward on a set of active destination rows (pg_spmm_max_bwd_rows and its bf16
twin) against the plain pg_spmm_max_bwd on a copy of dout whose inactive rows are zero: dx
bitwise equal. In the active-rows call the inactive rows of dout hold NaN and those of
argpos positions past every row's length, so a kernel that read them could not agree.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 2000
BAD_POS = 0x7000  # an argmax position no row of the graph has (and not the "none" 0xFFFF)


def _power_law_coo():
    """Seeded power-law multigraph: destinations and sources drawn with weight 1 / rank, so a
    few destination rows pass the pack's one-wave limit (in-degree > 256) and a few sources
    have hundreds of out-edges; the last 100 nodes never send (no out-edges, no self-loop)."""
    rng = np.random.default_rng(7)
    p = 1.0 / np.arange(1, N + 1)
    ps = p[: N - 100] / p[: N - 100].sum()
    E = 16000
    src = rng.choice(N - 100, E, p=ps)
    dst = rng.permutation(N)[rng.choice(N, E, p=p / p.sum())]
    loops = np.arange(N - 100)
    return (np.concatenate([src, loops]).astype(np.int64), np.concatenate([dst, loops]).astype(np.int64))


_graphs = {}


def _graph(trans, monkeypatch):
    """Source rows split by a backward chunk of 4; descriptors at the in-CSR slots or
    transposed. Built through the module's tuning globals, as bench.py sets them."""
    import plagnn
    import plagnn.graph as pgraph

    if trans not in _graphs:
        monkeypatch.setattr(pgraph, "CHUNK_BWD_OVERRIDE", 4)
        monkeypatch.setattr(pgraph, "TRANS_MIN_EDGES", 0 if trans else 1 << 40)
        src, dst = _power_law_coo()
        g = plagnn.CSRGraph(src, dst, N)
        assert g.bwd_trans == trans and g.bwd.chunk == 4 and g.bwd.n_merges > 300
        assert g.in_degrees().max() > 256 and (g.out_degrees() == 0).sum() >= 100
        _graphs[trans] = g
    return _graphs[trans]


def _bwd(dg, argpos, dout, ews, mask, active=None):
    from plagnn import _lib
    from plagnn._lib import call, ptr

    F = dout.shape[1]
    bf = dout.dtype == torch.bfloat16
    g, gt = dg.fwd.struct(ews), dg.bwd.struct(None)
    ws_n = _lib.lib().pg_spmm_max_bwd_workspace(gt, F)
    ws = torch.empty(max(ws_n, 256), dtype=torch.uint8, device=DEV)
    dx = torch.full((N, F), float("nan"), dtype=dout.dtype, device=DEV)
    kind = dg.arg_kind | _lib.PG_ARG_DEAD_NONE
    head = (g, gt, ptr(argpos), F, kind, ptr(dout), F, F, ptr(mask), F, None, 0, ptr(dx), F)
    tail = (ptr(ws), ws_n, torch.cuda.current_stream().cuda_stream)
    sfx = "_bf16" if bf else ""
    if active is None:
        call("pg_spmm_max_bwd" + sfx, *head, *tail)
    else:
        row_active = active.to(torch.int8)
        eslot_active = torch.where(active[dg.bwd.col.long()], dg.bwd.eslot, torch.full_like(dg.bwd.eslot, -1))
        call("pg_spmm_max_bwd_rows" + sfx, *head, ptr(row_active), ptr(eslot_active), *tail)
    torch.cuda.synchronize()
    return dx


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("F", [64, 256, 504])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_max_bwd_rows_bitwise(F, weighted, trans, dtype, monkeypatch):
    from plagnn import _lib, ops

    g = _graph(trans, monkeypatch)
    dg = g.on(DEV)
    assert dg.arg_kind == _lib.PG_ARG_U16
    rng = np.random.default_rng(F + 2 * weighted)
    ews = torch.from_numpy(rng.uniform(0.5, 2, g.num_edges).astype(np.float32)).to(DEV) if weighted else None
    if ews is not None:
        ews = dg.edge_weight_slots(ews)
    X = np.abs(rng.standard_normal((N, F))).astype(np.float32)  # a relu output: >= 0, 40 % zeros
    X[rng.random((N, F)) < 0.4] = 0.0
    X = torch.from_numpy(X).to(DEV, dtype)
    _, argpos = ops.spmm_max(dg, X, ews, dead_none=True)
    dout = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(DEV, dtype)
    plain = _bwd(dg, argpos, dout, ews, X)

    for frac in (0.4, 1.0, 0.0):
        active = torch.from_numpy(rng.random(N) < frac).to(DEV)
        if frac == 0.4:  # both kinds of row among the long ones (one workgroup per row)
            long_rows = np.flatnonzero(g.in_degrees() > 256)
            assert len(long_rows) >= 2
            active[int(long_rows[0])] = True
            active[int(long_rows[1])] = False
        zeroed = torch.where(active[:, None], dout, torch.zeros_like(dout))
        ref = plain if frac == 1.0 else _bwd(dg, argpos, zeroed, ews, X)
        poisoned = torch.where(active[:, None], dout, torch.full_like(dout, float("nan")))
        bad_arg = torch.where(active[:, None], argpos, torch.full_like(argpos, BAD_POS))
        dx = _bwd(dg, bad_arg, poisoned, ews, X, active)
        dx2 = _bwd(dg, bad_arg, poisoned, ews, X, active)
        assert torch.equal(_bits(dx), _bits(ref)), f"active fraction {frac}"
        assert torch.equal(_bits(dx), _bits(dx2)), f"two calls differ, active fraction {frac}"
        if frac == 0.0:
            assert not _bits(dx).any()  # every element +0


def test_max_bwd_rows_arguments(monkeypatch):
    """Both arrays NULL is the plain call; one alone is an argument error."""
    from plagnn import _lib, ops
    from plagnn._lib import ptr

    g = _graph(False, monkeypatch)
    dg = g.on(DEV)
    F = 64
    rng = np.random.default_rng(1)
    X = torch.from_numpy(np.abs(rng.standard_normal((N, F))).astype(np.float32)).to(DEV)
    _, argpos = ops.spmm_max(dg, X, None, dead_none=True)
    dout = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32)).to(DEV)
    plain = _bwd(dg, argpos, dout, None, X)
    gs, gt = dg.fwd.struct(None), dg.bwd.struct(None)
    ws_n = _lib.lib().pg_spmm_max_bwd_workspace(gt, F)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(dout)
    st = torch.cuda.current_stream().cuda_stream
    head = (gs, gt, ptr(argpos), F, dg.arg_kind | _lib.PG_ARG_DEAD_NONE, ptr(dout), F, F, ptr(X), F, None, 0, ptr(dx), F)
    assert _lib.lib().pg_spmm_max_bwd_rows(*head, None, None, ptr(ws), ws_n, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(dx), _bits(plain))
    flags = torch.ones(N, dtype=torch.int8, device=DEV)
    assert _lib.lib().pg_spmm_max_bwd_rows(*head, ptr(flags), None, ptr(ws), ws_n, st) == -1  # PG_ERR_INVALID
