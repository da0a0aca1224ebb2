"""One case per host branch of the max forward / backward dispatch (launch_max_fwd,
max_bwd_entry, launch_max_bwd): values and positions of pg_spmm_max_fwd, and dx of
pg_spmm_max_bwd, bitwise against the host twins pg_spmm_max_fwd_cpu / pg_spmm_max_bwd_cpu.

The graph is the ladder graph of sum_common at a forward chunk of 4: its in-degrees sit on
every gather, window, chunk and merge boundary, nearly every row is split, and the
out-degrees pass the backward chunk, so every case below runs with split rows.

Operands are small integers (30 % zeros, so most maxima are ties and the earliest maximal
edge must win) and weights from {-1, 0.5, 1, 2}: every product is exact in f32 and in bf16,
so bf16 storage gives the f32 twin's values rounded (exactly) to bf16. The backward's sums of
such terms are exact in f32 in any order (|term| <= 8, at most a few thousand terms, steps
of 0.5), so the twin's sequential order and the schedule's piecewise order give the same
bits on split rows too, while a dropped, doubled or misplaced term changes the value.

Branches (F is the smallest width that reaches each; f32 widths, bf16 where it differs):
  forward, scalar path, split rows through the max_merge_kernel launch: F = 65; F = 256 with
    X one element off a 16-byte boundary;
  forward, vector whole-row path with two feature tiles: F = 300 with the workspace 16 B off
    a 256-byte boundary (no tickets: the merge is a launch of its own) and aligned (the
    in-launch combine);
  forward, slice path: F = 256 weighted and unweighted (fewer than 8 slices: 8 pieces in
    flight), F = 512 unweighted (8 slices: 4 in flight; bf16: F = 1024), F = 400 (f32: 7
    slices of 64 columns do not share out, 4 of 128 do);
  each of these with u16 and i32 records and with f32 and bf16 storage;
  backward, grouped path with descriptors at the in-CSR slots and transposed (g->epos):
    F = 65 (scalar pack, merge launch), F = 260 (two-chunk vector pack, in-pull combine),
    F = 1024 (four chunks), f32 and bf16 (4-byte records unweighted, 8-byte weighted);
  backward, launch_max_bwd (i32 records): F = 260 (vector, a 256 and a 4 column tile) and
    F = 65 (scalar);
  backward on active rows (pg_spmm_max_bwd_rows) with a hub row inactive.
No case is left to test_gpu_kernels.py: the shapes here are small enough to run them all.
"""
import numpy as np
import pytest
import torch

from max_common import case as _case, graph as _graph, same as _same

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a, dtype=torch.float32, offset=False):
    """numpy -> device tensor of `dtype`; offset: the base pointer one element past a 16-byte
    boundary (a contiguous view of a longer buffer)."""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(DEV)
    if t.dtype == torch.float32 and t.dim() == 2:
        t = t.to(dtype)
    if offset:
        flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = flat[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == t.element_size()
        t = v
    return t


def _offset_workspace(monkeypatch, off=16):
    """ops' scratch buffer `off` bytes past an allocation's (256-byte aligned) start."""
    from plagnn import ops

    def ws(nbytes, device):
        if nbytes <= 0:
            return None
        buf = torch.empty(int(nbytes) + off, dtype=torch.uint8, device=device)[off:]
        assert buf.data_ptr() % 256 == off
        return buf

    monkeypatch.setattr(ops, "_workspace", ws)


FWD_CASES = [
    # id, F (f32), F (bf16), weighted, X offset, workspace offset
    ("scalar", 65, 65, True, False, False),
    ("scalar_x_offset", 256, 256, False, True, False),
    ("whole_row_merge_launch", 300, 300, True, False, True),
    ("whole_row_in_launch", 300, 300, False, False, False),
    ("slices_weighted", 256, 256, True, False, False),
    ("slices_u8", 256, 256, False, False, False),
    ("slices_u4", 512, 1024, False, False, False),
    ("slices_doubled", 400, 400, False, False, False),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("i32", [False, True], ids=["u16", "i32"])
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_max_fwd_branch(case, i32, dtype, monkeypatch):
    from plagnn import ops

    name, F32, F16, weighted, x_off, ws_off = case
    F = F16 if dtype == torch.bfloat16 else F32
    X, w, out_ref, arg_ref, *_ = _case(F, weighted, i32)
    dg = _graph(False, i32).on(DEV)
    assert dg.arg_dtype == (torch.int32 if i32 else torch.int16)
    if ws_off:
        _offset_workspace(monkeypatch)
    Xd, wd = _dev(X, dtype, offset=x_off), _dev(w)
    out, arg = ops.spmm_max(dg, Xd, wd)
    out2, arg2 = ops.spmm_max(dg, Xd, wd)  # (the split rows' tickets restart every call)
    torch.cuda.synchronize()
    assert out.dtype == dtype
    _same(out, out_ref, f"{name}: values")
    assert np.array_equal(arg.cpu().numpy(), arg_ref), f"{name}: positions"
    assert torch.equal(out, out2) and torch.equal(arg, arg2), f"{name}: second call"


def _bwd_case(F, weighted, trans, i32, dtype):
    from plagnn import ops

    X, w, _, arg, dout, dx_ref, dxm_ref = _case(F, weighted, i32)
    dg = _graph(trans, i32).on(DEV)
    argd, dd, wd, Xd = _dev(arg), _dev(dout, dtype), _dev(w), _dev(X, dtype)
    name = f"F={F} weighted={weighted} trans={trans} i32={i32} {dtype}"
    dx = ops.spmm_max_backward(dg, argd, dd, wd)
    dx2 = ops.spmm_max_backward(dg, argd, dd, wd)
    dxm = ops.spmm_max_backward(dg, argd, dd, wd, mask=Xd)
    torch.cuda.synchronize()
    assert dx.dtype == dtype
    _same(dx, dx_ref, name)
    _same(dxm, dxm_ref, name + ": relu' mask")
    assert torch.equal(dx, dx2), name + ": second call"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("trans", [False, True], ids=["slots", "epos"])
@pytest.mark.parametrize("F,weighted", [(65, False), (65, True), (260, False), (260, True), (1024, False)])
def test_max_bwd_grouped(F, weighted, trans, dtype):
    _bwd_case(F, weighted, trans, False, dtype)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("F", [260, 65])
def test_max_bwd_record_gather(F, weighted):
    _bwd_case(F, weighted, False, True, torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("trans", [False, True], ids=["slots", "epos"])
def test_max_bwd_rows_hub_inactive(trans, dtype):
    """pg_spmm_max_bwd_rows with the longest destination row and every third row inactive:
    their dout rows hold NaN in the call and count as zero in the twin."""
    from plagnn import _lib, ops
    from plagnn._lib import call, ptr

    F, weighted = 260, True
    X, w, _, arg, dout, *_ = _case(F, weighted, False)
    g = _graph(trans, False)
    dg, cg = g.on(DEV), g.on("cpu")
    active = np.ones(g.num_dst, bool)
    active[::3] = False
    hub = int(np.argmax(g.in_degrees()))
    active[hub] = False
    assert g.in_degrees()[hub] == 129 and active.sum() > g.num_dst // 2
    zeroed = np.where(active[:, None], dout, np.float32(0))
    dx_ref = ops.spmm_max_backward(cg, torch.from_numpy(np.array(arg)), torch.from_numpy(zeroed),
                                   torch.from_numpy(np.array(w))).numpy()
    act = torch.from_numpy(active).to(DEV)
    dd = _dev(np.where(active[:, None], dout, np.float32("nan")), dtype)
    argd, wd = _dev(arg), _dev(w)
    row_active = act.to(torch.int8)
    eslot_active = torch.where(act[dg.bwd.col.long()], dg.bwd.eslot, torch.full_like(dg.bwd.eslot, -1))
    fs, gt = dg.fwd.struct(wd), dg.bwd.struct(None)
    ws_n = _lib.lib().pg_spmm_max_bwd_workspace(gt, F)
    ws = torch.empty(max(ws_n, 256), dtype=torch.uint8, device=DEV)
    dx = torch.full((g.num_src, F), float("nan"), dtype=dtype, device=DEV)
    call("pg_spmm_max_bwd_rows" + ("_bf16" if dtype == torch.bfloat16 else ""), fs, gt, ptr(argd), F, dg.arg_kind,
         ptr(dd), F, F, None, 0, None, 0, ptr(dx), F, ptr(row_active), ptr(eslot_active), ptr(ws), ws_n,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(dx, dx_ref, f"active rows trans={trans} {dtype}")
