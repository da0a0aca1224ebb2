"""Leading dimensions and base pointers of the max family at its C-ABI: pg_spmm_max_fwd,
pg_spmm_max_bwd, pg_spmm_max_bwd_rows, their _bf16 forms, pg_spmm_max_bwd_scatter and
pg_argpos_to_src, every operand a window of a padded buffer (max_common.window), bitwise
against the host twins on contiguous operands. test_gpu_max_paths.py holds the widths, record
kinds and schedule branches on contiguous tensors; here the same kernels get what the host
dispatch decides on: include/plagnn.h states the contract, max_common.predict_* restates it
and test_max_strides_cpu.py checks the tables below against it.

After every call: the F columns equal the twin, everything outside them (pad columns, the
elements before and after the rows) keeps its sentinel, and a second call into fresh buffers
gives the same bits. X pads hold 2^100, dout / mask / fwd_out pads NaN, out and dx NaN before
the call, argpos 0x7F7F.. before the forward; a pad value that is read changes a result.

Predicates and the cases that reach each branch (graph: the ladder graph at chunk 4, about
150 nodes, hub in-degree 129; rows split in both directions). Baseline: every operand in a
window with its own 4-multiple pad (F + 4, F + 8, ...: a swapped pair of leading dimensions
shows), bases aligned.
  launch_max_fwd, vector needs F, ldx, ldo, lda % 4, X / out / ws 16-byte aligned, argpos
  aligned to 4 records:
    baseline F = 256: slice kernel; F = 300: whole rows, two tiles, in-launch combine;
    ws16 F = 300: whole rows, split rows by max_merge_kernel's launch;
    ldx_odd, ldo_odd, lda_odd, x_off1, out_off1, arg_off1, arg_off2 (i32 records: 8 bytes is
    not enough): max_fwd_kernel<W = 1> and max_merge_kernel; arg_off4 (u16: 8 bytes is
    enough): the baseline's vector path;
    tiles_flat F = 1027, tiles_ldx F = 1100: the scalar kernels in two 1024-column tiles.
  max_bwd_entry at F = 260, descriptors at the slots and transposed, weighted and not (bf16
  unweighted: 4-byte records), modes mask / mask with fwd_out / dead-none records:
    baseline, ws16: vector pack, in-pull merge;
    lda_odd, ldd_odd, ldf_odd, arg_off1, dout_off1, fout_off1: group_pack_kernel<NV = 0>
    with the in-pull merge;
    ldx_odd, dx_off1, ldm_odd, mask_off1: vector pack, the pull's slot stores and
    sum_merge_kernel's launch (dead-none: the mask is not read, its buffer holds NaN, and the
    two mask terms stay on the in-pull merge);
    both: scalar pack and launch merge; F = 1024: four chunks, baseline and ldx_odd.
  pg_spmm_max_bwd_rows: hub row and every third row inactive (NaN dout rows): baseline,
    ldd_odd, ldx_odd.
  launch_max_bwd (i32 records, f32): baseline F = 260 (vector, 256 + 4 columns); lda, ldd, ldx,
    ldm odd: max_bwd_kernel<W = 1> and scalar sum_merge_kernel; F = 1100 ldd_odd: two launches.
  pg_spmm_max_bwd_scatter, pg_argpos_to_src: element accesses only; odd, distinct pads and
    offset bases.
Rejections: every leading dimension one below F and a backward workspace 4 bytes off give
PG_ERR_INVALID and leave the output buffers' sentinels.
"""
import pytest
import torch

import max_common as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = r"\(code -1\)"


@pytest.mark.parametrize("case", mc.FWD_CASES, ids=[c[0] for c in mc.FWD_CASES])
def test_max_fwd_windows(case):
    name, F, dt, kind, weighted, spec, _ = case
    mc.run_fwd(DEV, F, dt, kind, weighted, spec, name)


@pytest.mark.parametrize("case", mc.BWD_CASES, ids=[c[0] for c in mc.BWD_CASES])
def test_max_bwd_grouped_windows(case):
    name, F, dt, trans, weighted, mode, spec, _ = case
    mc.run_bwd(DEV, F, dt, trans, weighted, mode, spec, name)


@pytest.mark.parametrize("case", mc.ROWS_CASES, ids=[c[0] for c in mc.ROWS_CASES])
def test_max_bwd_rows_windows(case):
    name, F, dt, trans, weighted, mode, spec, _ = case
    mc.run_bwd(DEV, F, dt, trans, weighted, mode, spec, name, rows=True)


@pytest.mark.parametrize("case", mc.GATHER_CASES, ids=[c[0] for c in mc.GATHER_CASES])
def test_max_bwd_record_gather_windows(case):
    name, F, weighted, spec, _ = case
    mc.run_bwd(DEV, F, "f32", False, weighted, "mask", spec, name, i32=True)


@pytest.mark.parametrize("case", mc.SCATTER_CASES, ids=[c[0] for c in mc.SCATTER_CASES])
def test_max_bwd_scatter_windows(case):
    """The sums are exact in any order with this data, so the atomics' result is the twin's
    bit for bit; the callee's zero fill stays inside the F columns."""
    from plagnn import _lib

    name, F, kind, weighted = case
    i32 = kind == mc.I32
    _, _, _, arg, dout, dx_ref, _ = mc.case(F, weighted, i32)
    g = mc.graph(False, i32)
    dg = g.on(DEV)
    gs = dg.fwd.struct(mc._weights(F, weighted, i32, DEV))
    aw = mc._win(mc._t(arg, DEV), F, mc.SCATTER_SPEC, "arg", mc.ARG_NONE)
    dw = mc._win(mc._t(dout, DEV), F, mc.SCATTER_SPEC, "dout", mc.NAN)
    res = []
    for _ in range(2):
        xw = mc._out(g.num_src, F, torch.float32, DEV, mc.SCATTER_SPEC, "dx", mc.NAN)
        _lib.call("pg_spmm_max_bwd_scatter", gs, aw.ptr, aw.ld, kind, dw.ptr, dw.ld, F, xw.ptr, xw.ld, g.num_src,
                  mc._stream(DEV))
        res.append(xw)
    mc.same(res[0].view, dx_ref, name)
    assert mc.untouched(res[0]) and mc.untouched(res[1]), f"{name}: written outside the F columns"
    assert torch.equal(res[0].bits(), res[1].bits()), f"{name}: second call"


@pytest.mark.parametrize("kind", [mc.U16, mc.I32], ids=["u16", "i32"])
def test_argpos_to_src_windows(kind):
    mc.run_argsrc(DEV, kind)


# ------------------------------------------------------------------ rejections
def _fwd_rejected(dt, key):
    from plagnn import _lib

    F, kind = 256, mc.U16
    X = mc.case(F, False, False)[0]
    g = mc.graph(False, False)
    dg = g.on(DEV)
    gs = dg.fwd.struct(None)
    dtype = mc.DTYPES[dt]
    big = mc._with(mc.FWD_BASE)  # buffers at the baseline's size; only the argument is short
    Xw = mc._win(mc._t(X, DEV, dtype), F, big, "X", mc.X_PAD)
    ow = mc._out(g.num_dst, F, dtype, DEV, big, "out", mc.NAN)
    aw = mc._out(g.num_dst, F, torch.int16, DEV, big, "arg", mc.ARG_JUNK[kind])
    ld = {"X": Xw.ld, "out": ow.ld, "arg": aw.ld}
    ld[key] = F - 1
    ws_n = _lib.lib().pg_spmm_max_fwd_workspace(gs, F, kind)
    ws = mc.workspace(ws_n, DEV)
    with pytest.raises(_lib.PlagnnError, match=INVALID + ".*leading"):
        _lib.call("pg_spmm_max_fwd" + ("_bf16" if dt == "bf16" else ""), gs, Xw.ptr, ld["X"], F, ow.ptr, ld["out"],
                  aw.ptr, ld["arg"], kind, ws.data_ptr(), ws_n, mc._stream(DEV))
    torch.cuda.synchronize()
    assert mc.holds(ow) and mc.holds(aw), f"{dt} {key}: a rejected call wrote"


@pytest.mark.parametrize("key", ["X", "out", "arg"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_max_fwd_rejects_short_ld(dt, key):
    _fwd_rejected(dt, key)


@pytest.mark.parametrize("what", ["arg", "dout", "mask", "fout", "dx", "ws"])
@pytest.mark.parametrize("entry", ["pg_spmm_max_bwd", "pg_spmm_max_bwd_rows"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_max_bwd_rejects(dt, entry, what):
    """A leading dimension one below F, or a workspace 4 bytes off a 16-byte boundary:
    PG_ERR_INVALID before anything is launched, dx keeps its sentinel."""
    from plagnn import _lib

    F, rows = mc.BWD_F, entry.endswith("_rows")
    g = mc.graph(False, False)
    dg = g.on(DEV)
    aw, dw, mw, fw, _, wd = mc.bwd_operands(DEV, F, dt, True, False, "mask_fout", mc.BWD_BASE)
    xw = mc._out(g.num_src, F, mc.DTYPES[dt], DEV, mc.BWD_BASE, "dx", mc.NAN)
    extra = None
    if rows:
        row_active = torch.ones(g.num_dst, dtype=torch.int8, device=DEV)
        extra = (row_active.data_ptr(), dg.bwd.eslot.data_ptr())
    for w, k in ((aw, "arg"), (dw, "dout"), (mw, "mask"), (fw, "fout"), (xw, "dx")):
        if k == what:
            w.ld = F - 1  # (the buffer keeps the baseline's size)
    with pytest.raises(_lib.PlagnnError, match=INVALID + (".*16-byte" if what == "ws" else ".*leading")):
        mc.bwd_call(DEV, entry, g, dg, wd, F, dt, mc.U16, aw, dw, mw, fw, xw, 4 if what == "ws" else 0, extra)
    torch.cuda.synchronize()
    assert mc.holds(xw), f"{entry} {dt} {what}: a rejected call wrote"


@pytest.mark.parametrize("what", ["arg", "dout", "dx"])
def test_scatter_rejects_short_ld(what):
    from plagnn import _lib

    F = 65
    _, _, _, arg, dout, *_ = mc.case(F, False, False)
    g = mc.graph(False, False)
    aw = mc._win(mc._t(arg, DEV), F, mc.SCATTER_SPEC, "arg", mc.ARG_NONE)
    dw = mc._win(mc._t(dout, DEV), F, mc.SCATTER_SPEC, "dout", mc.NAN)
    xw = mc._out(g.num_src, F, torch.float32, DEV, mc.SCATTER_SPEC, "dx", mc.NAN)
    ld = {"arg": aw.ld, "dout": dw.ld, "dx": xw.ld}
    ld[what] = F - 1
    with pytest.raises(_lib.PlagnnError, match=INVALID + ".*leading"):
        _lib.call("pg_spmm_max_bwd_scatter", g.on(DEV).fwd.struct(None), aw.ptr, ld["arg"], mc.U16, dw.ptr, ld["dout"],
                  F, xw.ptr, ld["dx"], g.num_src, mc._stream(DEV))
    torch.cuda.synchronize()
    assert mc.holds(xw), f"{what}: a rejected call wrote"


@pytest.mark.parametrize("what", ["arg", "argx"])
def test_argpos_to_src_rejects_short_ld(what):
    from plagnn import _lib

    F = 65
    arg = mc.case(F, False, False)[3]
    g = mc.graph(False, False)
    aw = mc._win(mc._t(arg, DEV), F, mc.ARGSRC_SPEC, "arg", mc.ARG_NONE)
    xw = mc._out(g.num_dst, F, torch.int64, DEV, mc.ARGSRC_SPEC, "argx", -7)
    ld = {"arg": aw.ld, "argx": xw.ld}
    ld[what] = F - 1
    with pytest.raises(_lib.PlagnnError, match=INVALID + ".*leading"):
        _lib.call("pg_argpos_to_src", g.on(DEV).fwd.struct(None), aw.ptr, ld["arg"], mc.U16, F, xw.ptr, ld["argx"],
                  mc._stream(DEV))
    torch.cuda.synchronize()
    assert mc.holds(xw), f"{what}: a rejected call wrote"
