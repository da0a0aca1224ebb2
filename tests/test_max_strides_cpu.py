"""The stride suite's tables and harness without a GPU (max_common.py; the GPU cases are
test_gpu_max_strides.py).

check_tables: the case tables against the dispatch contract restated in max_common.predict_*:
every forward path and all four (pack, pull) combinations of the grouped backward are reached,
for both storage types and both descriptor placements, and each single-term case differs from
its baseline in exactly the decision it names.

The window / sentinel harness itself runs here against the host twins pg_spmm_max_fwd_cpu,
pg_spmm_max_bwd_cpu and pg_argpos_to_src_cpu, which take leading dimensions too: padded, odd
and offset windows must give the bits of the contiguous call, leave every pad element alone
and let no pad value (2^100 in X, NaN in dout and the mask, "none" records) reach a result.
"""
import pytest
import torch

import max_common as mc


def test_tables_reach_every_path():
    mc.check_tables()


def test_window_and_untouched():
    """window() places, pads and offsets as it says; untouched() sees one changed element
    before, between and after the rows, and none inside; a NaN fill compares as bits."""
    t = torch.arange(15, dtype=torch.float32).view(3, 5)
    for dtype, fill in ((torch.float32, mc.NAN), (torch.bfloat16, mc.X_PAD), (torch.int16, 0x7F7F),
                        (torch.int32, 0x7F7F7F7F), (torch.int64, -7)):
        w = mc.window(t.to(dtype), 7, 3, fill)
        assert w.ptr % 16 == (3 * w.view.element_size()) % 16 and w.ld == 7 and w.view.stride() == (7, 1)
        assert torch.equal(w.view, t.to(dtype)) and mc.untouched(w) and not mc.holds(w)
        assert w.flat.numel() == 3 + 3 * 7 + 4
        w.view[1, 2] = 5
        assert mc.untouched(w)
        for i in (0, 2, 3 + 5, 3 + 7 + 6, 3 + 2 * 7 + 5, 3 + 3 * 7, w.flat.numel() - 1):
            w2 = mc.window(t.to(dtype), 7, 3, fill)
            w2.flat[i] = 1
            assert not mc.untouched(w2), (dtype, i)
        assert mc.holds(mc.filled(3, 5, dtype, "cpu", 7, 3, fill))
    ws = mc.workspace(100, "cpu", 16)
    assert ws.data_ptr() % 256 == 16


FWD_CPU = [c for c in mc.FWD_CASES if c[2] == "f32" and (c[1] != 256 or c[3] == mc.U16)]


@pytest.mark.parametrize("case", FWD_CPU, ids=[c[0] for c in FWD_CPU])
def test_max_fwd_twin_windows(case):
    name, F, dt, kind, weighted, spec, _ = case
    mc.run_fwd("cpu", F, dt, kind, weighted, spec, name)


BWD_CPU = [c for c in mc.BWD_CASES if c[2] == "f32" and not c[3] and c[5] == "mask"]


@pytest.mark.parametrize("case", BWD_CPU, ids=[c[0] for c in BWD_CPU])
def test_max_bwd_twin_windows(case):
    name, F, dt, trans, weighted, mode, spec, _ = case
    mc.run_bwd("cpu", F, dt, trans, weighted, mode, spec, name)


@pytest.mark.parametrize("case", mc.GATHER_CASES, ids=[c[0] for c in mc.GATHER_CASES])
def test_max_bwd_twin_windows_i32(case):
    name, F, weighted, spec, _ = case
    mc.run_bwd("cpu", F, "f32", False, weighted, "mask", spec, name, i32=True)


def test_max_bwd_twin_dead_none_records():
    """The dead-none reference of the GPU cases: on relu inputs the twin's masked result on
    records with "none" at every zero maximum equals its masked result on the full records."""
    from plagnn import ops

    for weighted in (False, True):
        X, w, arg, dout, dx = mc.relu_case(mc.BWD_F, weighted)
        cg = mc.graph(False, False).on("cpu")
        wt = None if w is None else torch.from_numpy(w.copy())
        Xt = torch.from_numpy(X.copy())
        _, full = ops.spmm_max(cg, Xt, wt)
        want = ops.spmm_max_backward(cg, full, torch.from_numpy(dout.copy()), wt, mask=Xt)
        mc.same(torch.from_numpy(dx.copy()), want.numpy(), f"dead-none records, weighted={weighted}")


@pytest.mark.parametrize("kind", [mc.U16, mc.I32], ids=["u16", "i32"])
def test_argpos_to_src_twin_windows(kind):
    mc.run_argsrc("cpu", kind)
