"""TrainEngine.ACTIVE_TOP_ROWS (the top layer's backward on the train rows only) against the
all-rows backward from the same seed: losses, logits, every parameter and every gradient
bitwise equal after three steps, eager and as graph replays, with the full train set and
with every fourth train row (a data-parallel shard's share).
"""
import numpy as np
import pytest
import torch

from conftest import random_graph

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (40, 64, 64, 64, 20, 12)
N = 600


def _problem():
    rng = np.random.default_rng(11)
    src, dst = random_graph(N, 6000, seed=11, self_loop=True)
    x = torch.from_numpy(rng.standard_normal((N, DIMS[0])).astype(np.float32))
    labels = torch.from_numpy((rng.random((N, DIMS[-1])) < 0.3).astype(np.float32))
    labels[rng.random(N) < 0.5] = 0.0
    labelled = np.nonzero(labels.sum(1).numpy() > 0)[0]
    cut = len(labelled) * 9 // 10
    w = rng.uniform(0.5, 3.0, DIMS[-1])
    return src, dst, x, labels, w, labelled[:cut], labelled[cut:]


def _run(active, captured, train, poison):
    import plagnn
    from plagnn.model import GNN

    class Engine(plagnn.TrainEngine):
        ACTIVE_TOP_ROWS = active

    src, dst, x, labels, w, tr, va = _problem()
    tr = tr[::4] if train == "shard" else tr
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in GNN(list(DIMS)).state_dict().items()}
    eng = Engine(plagnn.CSRGraph(src, dst, N), x, labels, DIMS, w, tr, va, lr=1e-3, device=DEV, params=sd)
    if poison:  # the rows the active form never writes are never read either
        eng.dM[eng.L - 1][eng.row_active == 0] = float("nan")
    losses = []
    if captured:
        eng.capture(warmup=1)
        losses.append(eng.losses())
        for _ in range(2):
            eng.step()
            losses.append(eng.losses())
    else:
        for _ in range(3):
            eng.step_eager()
            losses.append(eng.losses())
    torch.cuda.synchronize()
    assert eng.steps_done == 3
    out = {"losses": torch.tensor(losses), "logits": eng.logits().clone()}
    out.update({"p." + k: v.clone() for k, v in eng.state_dict().items()})
    out.update({"g." + k: v.clone() for k, v in eng.grads().items()})
    return eng, out


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("train", ["full", "shard"])
def test_active_top_rows_bitwise(captured, train):
    off_eng, off = _run(False, captured, train, poison=False)
    on_eng, on = _run(True, captured, train, poison=True)
    assert on_eng._rows_gemm and on_eng._rows_spmm  # the row forms ran, not their fallbacks
    n_act = int(on_eng.row_active.sum())
    assert 0 < n_act < N and on_eng.train_rows.numel() == n_act
    assert set(on) == set(off)
    for k in off:
        a, b = on[k].contiguous(), off[k].contiguous()
        assert not torch.isnan(a).any(), k
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    # the work models count the top layer at the active rows
    assert on_eng.flops_per_step() < off_eng.flops_per_step()
    assert on_eng.gemm_bytes_per_step() < off_eng.gemm_bytes_per_step()
    top = on_eng.L - 1
    assert on_eng.spmm_bwd_bytes(top) < off_eng.spmm_bwd_bytes(top)
    assert on_eng.spmm_bwd_bytes(0) == off_eng.spmm_bwd_bytes(0)
