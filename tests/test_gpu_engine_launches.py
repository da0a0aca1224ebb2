"""The library entry points one training step issues, in order, with the launch site each
runs under: TrainEngine and TrainEngineBF16 on the problem of test_gpu_engine_active_rows.py
(three SAGE layers, both active-rows forms run), on a one-layer model (the single-bucket
path; the narrow shape of test_gpu_mlp_head.py), and the f32 engine with the head as separate
launches. The step driver is Python; this sequence is what a change to it must keep. One
step_eager() is recorded at the two functions the engine reaches the library through.
"""
import numpy as np
import pytest
import torch

from conftest import random_graph
from test_gpu_engine_active_rows import DIMS, N, _problem

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS1, N1, E1 = (33, 60, 28, 3), 97, 900


def _problem1():
    rng = np.random.default_rng(7)
    src, dst = random_graph(N1, E1, seed=7, self_loop=True)
    x = torch.from_numpy(rng.standard_normal((N1, DIMS1[0])).astype(np.float32))
    labels = torch.from_numpy((rng.random((N1, DIMS1[-1])) < 0.3).astype(np.float32))
    idx = rng.permutation(N1)
    w = rng.uniform(0.5, 3.0, DIMS1[-1])
    return src, dst, x, labels, w, idx[: N1 // 2], idx[N1 // 2: N1 // 2 + N1 // 5]


def _record(monkeypatch, cls, dims, n, problem):
    import plagnn
    from plagnn import _lib, engine
    from plagnn.model import GNN

    src, dst, x, labels, w, tr, va = problem()
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in GNN(list(dims)).state_dict().items()}
    eng = cls(plagnn.CSRGraph(src, dst, n), x, labels, dims, w, tr, va, lr=1e-3, device=DEV, params=sd)
    rec = []
    call, call_supported = engine.call, _lib.call_supported

    def rec_call(name, *args):
        rec.append((eng._cur, name))
        return call(name, *args)

    def rec_call_supported(name, *args):
        rec.append((eng._cur, name))
        return call_supported(name, *args)

    monkeypatch.setattr(engine, "call", rec_call)
    monkeypatch.setattr(_lib, "call_supported", rec_call_supported)
    eng.step_eager()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert eng.steps_done == 1 and all(np.isfinite(eng.losses()))
    return rec


F32_L3 = [
    ("gemm.fwd.pool.l1", "pg_gemm_f32"),
    ("spmm_max_fwd.l1", "pg_spmm_max_fwd"),
    ("gemm.fwd.cat.l1", "pg_gemm_f32"),
    ("gemm.fwd.pool.l2", "pg_gemm_f32"),
    ("spmm_max_fwd.l2", "pg_spmm_max_fwd"),
    ("gemm.fwd.cat.l2", "pg_gemm_f32"),
    ("gemm.fwd.pool.l3", "pg_gemm_f32"),
    ("spmm_max_fwd.l3", "pg_spmm_max_fwd"),
    ("gemm.fwd.cat.l3", "pg_gemm_f32"),
    ("head.l1", "pg_mlp_l1_head_ex"),
    ("gemm.dgrad.neigh.l3", "pg_gemm_f32_rows"),
    ("spmm_max_bwd.l3", "pg_spmm_max_bwd_rows"),
    ("gemm.dgrad.stack.l3", "pg_gemm_f32"),
    ("gemm.dgrad.neigh.l2", "pg_gemm_f32"),
    ("spmm_max_bwd.l2", "pg_spmm_max_bwd"),
    ("gemm.dgrad.stack.l2", "pg_gemm_f32"),
    ("gemm.dgrad.neigh.l1", "pg_gemm_f32"),
    ("spmm_max_bwd.l1", "pg_spmm_max_bwd"),
    ("gemm.wgrad.group", "pg_gemm_f32_group"),
    ("adam", "pg_adam_apply_l1"),
]

# FUSED_L1_HEAD = False: liner1 as GEMMs around pg_mlp_head, no kept W1 pieces, so the plain Adam
F32_L3_UNFUSED = F32_L3[:9] + [
    ("gemm.fwd.liner1", "pg_gemm_f32"),
    ("head", "pg_mlp_head"),
    ("gemm.dgrad.liner1", "pg_gemm_f32"),
] + F32_L3[10:19] + [
    ("adam", "pg_adam_prepare"),
    ("adam", "pg_adam_apply"),
]

BF16_L3 = [
    ("gemm.fwd.pool.l1", "pg_gemm_bf16"),
    ("spmm_max_fwd.l1", "pg_spmm_max_fwd_bf16"),
    ("gemm.fwd.cat.l1", "pg_gemm_bf16"),
    ("gemm.fwd.pool.l2", "pg_gemm_bf16"),
    ("spmm_max_fwd.l2", "pg_spmm_max_fwd_bf16"),
    ("gemm.fwd.cat.l2", "pg_gemm_bf16"),
    ("gemm.fwd.pool.l3", "pg_gemm_bf16"),
    ("spmm_max_fwd.l3", "pg_spmm_max_fwd_bf16"),
    ("gemm.fwd.cat.l3", "pg_gemm_bf16"),
    ("gemm.fwd.liner1", "pg_gemm_bf16"),
    ("head", "pg_mlp_head"),
    ("gemm.dgrad.liner1", "pg_gemm_bf16"),
    ("gemm.dgrad.neigh.l3", "pg_gemm_bf16"),
    ("spmm_max_bwd.l3", "pg_spmm_max_bwd_rows_bf16"),
    ("gemm.dgrad.stack.l3", "pg_gemm_bf16"),
    ("gemm.dgrad.neigh.l2", "pg_gemm_bf16"),
    ("spmm_max_bwd.l2", "pg_spmm_max_bwd_bf16"),
    ("gemm.dgrad.stack.l2", "pg_gemm_bf16"),
    ("gemm.dgrad.neigh.l1", "pg_gemm_bf16"),
    ("spmm_max_bwd.l1", "pg_spmm_max_bwd_bf16"),
    ("gemm.wgrad.group", "pg_gemm_bf16_group"),
    ("adam", "pg_adam_prepare"),
    ("adam", "pg_adam_apply"),
    ("adam", "pg_cast_f32_bf16"),
]

F32_L1 = [
    ("gemm.fwd.pool.l1", "pg_gemm_f32"),
    ("spmm_max_fwd.l1", "pg_spmm_max_fwd"),
    ("gemm.fwd.cat.l1", "pg_gemm_f32"),
    ("head.l1", "pg_mlp_l1_head_ex"),
    ("gemm.dgrad.neigh.l1", "pg_gemm_f32_rows"),
    ("spmm_max_bwd.l1", "pg_spmm_max_bwd_rows"),
    ("gemm.wgrad.group", "pg_gemm_f32_group"),
    ("adam", "pg_adam_apply_l1"),
]

BF16_L1 = [
    ("gemm.fwd.pool.l1", "pg_gemm_bf16"),
    ("spmm_max_fwd.l1", "pg_spmm_max_fwd_bf16"),
    ("gemm.fwd.cat.l1", "pg_gemm_bf16"),
    ("gemm.fwd.liner1", "pg_gemm_bf16"),
    ("head", "pg_mlp_head"),
    ("gemm.dgrad.liner1", "pg_gemm_bf16"),
    ("gemm.dgrad.neigh.l1", "pg_gemm_bf16"),
    ("spmm_max_bwd.l1", "pg_spmm_max_bwd_rows_bf16"),
    ("gemm.wgrad.group", "pg_gemm_bf16_group"),
    ("adam", "pg_adam_prepare"),
    ("adam", "pg_adam_apply"),
    ("adam", "pg_cast_f32_bf16"),
]


def _engine(kind):
    import plagnn

    if kind == "unfused":
        return type("Unfused", (plagnn.TrainEngine,), {"FUSED_L1_HEAD": False})
    return plagnn.TrainEngineBF16 if kind == "bf16" else plagnn.TrainEngine


@pytest.mark.parametrize("kind,want", [("f32", F32_L3), ("bf16", BF16_L3), ("unfused", F32_L3_UNFUSED)])
def test_step_launch_sequence_three_layers(monkeypatch, kind, want):
    assert _record(monkeypatch, _engine(kind), DIMS, N, _problem) == want


@pytest.mark.parametrize("kind,want", [("f32", F32_L1), ("bf16", BF16_L1)])
def test_step_launch_sequence_one_layer(monkeypatch, kind, want):
    assert _record(monkeypatch, _engine(kind), DIMS1, N1, _problem1) == want
