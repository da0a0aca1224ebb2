"""TrainEngineBF16 — the PLA-GNN training step in bf16 storage with f32 accumulation
(BASELINE configs[4]: "hidden=512 bf16"; SURVEY.md §8d cfg5: "bf16 storage with f32
accumulate"). Not a configuration of the reference (fp32 only): reference-unpinned; the
step is checked against the fp32 oracle at a bf16 tolerance (tests/test_gpu_engine_bf16.py).

The step itself is TrainEngine's (code/train.py:197-207; engine.py), with the same flat f32
master parameters, f32 gradients, f32 Adam (one launch) and f32 loss; this class states what
bf16 storage changes, the storage of every N-row tensor and the operands of every product:
  * activations and activation gradients are bf16 (half the bytes of every SpMM gather
    and GEMM operand stream); every GEMM runs on v_mfma_f32_32x32x16_bf16 with f32
    accumulate (pg_gemm_bf16, 16x the f32 MFMA rate); the max aggregation selects bf16
    values exactly and its backward sums in f32 (pg_spmm_max_*_bf16);
  * the GEMMs read bf16 copies of the weights, written from the f32 master parameters by
    one gather-cast launch after every Adam step (pg_cast_f32_bf16) in the layouts the
    products want, including a stacked [Wself ; Wpool] so that the input gradient of a
    SAGE layer, dH = (dY Wself + dP Wpool) * leaky'(H), is ONE K = Fo + Fi product with a
    single rounding: dY and dP are stored side by side in DYP_l[N][Fo + Fi].
Widths are padded to multiples of 8 (16-B rows of bf16) instead of 4.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import ptr
from .engine import TrainEngine, _Flat, pg_dtype


class TrainEngineBF16(TrainEngine):
    ACT_DTYPE = torch.bfloat16
    WIDTH_ALIGN = 8
    GEMM = "pg_gemm_bf16"
    SPMM_SUFFIX = "_bf16"
    # the fused liner1 + head kernel is f32 only: bf16 storage keeps liner1 as bf16 GEMMs
    # around pg_mlp_head, which also writes dZ's bf16 copy (liner2's weight-gradient operand)
    FUSED_L1_HEAD = False

    def _setup_active_rows(self, active: np.ndarray) -> None:
        super()._setup_active_rows(active)
        self._rows_gemm = False  # pg_gemm_bf16 has no row-list form: dgrad.neigh runs on all rows

    def _gemm_launch(self, transa, transb, M, N, K, alpha, A, lda, B, ldb, beta, C, ep) -> None:
        # (pg_gemm_bf16 takes the output's dtype: bf16 activations, f32 anything else)
        self._call(self.GEMM, transa, transb, M, N, K, alpha, A, lda, B, ldb, beta, ptr(C), C.stride(0),
                   pg_dtype(C), ep, 1, ptr(self.ws), self.ws_bytes, self._s())

    # ------------------------------------------------------------------ weight copies
    def _weights(self):
        return self.Wb

    def _stack_weight(self, p: str):
        # stored transposed, [Wself ; Wpool]^T as [Fi][Fo + Fi] (B^T, a row image: the A B^T
        # ping-pong kernel of pg_gemm_bf16 takes the product) instead of a [Fo + Fi][Fi] k image
        return self.Wb[p + "WstackT"], True

    def _alloc_param_copies(self) -> None:
        super()._alloc_param_copies()
        self._build_weight_copies()

    def _build_weight_copies(self) -> None:
        """bf16 weight buffer + the gather map from the f32 flat parameters."""
        pd, L = self.pd, self.L
        wl = _Flat()
        for l in range(L):
            Fi, Fo = pd[l], pd[l + 1]
            wl.add(f"conv{l + 1}.Wpool", (Fi, Fi))
            wl.add(f"conv{l + 1}.Wcat", (Fo, 2 * Fi))
            wl.add(f"conv{l + 1}.WstackT", (Fi, Fo + Fi))  # [Wself ; Wpool]^T
        wl.add("liner1.W", (pd[-2], pd[-3]))
        idx = np.full(wl.size, -1, np.int64)
        flat_ids = self.flat_layout.views(torch.arange(self.flat_layout.size))  # flat index of every entry

        def put(name, rows: np.ndarray):
            o = wl.offsets[name]
            idx[o:o + rows.size] = rows.ravel()

        def ids(name, shape):
            t = flat_ids[name].numpy()
            assert t.shape == tuple(shape), (name, t.shape, shape)
            return t

        for l in range(L):
            Fi, Fo = pd[l], pd[l + 1]
            p = f"conv{l + 1}."
            wp = ids(p + "Wpool", (Fi, Fi))
            wc = ids(p + "Wcat", (Fo, 2 * Fi))
            put(p + "Wpool", wp)
            put(p + "Wcat", wc)
            put(p + "WstackT", np.ascontiguousarray(np.concatenate([wc[:, :Fi], wp], axis=0).T))
        put("liner1.W", ids("liner1.W", (pd[-2], pd[-3])))
        self.wb_layout = wl
        self.wb_map = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        self.wb = torch.zeros(wl.size, dtype=torch.bfloat16, device=self.device)
        self.Wb = wl.views(self.wb)

    def _cast_weights(self) -> None:
        self._call("pg_cast_f32_bf16", ptr(self.flat), ptr(self.wb_map), self.wb.numel(), ptr(self.wb), self._s())

    def params_updated(self) -> None:
        """The bf16 weight copies follow the f32 master parameters."""
        super().params_updated()
        self._cast_weights()

    def adam(self) -> None:
        super().adam()
        with self._t("adam"):
            self._cast_weights()
