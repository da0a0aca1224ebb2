"""Vector-edge-feature micro-benchmark on the cfg2 graph (S0, N = 24 041) at F = 64 and 256:
per-call medians, HIP-event timed after warm-up, of
  - pg_gspmm for mul / sum, add / max and copy_rhs / sum on the in-CSR and on the transposed CSR,
  - pg_gsddmm for sub (u, v) and for the masked copy of the max / min backward,
and, from the same build in the same run, their yardsticks:
  - a torch composition of each aggregation (index_select, the operator, index_add_ or
    scatter_reduce), which writes and re-reads an (E, F) message tensor,
  - the weighted pg_spmm_sum at the same F (one scalar per edge instead of an (E, F) stream).
Edge tensors are in edge-id order and reach the kernels through the cached edge map.
Prints one JSON line with the medians and the ratios; exits 1 if mul / sum at F = 256 is not
faster than its torch composition.
    python scripts/gspmm_bench.py [--calls 30] [--warmup 5] [--config cfg2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pla-gnn_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import plagnn  # noqa: E402, F401
from plagnn import ops, workload  # noqa: E402


def median_us(fn, calls, warmup):
    """Median over `calls` single calls, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gspmm_bench.py needs a HIP device")
    g = workload.build(args.config).graph()
    dg = g.on("cuda")
    N, E = g.num_nodes, g.num_edges
    c, wu = args.calls, args.warmup
    ptr = g.fwd.ptr.astype(np.int64)
    eid = g.eid.astype(np.int64)
    src_np, dst_np = np.empty(E, np.int64), np.empty(E, np.int64)
    src_np[eid], dst_np[eid] = g.fwd.col, np.repeat(np.arange(N), np.diff(ptr))
    src, dst = torch.from_numpy(src_np).cuda(), torch.from_numpy(dst_np).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {"config": args.config, "N": N, "E": E, "calls": c, "split_rows": int(g.fwd.n_merges),
           "max_in_degree": int(g.fwd.max_deg)}
    for F in (64, 256):
        X = torch.randn(N, F, device="cuda", generator=gen)
        D = torch.randn(N, F, device="cuda", generator=gen)
        Y = torch.randn(E, F, device="cuda", generator=gen)
        w = torch.rand(E, device="cuda", generator=gen)
        out_n, out_e = torch.empty(N, F, device="cuda"), torch.empty(E, F, device="cuda")
        arg = torch.empty(N, F, dtype=dg.arg_dtype, device="cuda")
        idx = dst[:, None].expand(-1, F)

        def torch_mul_sum():
            return torch.zeros(N, F, device="cuda").index_add_(0, dst, X.index_select(0, src) * Y)

        def torch_add_max():
            return torch.full((N, F), float("-inf"), device="cuda").scatter_reduce(
                0, idx, X.index_select(0, src) + Y, "amax")

        def torch_copy_sum():
            return torch.zeros(N, F, device="cuda").index_add_(0, dst, Y)

        r = {}
        for tr, tag in ((False, ""), (True, "_transposed")):
            r["gspmm_mul_sum" + tag + "_us"] = median_us(
                lambda: ops.gspmm(dg, "mul", "sum", X, Y, transpose=tr, out=out_n), c, wu)
            r["gspmm_add_max" + tag + "_us"] = median_us(
                lambda: ops.gspmm(dg, "add", "max", X, Y, transpose=tr, out=out_n, argpos=arg), c, wu)
            r["gspmm_copy_rhs_sum" + tag + "_us"] = median_us(
                lambda: ops.gspmm(dg, "copy_rhs", "sum", None, Y, transpose=tr, out=out_n), c, wu)
        ops.gspmm(dg, "add", "max", X, Y, out=out_n, argpos=arg)
        r["gsddmm_sub_us"] = median_us(lambda: ops.gsddmm(dg, "sub", X, D, "u", "v", out=out_e), c, wu)
        r["gsddmm_masked_copy_us"] = median_us(
            lambda: ops.gsddmm(dg, "copy_lhs", D, None, "v", "e", out=out_e, argpos=arg), c, wu)
        r["torch_mul_sum_us"] = median_us(torch_mul_sum, c, min(wu, 3))
        r["torch_add_max_us"] = median_us(torch_add_max, c, min(wu, 3))
        r["torch_copy_sum_us"] = median_us(torch_copy_sum, c, min(wu, 3))
        r["spmm_sum_weighted_us"] = median_us(lambda: ops.spmm_sum(dg, X, ew_slots=w, out=out_n), c, wu)
        r["torch_over_gspmm_mul_sum"] = r["torch_mul_sum_us"] / r["gspmm_mul_sum_us"]
        r["torch_over_gspmm_add_max"] = r["torch_add_max_us"] / r["gspmm_add_max_us"]
        r["torch_over_gspmm_copy_rhs_sum"] = r["torch_copy_sum_us"] / r["gspmm_copy_rhs_sum_us"]
        r["gspmm_mul_sum_over_spmm_sum_weighted"] = r["gspmm_mul_sum_us"] / r["spmm_sum_weighted_us"]
        # forward byte model: the E x F stream, E gathered rows, N x F written
        r["gspmm_mul_sum_model_GBps"] = (2 * E * F + N * F) * 4 / r["gspmm_mul_sum_us"] / 1e3
        ref = torch.zeros(N, F, dtype=torch.float64, device="cuda").index_add_(0, dst, X.double()[src] * Y.double())
        r["mul_sum_max_abs_err_vs_f64"] = (ops.gspmm(dg, "mul", "sum", X, Y).double() - ref).abs().max().item()
        res[f"F{F}"] = r
    res["mul_sum_F256_faster_than_torch"] = res["F256"]["gspmm_mul_sum_us"] < res["F256"]["torch_mul_sum_us"]
    print(json.dumps(res))
    if not res["mul_sum_F256_faster_than_torch"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
