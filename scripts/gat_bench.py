"""Multi-head attention micro-benchmark on the cfg2 graph (S0, N = 24 041) with H = 4 heads of
Fh = 64 features: per-call medians, HIP-event timed after warm-up, of
  - pg_edge_softmax_fwd and pg_edge_softmax_bwd on (E, H) scores,
  - pg_spmm_sum_heads on the in-CSR and on the transposed CSR (the feature gradient),
  - pg_sddmm_dot_heads,
and, from the same build in the same run, their yardsticks:
  - weighted pg_spmm_sum and plain pg_sddmm_dot at F = H * Fh: they gather the same bytes as
    the two per-head kernels,
  - a torch composition of the edge softmax (scatter_reduce amax, exp, index_add_, divide).
Prints one JSON line with the medians and the ratios.
    python scripts/gat_bench.py [--calls 50] [--warmup 10] [--H 4] [--Fh 64] [--config cfg2]"""
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


def torch_edge_softmax(s, dst, n):
    H = s.shape[1]
    idx = dst[:, None].expand(-1, H)
    m = torch.full((n, H), float("-inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, idx, s, "amax")
    ex = torch.exp(s - m[dst])
    tot = torch.zeros(n, H, dtype=s.dtype, device=s.device).index_add_(0, dst, ex)
    return ex / tot[dst]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--H", type=int, default=4)
    ap.add_argument("--Fh", type=int, default=64)
    ap.add_argument("--config", default="cfg2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench.py needs a HIP device")
    wl = workload.build(args.config)
    g = wl.graph()
    dg = g.on("cuda")
    N, E, H, Fh = g.num_nodes, g.num_edges, args.H, args.Fh
    F = H * Fh
    c, wu = args.calls, args.warmup
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(N, F, device="cuda", generator=gen)
    D = torch.randn(N, F, device="cuda", generator=gen)
    s = torch.randn(E, H, device="cuda", generator=gen) * 3
    da = torch.randn(E, H, device="cuda", generator=gen)
    w = torch.rand(E, device="cuda", generator=gen)
    ptr = g.fwd.ptr.astype(np.int64)
    dst = torch.from_numpy(np.repeat(np.arange(N), np.diff(ptr))).cuda()
    a = ops.edge_softmax(dg, s)
    buf_e, buf_n = torch.empty(E, H, device="cuda"), torch.empty(N, F, device="cuda")

    res = {
        "config": args.config, "N": N, "E": E, "H": H, "Fh": Fh, "calls": c,
        "split_rows": int(g.fwd.n_merges), "max_in_degree": int(g.fwd.max_deg),
        "edge_softmax_fwd_us": median_us(lambda: ops.edge_softmax(dg, s, out=buf_e), c, wu),
        "edge_softmax_bwd_us": median_us(lambda: ops.edge_softmax_backward(dg, a, da, out=buf_e), c, wu),
        "torch_edge_softmax_us": median_us(lambda: torch_edge_softmax(s, dst, N), c, min(wu, 3)),
        "spmm_sum_heads_us": median_us(lambda: ops.spmm_sum_heads(dg, a, X, H, out=buf_n), c, wu),
        "spmm_sum_heads_transposed_us": median_us(
            lambda: ops.spmm_sum_heads(dg, a, X, H, transpose=True, out=buf_n), c, wu),
        "spmm_sum_weighted_us": median_us(lambda: ops.spmm_sum(dg, X, ew_slots=w, out=buf_n), c, wu),
        "spmm_sum_weighted_transposed_us": median_us(
            lambda: ops.spmm_sum(dg, X, ew_slots=w, transpose=True, out=buf_n), c, wu),
        "sddmm_dot_heads_us": median_us(lambda: ops.sddmm_dot_heads(dg, D, X, H, out=buf_e), c, wu),
        "sddmm_dot_us": median_us(lambda: ops.sddmm_dot(dg, D, X), c, wu),
    }
    res["sum_heads_over_sum"] = res["spmm_sum_heads_us"] / res["spmm_sum_weighted_us"]
    res["sum_heads_T_over_sum_T"] = res["spmm_sum_heads_transposed_us"] / res["spmm_sum_weighted_transposed_us"]
    res["sddmm_heads_over_sddmm"] = res["sddmm_dot_heads_us"] / res["sddmm_dot_us"]
    res["torch_softmax_over_fwd"] = res["torch_edge_softmax_us"] / res["edge_softmax_fwd_us"]
    ref = torch_edge_softmax(s.double(), dst, N)
    res["softmax_max_abs_err_vs_f64"] = (a.double() - ref).abs().max().item()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
