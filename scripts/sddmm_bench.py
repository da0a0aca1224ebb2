"""pg_sddmm_dot micro-benchmark on the cfg2 graph (S0, N = 24 041, F = 256): per-call medians,
HIP-event timed after warm-up, of
  - pg_sddmm_dot, plain form (the edge-weight gradient of a sum aggregation),
  - pg_sddmm_dot, max form (records of the weighted max aggregation of a relu input),
  - weighted pg_spmm_sum on the same graph and F, from the same build: it gathers the same
    bytes, so it is the yardstick,
  - the torch composition (D[dst] * X[src]).sum(1), which materialises two E x F tensors,
and the ratio of the plain form to the sum. Prints one JSON line.
    python scripts/sddmm_bench.py [--calls 50] [--warmup 10] [--F 256] [--config cfg2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pla-gnn_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import plagnn  # noqa: E402
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--F", type=int, default=256)
    ap.add_argument("--config", default="cfg2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_bench.py needs a HIP device")
    wl = workload.build(args.config)
    g = wl.graph()
    dg = g.on("cuda")
    N, E, F = g.num_nodes, g.num_edges, args.F
    gen = torch.Generator(device="cuda").manual_seed(1)
    D = torch.randn(N, F, device="cuda", generator=gen)
    X = torch.relu(torch.randn(N, F, device="cuda", generator=gen))
    w = torch.rand(E, device="cuda", generator=gen)
    argpos = ops.spmm_max(dg, X, w)[1]
    out = torch.empty(N, F, device="cuda")
    dst, src = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _slot_edges(g))

    res = {
        "config": args.config, "N": N, "E": E, "F": F, "calls": args.calls,
        "sddmm_plain_us": median_us(lambda: ops.sddmm_dot(dg, D, X), args.calls, args.warmup),
        "sddmm_max_us": median_us(lambda: ops.sddmm_dot(dg, D, X, argpos=argpos), args.calls, args.warmup),
        "spmm_sum_weighted_us": median_us(lambda: ops.spmm_sum(dg, X, ew_slots=w, out=out), args.calls,
                                          args.warmup),
        "torch_composition_us": median_us(lambda: (D[dst] * X[src]).sum(1), args.calls, min(args.warmup, 3)),
    }
    res["plain_over_sum"] = res["sddmm_plain_us"] / res["spmm_sum_weighted_us"]
    # the bytes both gathers move at least: E rows of X, plus D / out once, ids and de
    gathered = 4.0 * E * F
    res["sddmm_plain_gather_GBps"] = gathered / res["sddmm_plain_us"] / 1e3
    res["spmm_sum_gather_GBps"] = gathered / res["spmm_sum_weighted_us"] / 1e3
    err = (ops.sddmm_dot(dg, D, X).double() - (D[dst].double() * X[src].double()).sum(1)).abs().max().item()
    res["max_abs_err_vs_f64"] = err
    print(json.dumps(res))


def _slot_edges(g):
    """(dst, src) of every in-CSR slot."""
    ptr = g.fwd.ptr.astype(np.int64)
    dst = np.repeat(np.arange(g.num_nodes), np.diff(ptr))
    return dst, g.fwd.col.astype(np.int64)


if __name__ == "__main__":
    main()
