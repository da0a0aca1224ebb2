"""GATv2 attention-score micro-benchmark on the cfg2 graph (S0, N = 24 041) at H = 4 and
H*Fh = 64 and 256: per-call medians, HIP-event timed after warm-up, of
  - the fused score forward (pg_gatv2_score),
  - the fused backward with all three gradients (two pg_gatv2_bwd passes, dattn on the first),
  - forward + backward of ops.GATv2Score through autograd,
and, from the same build in the same run, the unfused composition on the shim's own primitives
(apply_edges(u_add_v) -> leaky_relu -> * attn -> sum(-1)), forward and forward + backward, which
writes and re-reads (E, H, Fh) tensors. torch.cuda.max_memory_allocated above the inputs is
recorded for each. Writes one JSON document (also printed as one line); exits 1 if the fused
forward or the fused forward + backward is not faster than the composition.
    python scripts/gatv2_bench.py [--calls 30] [--warmup 5] [--config cfg2] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pla-gnn_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dgl  # noqa: E402
import dgl.function as fn  # noqa: E402
import plagnn  # noqa: E402, F401
from plagnn import ops, workload  # noqa: E402


def measure(fn_, calls, warmup):
    """(median us over `calls` single calls, each between its own pair of events; peak bytes
    allocated above what was live before the first timed call)."""
    for _ in range(warmup):
        fn_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn_()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "gatv2_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gatv2_bench.py needs a HIP device")
    g = workload.build(args.config).graph()
    dg = g.on("cuda")
    N, E = g.num_nodes, g.num_edges
    c, wu = args.calls, args.warmup
    ptr = g.fwd.ptr.astype(np.int64)
    eid = g.eid.astype(np.int64)
    src_np, dst_np = np.empty(E, np.int64), np.empty(E, np.int64)
    src_np[eid], dst_np[eid] = g.fwd.col, np.repeat(np.arange(N), np.diff(ptr))
    sg = dgl.graph((torch.from_numpy(src_np), torch.from_numpy(dst_np)), num_nodes=N).to("cuda")
    eid_t = torch.from_numpy(eid).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    H, slope = 4, 0.2
    res = {"config": args.config, "N": N, "E": E, "H": H, "calls": c, "warmup": wu,
           "split_rows": int(g.fwd.n_merges), "max_in_degree": int(g.fwd.max_deg), "ok": True}
    for F in (64, 256):
        Fh = F // H
        xl = torch.randn(N, F, device="cuda", generator=gen)
        xr = torch.randn(N, F, device="cuda", generator=gen)
        attn = torch.randn(1, H, Fh, device="cuda", generator=gen)
        flat = attn.reshape(-1)
        ds = torch.randn(E, H, device="cuda", generator=gen)       # slot order
        ds_eid = torch.empty_like(ds).index_copy(0, eid_t, ds)     # the same values in edge-id order
        s_out = torch.empty(E, H, device="cuda")
        leaves = [t.clone().requires_grad_(True) for t in (xl, xr, attn)]

        def fused_fwd():
            return ops.gatv2_score(dg, xl, xr, flat, H, slope, out=s_out)

        def fused_bwd():
            return ops.gatv2_score_backward(dg, ds, xl, xr, flat, H, slope)

        def fused_fwd_bwd():
            for t in leaves:
                t.grad = None
            ops.GATv2Score.apply(leaves[0], leaves[1], leaves[2], dg, H, slope).backward(ds)

        def unfused(a, b, w):
            with sg.local_scope():
                sg.srcdata["el"], sg.dstdata["er"] = a.view(N, H, Fh), b.view(N, H, Fh)
                sg.apply_edges(fn.u_add_v("el", "er", "e"))
                e = torch.nn.functional.leaky_relu(sg.edata.pop("e"), slope)
                return (e * w).sum(-1)                                # (E, H), edge-id order

        def unfused_fwd():
            with torch.no_grad():
                return unfused(xl, xr, attn)

        def unfused_fwd_bwd():
            for t in leaves:
                t.grad = None
            unfused(*leaves).backward(ds_eid)

        r = {}
        for name, f_, w_ in (("fused_fwd", fused_fwd, wu), ("fused_bwd", fused_bwd, wu),
                             ("fused_fwd_bwd", fused_fwd_bwd, wu), ("unfused_fwd", unfused_fwd, min(wu, 3)),
                             ("unfused_fwd_bwd", unfused_fwd_bwd, min(wu, 3))):
            r[name + "_us"], r[name + "_peak_bytes"] = measure(f_, c, w_)
        r["unfused_over_fused_fwd"] = r["unfused_fwd_us"] / r["fused_fwd_us"]
        r["unfused_over_fused_fwd_bwd"] = r["unfused_fwd_bwd_us"] / r["fused_fwd_bwd_us"]
        # forward byte model: E gathered rows of H*Fh*4 B, E*H*4 B written
        r["fused_fwd_model_GBps"] = (E * F + E * H) * 4 / r["fused_fwd_us"] / 1e3
        # the two agree (scores in slot order against the composition's, gradients of one run each)
        s_ref = unfused_fwd().index_select(0, eid_t)
        r["fwd_max_abs_diff_vs_unfused"] = (fused_fwd() - s_ref).abs().max().item()
        unfused_fwd_bwd()
        g_ref = [t.grad.clone() for t in leaves]
        fused_fwd_bwd()
        r["grad_max_rel_diff_vs_unfused"] = max(
            ((t.grad - gr).abs().max() / gr.abs().max()).item() for t, gr in zip(leaves, g_ref))
        r["edge_tensor_bytes"] = E * F * 4
        res[f"F{F}"] = r
        res["ok"] = res["ok"] and r["unfused_over_fused_fwd"] > 1.0 and r["unfused_over_fused_fwd_bwd"] > 1.0
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    if not res["ok"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
