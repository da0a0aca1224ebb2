"""Link-prediction mini-batch timing on the cfg2 graph (S0, N = 24 041, made bidirected: edge
e + E is the reverse of edge e). Per batch, host clock around a call that ends in a device
synchronise:
  - edge-seeded: 1024 seed edges through as_edge_prediction_sampler(NeighborSampler([10, 10,
    10]), exclude='reverse_id', negative_sampler=Uniform(5)): find_edges, the negatives
    (pg_negative_sample), the pair graphs' compaction, the exclusion bits set and cleared
    (pg_edge_bits_update) and three layers of pg_sample_*_excl + block builds;
  - node-seeded, beside it in the same process and alternating batch by batch:
    NeighborSampler([10, 10, 10]).sample_blocks on as many seed nodes as the edge batch's pair
    graphs hold (pg_sample_count / pg_sample_fill: the yardstick for what exclusion and
    negatives add).
Median, p10 and p90 over the timed batches; one JSON line. Needs a HIP device.
    python scripts/linkpred_sample_time.py [--batches 60] [--warmup 10] [--config cfg2] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pla-gnn_amd"), ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dgl  # noqa: E402
from dgl.dataloading import NeighborSampler, as_edge_prediction_sampler, negative_sampler  # noqa: E402
from plagnn import workload  # noqa: E402

FANOUTS = [10, 10, 10]
SEED_EDGES = 1024
K = 5


def pct(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "linkpred_sample_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linkpred_sample_time.py needs a HIP device")
    wl = workload.build(args.config)
    src, dst = torch.from_numpy(np.asarray(wl.src)).long(), torch.from_numpy(np.asarray(wl.dst)).long()
    E, n = src.numel(), wl.n
    g = dgl.graph((torch.cat([src, dst]), torch.cat([dst, src])), num_nodes=n).to("cuda")
    rev = torch.cat([torch.arange(E) + E, torch.arange(E)]).to("cuda")
    nodes = NeighborSampler(FANOUTS)
    edges = as_edge_prediction_sampler(nodes, exclude="reverse_id", reverse_eids=rev,
                                       negative_sampler=negative_sampler.Uniform(K))
    rng = np.random.default_rng(0)
    dgl.seed(0)
    t_edge, t_node, n_nodes, n_inputs = [], [], [], []
    for i in range(args.warmup + args.batches):
        batch = torch.from_numpy(rng.choice(2 * E, SEED_EDGES, replace=False)).to("cuda")
        (inp, pair, neg, blocks), te = timed(lambda: edges.sample(g, batch))
        m = pair.num_nodes()
        seeds = torch.from_numpy(rng.choice(n, m, replace=False)).to("cuda")
        _, tn = timed(lambda: nodes.sample_blocks(g, seeds))
        if i >= args.warmup:
            t_edge.append(te)
            t_node.append(tn)
            n_nodes.append(m)
            n_inputs.append(int(inp.numel()))
    res = {"device": torch.cuda.get_device_name(0), "config": args.config, "nodes": n, "edges": 2 * E,
           "seed_edges": SEED_EDGES, "negatives_per_edge": K, "fanouts": FANOUTS, "exclude": "reverse_id",
           "batches": args.batches, "warmup": args.warmup,
           "seed_nodes_per_batch_median": float(np.median(n_nodes)),
           "input_nodes_per_batch_median": float(np.median(n_inputs)),
           "edge_seeded_ms": pct(t_edge), "node_seeded_same_seed_count_ms": pct(t_node)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
