"""Mini-batch sampling benchmark: NeighborSampler([10, 10, 10]).sample_blocks for 1024 seeds on
the cfg2 graph (S0, N = 24 041) and the cfg5 graph (RMAT x16, N = 384 656), per batch:
  - end to end (host clock around a call that ends in a device synchronise): median, p10, p90;
  - the same work split, with a synchronise after every part, into the sampling kernels
    (pg_sample_count + pg_sample_fill), the compaction kernels (pg_block_compact), the count
    read-backs (device -> host scalars) and, for the host build (plagnn.graph.DEVICE_BUILD =
    False), the device -> host copies of ptr / col, the host transpose + schedule build
    (CSRGraph.from_in_csr) and the upload of the block's CSR; for the device build, the
    transpose kernels (pg_csr_transpose_dev) and the schedule kernels (pg_schedule_count_dev +
    pg_schedule_build_dev) in their place;
  - one forward + backward of three SAGEConv('pool') layers on those blocks (HIP events),
    beside one eager full-graph TrainEngine step (forward + backward, the same f32 dims).
--build host|device|both picks the block build; `both` alternates the two batch by batch on the
same seeds inside one process, after a warm-up of each, so that the two medians share one run's
spread. Writes one JSON document (also printed as one line). Needs a HIP device.
    python scripts/sample_bench.py [--build both] [--batches 60] [--warmup 10] [--configs cfg2,cfg5-f32] [--out PATH]"""
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
import plagnn  # noqa: E402
from dgl.dataloading import NeighborSampler  # noqa: E402
from dgl.nn.pytorch import SAGEConv  # noqa: E402
from plagnn import graph as engine_graph  # noqa: E402
from plagnn import ops, workload  # noqa: E402

FANOUTS = [10, 10, 10]
COMMON_PARTS = ["sample_kernels", "compact_kernels", "count_readbacks"]
BUILD_PARTS = {"host": ["d2h_copies", "host_transpose_schedule", "upload"],
               "device": ["transpose_kernels", "schedule_kernels"]}
PARTS = COMMON_PARTS + BUILD_PARTS["host"] + BUILD_PARTS["device"]


def pct(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90))}


class Clock:
    def __init__(self):
        self.t = {k: 0.0 for k in PARTS}
        self.last = None

    def start(self):
        torch.cuda.synchronize()
        self.last = time.perf_counter()

    def lap(self, part, sync=True):
        if sync:
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.t[part] += (now - self.last) * 1e3
        self.last = now


def split_batch(g, seeds, build):
    """One batch with the sampler's own steps (dgl/dataloading/__init__.py, plagnn/ops.py) and a
    synchronise after each part; returns the milliseconds per part."""
    from plagnn import _lib
    from plagnn._lib import call, ptr

    dg = g._device_graph(g.device)
    dev = g.device
    ck = Clock()
    n_parent = g.num_nodes()
    st = _lib.stream_handle(dev)
    for fanout in reversed(FANOUTS):
        s32 = seeds.to(torch.int32).contiguous()
        n = s32.numel()
        gs_, emap = dg.fwd.struct(None), dg.edge_map()
        out_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        ws_n = _lib.lib().pg_sample_count_workspace(n)
        ws = ops._workspace(ws_n, dev)
        ck.start()
        call("pg_sample_count", gs_, ptr(s32), n, fanout, ptr(out_ptr), ptr(ws), ws_n, st)
        ck.lap("sample_kernels")
        total = int(out_ptr[n])
        ck.lap("count_readbacks")
        col = torch.empty(total, dtype=torch.int32, device=dev)
        eid = torch.empty(total, dtype=torch.int32, device=dev)
        ck.start()
        call("pg_sample_fill", gs_, ptr(emap), ptr(s32), n, fanout, 12345, ptr(out_ptr), ptr(col), ptr(eid), st)
        ck.lap("sample_kernels")
        src_ids = torch.empty(n + total, dtype=torch.int32, device=dev)
        col_local = torch.empty(total, dtype=torch.int32, device=dev)
        n_src = torch.empty(1, dtype=torch.int32, device=dev)
        ws_n = _lib.lib().pg_block_compact_workspace(n, total, n_parent)
        ws = ops._workspace(ws_n, dev)
        ck.start()
        call("pg_block_compact", ptr(s32), n, ptr(col), total, n_parent, ptr(src_ids), ptr(col_local), ptr(n_src),
             ptr(ws), ws_n, st)
        ck.lap("compact_kernels")
        ns = int(n_src[0])
        ck.lap("count_readbacks")
        if build == "host":
            hp, hc = out_ptr.cpu().numpy(), col_local.cpu().numpy()
            ck.lap("d2h_copies")
            blk = plagnn.CSRGraph.from_in_csr(hp, hc, ns)
            ck.lap("host_transpose_schedule", sync=False)
            blk.on(dev)
            ck.lap("upload")
        else:  # DeviceGraph.from_in_csr's steps
            chunk, chunk_bwd = engine_graph.DEFAULT_CHUNK, engine_graph.default_chunk_bwd(max(ns, n))
            cf = engine_graph._schedule_count_dev(out_ptr, chunk)
            ck.lap("schedule_kernels")
            tptr, tcol, tslot, tpos, status = engine_graph._transpose_dev(out_ptr, col_local, ns)
            ck.lap("transpose_kernels")
            cb = engine_graph._schedule_count_dev(tptr, chunk_bwd)
            ck.lap("schedule_kernels")
            back = torch.cat([cf, cb, status.to(torch.int64)]).tolist()
            ck.lap("count_readbacks")
            engine_graph._schedule_build_dev(out_ptr, chunk, back[0], back[1], back[3])
            engine_graph._schedule_build_dev(tptr, chunk_bwd, back[6], back[7], back[9])
            ck.lap("schedule_kernels")
        seeds = src_ids[:ns].to(torch.int64)
    return ck.t


def model_step(g, layers, x, sampler, seeds, calls, warmup):
    inp, out, blocks = sampler.sample_blocks(g, seeds)
    h0 = x[inp]

    def run():
        h = h0
        for layer, b in zip(layers, blocks):
            h = torch.relu(layer(b, h))
        h.sum().backward()

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        run()
        b.record()
    torch.cuda.synchronize()
    return pct([a.elapsed_time(b) for a, b in ev]), [int(b.num_src_nodes()) for b in blocks], \
        [int(b.num_edges()) for b in blocks]


def full_step(wl, calls, warmup):
    eng = plagnn.TrainEngine(wl.graph(), torch.from_numpy(wl.ds.feat), torch.from_numpy(wl.ds.loc.astype(np.float32)),
                             wl.dims, wl.class_weight, wl.train_index, wl.val_index, device="cuda")
    for _ in range(warmup):
        eng.forward()
        eng.backward()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        eng.forward()
        eng.backward()
        b.record()
    torch.cuda.synchronize()
    return pct([a.elapsed_time(b) for a, b in ev])


def bench(name, batches, warmup, builds):
    wl = workload.build(name)
    n = wl.n
    g = dgl.graph((torch.from_numpy(wl.src), torch.from_numpy(wl.dst)), num_nodes=n).to("cuda")
    rng = np.random.default_rng(0)
    train = np.asarray(wl.train_index)
    sampler = NeighborSampler(FANOUTS)
    pick = lambda: torch.from_numpy(rng.choice(train, 1024, replace=False)).to("cuda")  # noqa: E731
    dgl.seed(0)
    e2e = {b: [] for b in builds}
    for i in range(warmup + batches):
        seeds = pick()
        for b in builds:  # the same seeds through every build, one after the other
            engine_graph.DEVICE_BUILD = b == "device"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.sample_blocks(g, seeds)
            torch.cuda.synchronize()
            if i >= warmup:
                e2e[b].append((time.perf_counter() - t0) * 1e3)
    parts = {b: {k: [] for k in COMMON_PARTS + BUILD_PARTS[b]} for b in builds}
    for i in range(warmup + batches):
        seeds = pick()
        for b in builds:
            t = split_batch(g, seeds, b)
            if i >= warmup:
                for k in parts[b]:
                    parts[b][k].append(t[k])
    med = {b: {k: float(np.median(v)) for k, v in parts[b].items()} for b in builds}
    total = {b: sum(med[b].values()) for b in builds}
    engine_graph.DEVICE_BUILD = builds[-1] == "device"
    dims = wl.dims
    torch.manual_seed(0)
    layers = [SAGEConv(dims[i], dims[i + 1], "pool").to("cuda") for i in range(3)]
    x = torch.from_numpy(wl.ds.feat).to("cuda")
    step, n_src, n_edges = model_step(g, layers, x, sampler, pick(), 30, 5)
    del layers, x, g
    torch.cuda.empty_cache()
    full = full_step(wl, 20, 3)
    return {"config": name, "nodes": n, "edges": int(len(wl.src)), "seeds": 1024, "fanouts": FANOUTS,
            "batches": batches, "builds": builds, "sample_blocks_ms": {b: pct(e2e[b]) for b in builds},
            "parts_median_ms": med, "parts_sum_ms": total,
            "block_src_nodes": n_src, "block_edges": n_edges, "sage_pool3_fwd_bwd_on_blocks_ms": step,
            "full_graph_engine_fwd_bwd_ms": full}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default="cfg2,cfg5-f32")
    ap.add_argument("--build", choices=["host", "device", "both"], default="both")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "sample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench.py needs a HIP device")
    builds = ["host", "device"] if args.build == "both" else [args.build]
    res = {"device": torch.cuda.get_device_name(0), "results": []}
    for name in args.configs.split(","):
        res["results"].append(bench(name, args.batches, args.warmup, builds))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
