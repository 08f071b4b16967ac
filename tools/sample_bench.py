#!/usr/bin/env python3
"""Neighbour sampling next to the training step it feeds, on workload L's synthetic graph (bench.synth: |V| = 2 M,
|E| = 60 M, d = 128) and on the power-law graph of the same size (hub rows of 10^4 .. 10^5 slots).

Per (graph, fan-outs, batch size), over `--batches` batches of distinct random seeds, all in one process and one run:
  sample_ms   NeighborSampler.sample alone, wall clock from call to a finished device (the sampler waits for the device
              twice per hop itself, so host time IS part of what a training loop pays; an event pair would hide it)
  step_ms     the training step on that very batch: gather of the feature rows and labels, GraphSAGE (one SAGEConv layer
              per hop, hidden 128) training forward, masked cross-entropy on the seed rows, backward, one Adam step —
              what experiment(num_neighbors=...) runs per batch; wall clock to a finished device as well
  edges/s     sampled edges per second of sample_ms
The medians are reported (min and max next to them), then whether sampling is below the batch's own training step.
One warm-up batch per configuration is not counted. Prints a table, then one JSON line.
Usage: python tools/sample_bench.py [--workload L|S] [--batches B] [--graphs uniform,powerlaw]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import WORKLOADS, synth
from rgb_experiment_amd import NeighborSampler, ops
from rgb_experiment_amd.graph import forget
from rgb_experiment_amd.models import GraphSAGE
from rgb_experiment_amd.models._stack import masked_ce

FANOUTS = ([25, 10], [10, 10, 10])
BATCH_SIZES = (1024, 8192)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run(tag, ei, x, y, N, batches, dev, res):
    deg = torch.bincount(ei[1], minlength=N)
    print(f"--- {tag}: {N} nodes, {ei.size(1)} edges, mean in-degree {ei.size(1) / N:.1f}, max {int(deg.max())}")
    gen = torch.Generator().manual_seed(99)
    for fanouts in FANOUTS:
        sampler = NeighborSampler(ei, N, fanouts)
        torch.manual_seed(7)
        net = GraphSAGE(num_layers=len(fanouts), hidden_unit=128, input_dim=x.size(1), output_dim=int(y.max()) + 1,
                        dropout_rate=0.5).to(dev).train()
        opt = torch.optim.Adam(net.parameters(), lr=0.01, capturable=True)
        for bs in BATCH_SIZES:
            t_s, t_t, n_e, n_n = [], [], [], []
            for b in range(batches + 1):
                seeds = torch.randperm(N, generator=gen)[:bs].to(dev)
                batch, ms_s = timed(lambda: sampler.sample(seeds, seed=(b, 17)))

                def step():
                    x_b = ops.gather_rows(x, batch.n_id.to(torch.int32))
                    y_b = y[batch.n_id]
                    rows = torch.arange(batch.n_id.numel(), device=dev) < batch.num_seeds
                    opt.zero_grad()
                    loss, _ = masked_ce(net, {"x": x_b, "edge_index": batch.edge_index}, y_b, rows)
                    loss.backward()
                    opt.step()
                _, ms_t = timed(step)
                forget(batch.edge_index)  # as experiment() does: no pile of batch graphs in the cache
                if b:  # the first batch warms code objects and the allocator
                    t_s.append(ms_s), t_t.append(ms_t), n_e.append(batch.e_id.numel()), n_n.append(batch.n_id.numel())
            ms_s, ms_t = statistics.median(t_s), statistics.median(t_t)
            eps = statistics.median(n_e) / (ms_s * 1e-3)
            key = f"{tag}/{'-'.join(map(str, fanouts))}/bs{bs}"
            print(f"{key:34s} sample {ms_s:8.3f} ms (min {min(t_s):.3f}, max {max(t_s):.3f})   step {ms_t:8.3f} ms "
                  f"(min {min(t_t):.3f}, max {max(t_t):.3f})   nodes {int(statistics.median(n_n)):8d}  edges "
                  f"{int(statistics.median(n_e)):9d}   {eps / 1e6:8.1f} M sampled edges/s   sampling is "
                  f"{'BELOW' if ms_s < ms_t else 'ABOVE'} the step ({ms_s / ms_t:.2f}x)")
            res[key] = {"sample_ms": round(ms_s, 3), "step_ms": round(ms_t, 3), "edges": int(statistics.median(n_e)),
                        "nodes": int(statistics.median(n_n)), "sampled_edges_per_s": round(eps),
                        "sampling_below_step": ms_s < ms_t}
        del sampler, net, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--graphs", default="uniform,powerlaw")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E, d = wl["N"], wl["E"], wl["d"]
    dev = torch.device("cuda:0")
    res = {"workload": args.workload, "N": N, "E": E, "d": d, "batches": args.batches}
    for degree in args.graphs.split(","):
        ei, x, y = synth(N, E, d, degree)
        from rgb_experiment_amd import graph
        graph.clear_cache()
        torch.cuda.empty_cache()
        run(degree, ei.to(dev), x.to(dev), y.to(dev), N, args.batches, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
