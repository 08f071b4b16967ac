#!/usr/bin/env python3
"""SuperGAT on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M, F = 128) at H = 8, C = 8, forms run
alternately in one process, timed with HIP events, medians reported:
  1. the eval forward of one layer (rgbx_supergat_aggregate_fwd_f32) next to rgbx_gat_aggregate_fwd_f32 at the same
     H, C on the same graph — the same bytes, E' (H C 4 + 4) + N (2 H C 4 + 4) — as ms and as a fraction of 8 TB/s;
  2. a training step of one layer (forward + sampler + loss + both backward passes) with the attention loss in the
     kernels, next to the same step with the loss composed from torch index ops on the sampled edge lists
     ([n, H, C] gathers; the kernels then run with edge_sample_ratio = 0 and no negatives);
  3. the default SuperGAT epoch (training forward + backward + Adam step, eval forward).
Prints a table, then one JSON line. Usage: python tools/supergat_bench.py [--rounds R] [--reps K] [--workload L|S]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import WORKLOADS, synth
from rgb_experiment_amd import ops
from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
from rgb_experiment_amd.models import SuperGAT

PEAK = 8e12  # HBM bytes / s


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    wl = WORKLOADS[args.workload]
    N, E, F = wl["N"], wl["E"], wl["d"]
    H, C, n_cls, p, ratio, nratio = 8, 8, 16, 0.6, 0.8, 0.5
    dev = torch.device("cuda:0")
    ei, x, y = synth(N, E, F)
    ei, x, y = ei.to(dev), x.to(dev), (y % n_cls).to(dev)
    graph = get_graph(ei, N, LOOPS_REMOVE_ADD)
    nnz = graph.fwd.nnz
    graph.undirected_keys, graph.t2f  # once per graph: not part of a step
    torch.manual_seed(0)
    h0 = (torch.randn(N, H * C, device=dev) * 0.3)
    att = [torch.randn(1, H, C, device=dev) * 0.3 for _ in range(2)]
    bias = torch.zeros(H * C, device=dev)

    def eval_sgat():
        with torch.no_grad():
            return ops.supergat_attend(h0, att[0], att[1], graph, H, C, bias=bias)[0]

    def eval_gat():
        with torch.no_grad():
            return ops.gat_attend(h0, att[0], att[1], graph, H, C, bias=bias)

    hg = h0.clone().requires_grad_(True)
    ag = [a.clone().requires_grad_(True) for a in att]
    cot = torch.randn(N, H * C, device=dev)

    def train_fused():
        hg.grad = None
        out, loss = ops.supergat_attend(hg, ag[0], ag[1], graph, H, C, bias=bias, training=True, p_drop=p,
                                        pos_ratio=ratio, neg_ratio=nratio)
        ((out * cot).sum() + 4 * loss).backward()

    src = graph.fwd.col[:nnz].long()
    deg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(N, device=dev), deg)
    none = torch.empty((2, 0), dtype=torch.int64, device=dev)

    def train_composed():
        hg.grad = None
        out, _ = ops.supergat_attend(hg, ag[0], ag[1], graph, H, C, bias=bias, training=True, p_drop=p, pos_ratio=0.0,
                                     neg_ratio=0.0, neg_edge_index=none)
        keep = torch.rand(nnz, device=dev) < ratio
        seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
        neg, valid = ops.supergat_sample_negatives(graph, seed, int(nratio * ratio * nnz))
        h3 = hg.view(N, H, C)
        pos = (h3[src[keep]] * h3[dst[keep]]).sum(-1).mean(-1)
        ng = (h3[neg[0]] * h3[neg[1]]).sum(-1).mean(-1)[valid.bool()]
        logits = torch.cat([pos, ng])
        labels = torch.cat([torch.ones_like(pos), torch.zeros_like(ng)])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
        ((out * cot).sum() + 4 * loss).backward()

    model = SuperGAT(input_dim=F, output_dim=n_cls, hidden_dim=C, heads=H, dropout_rate=p, edge_sample_ratio=ratio,
                     neg_sample_ratio=nratio).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    train_mask = torch.rand(N, device=dev) < 0.6

    def epoch():
        model.train()
        opt.zero_grad()
        res = model(x, ei)
        (torch.nn.functional.nll_loss(res["out"][train_mask], y[train_mask]) + 4 * res["att_loss"]).backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            model(x, ei)

    forms = {"sgat_eval_fwd": eval_sgat, "gat_eval_fwd": eval_gat, "train_step_fused_loss": train_fused,
             "train_step_composed_loss": train_composed, "epoch": epoch}
    for fn in forms.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):  # alternately, so drift in clocks or neighbours hits all forms alike
        for k, fn in forms.items():
            times[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    nb = nnz * (H * C * 4 + 4) + N * (2 * H * C * 4 + 4)
    res = {"workload": args.workload, "N": N, "nnz": nnz, "H": H, "C": C, "eval_fwd_GB": round(nb / 1e9, 2)}
    for k, ms in med.items():
        res[f"{k}_ms"] = round(ms, 3)
        print(f"{k:26s} {ms:9.3f} ms" + (f"  {nb / (ms * 1e-3) / PEAK:.3f} of 8 TB/s" if k.endswith("eval_fwd") else ""))
    res["sgat_eval_frac_8TBs"] = round(nb / (med["sgat_eval_fwd"] * 1e-3) / PEAK, 3)
    res["gat_eval_frac_8TBs"] = round(nb / (med["gat_eval_fwd"] * 1e-3) / PEAK, 3)
    res["sgat_over_gat_eval_fwd"] = round(med["sgat_eval_fwd"] / med["gat_eval_fwd"], 3)
    print(f"eval forward, SuperGAT / GAT: {res['sgat_over_gat_eval_fwd']:.3f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
