#!/usr/bin/env python3
"""GGNN on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M, F = 128): the default GGNN epoch (C = 64,
2 steps: one training forward + backward + Adam step and one eval forward) and one GatedGraphConv step in the fused
and the composed form (csrc/gru.hip), run alternately in the same process, timed with HIP events. Prints the
algorithmic bytes of each step form and their fraction of 8 TB/s, then one JSON line.
Usage: python tools/ggnn_bench.py [--rounds R] [--reps K] [--workload L|S] [--epoch-only]"""
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
from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
from rgb_experiment_amd.models import GGNN

PEAK = 8e12  # HBM bytes / s


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def step_bytes(N, nnz, C, form, train):
    """Algorithmic bytes of one step: CSR, gathered rows, own rows, output; the training forward adds the stored
    aggregate and pre. The composed form adds the [N, 4C] pre round trip (written by the aggregating kernel, read by the
    gate kernel) and the gate kernel's second read of the own rows."""
    f = 4
    b = (N + 1) * 4 + nnz * 4 + nnz * C * f + N * C * f + N * C * f
    if train:
        b += N * C * f + N * 4 * C * f  # z, pre
    if form == "composed":
        b += N * C * f  # the gate kernel reads the own rows again
        b += N * 4 * C * f if train else 2 * N * 4 * C * f  # training: pre is written anyway, read once more
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epoch-only", action="store_true", help="time the epoch alone (for a kernel-trace run)")
    args = ap.parse_args()
    wl = WORKLOADS[args.workload]
    N, E, F = wl["N"], wl["E"], wl["d"]
    C, L, n_cls = 64, 2, 16
    dev = torch.device("cuda:0")
    ei, x, y = synth(N, E, F)
    ei, x, y = ei.to(dev), x.to(dev), (y % n_cls).to(dev)
    graph = get_graph(ei, N, LOOPS_KEEP)
    nnz = graph.fwd.nnz

    torch.manual_seed(0)
    model = GGNN(num_layers=L, hidden_unit=C, input_dim=F, output_dim=n_cls, dropout_rate=0.5).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    train_mask = torch.rand(N, device=dev) < 0.6

    def epoch():
        model.train()
        opt.zero_grad()
        out = model(x, ei)["out"]
        torch.nn.functional.nll_loss(out[train_mask], y[train_mask]).backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            model(x, ei)

    if args.epoch_only:
        epoch()
        torch.cuda.synchronize()
        ms = statistics.median(timed(epoch, args.reps) for _ in range(args.rounds))
        print(json.dumps({"workload": args.workload, "N": N, "nnz": nnz, "C": C, "steps": L, "epoch_ms": round(ms, 3),
                          "default_form": ops.gru_step_form(C)}))
        return

    conv = model.conv
    h = torch.randn(N, C, device=dev)
    with torch.no_grad():
        ops_args = ops.gru_operands(conv.weight[0], conv.rnn.weight_ih, conv.rnn.weight_hh, conv.rnn.bias_ih,
                                    conv.rnn.bias_hh, C)

    def step(form, train):
        return lambda: ops.gru_step_raw(h, graph, *ops_args, form, want_saved=train)

    # same numbers from both forms before anything is timed
    a, b = step("fused", False)()[0], step("composed", False)()[0]
    agree = (a - b).abs().max().item()

    epoch()
    for form in ("fused", "composed"):
        step(form, True)()
    torch.cuda.synchronize()
    times = {k: [] for k in ("epoch", "fused_eval", "composed_eval", "fused_train", "composed_train")}
    for _ in range(args.rounds):  # alternately, so drift in clocks or neighbours hits both forms alike
        times["epoch"].append(timed(epoch, args.reps))
        for form in ("fused", "composed"):
            times[f"{form}_eval"].append(timed(step(form, False), args.reps))
            times[f"{form}_train"].append(timed(step(form, True), args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"workload": args.workload, "N": N, "nnz": nnz, "C": C, "steps": L, "epoch_ms": round(med["epoch"], 3),
           "max_abs_fused_vs_composed": agree, "default_form": ops.gru_step_form(C)}
    for form in ("fused", "composed"):
        for mode, train in (("eval", False), ("train", True)):
            ms = med[f"{form}_{mode}"]
            nb = step_bytes(N, nnz, C, form, train)
            res[f"{form}_{mode}_ms"] = round(ms, 3)
            res[f"{form}_{mode}_GB"] = round(nb / 1e9, 2)
            res[f"{form}_{mode}_frac_8TBs"] = round(nb / (ms * 1e-3) / PEAK, 3)
            print(f"step {form:8s} {mode:5s}: {ms:7.3f} ms  {nb / 1e9:6.2f} GB  {nb / (ms * 1e-3) / PEAK:.3f} of 8 TB/s")
    print(f"epoch (train fwd+bwd+Adam, eval fwd): {med['epoch']:.3f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
