#!/usr/bin/env python3
"""GINEConv's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at C = 64 and C = 128, next
to two yardsticks in the SAME run: ResGatedGraphConv's kernels at the same C — two C-wide rows per slot as well, both
gathered, with an expf and a division per element — and the plain sum aggregation (ops.propagate_sum: one gathered row
per slot). The forms run alternately in one process; every launch is timed with HIP events on its stream
(ops.set_event_sink) and the median per launch kind, after one warm-up call of every form, is reported:
  gine_fwd (no_grad form and the grad-recording one: the same kernel), gine_bwd_edge, gine_bwd_src,
  resgated_fwd / resgated_bwd_dst / resgated_bwd_src, sum_fwd.
The GINE forms run TWICE per round under two names (A and A'): the ratio of their medians is the tool's A/A spread, which
a GINE / ResGated ratio has to be read against. x is one [N, C] matrix, e one [E, C] matrix in slot order (what the
layer's lin produces); k, q, v are the column blocks of one [N, 3 C] matrix. All forms take the edges as given (E slots).

Byte model (fp32, E slots, N rows; index traffic included):
  gine forward       an x row gathered and an e row streamed per slot:        E (8 C + 4) + 8 N C + 4 N   (x root read, out
                                                                                                            written, rowptr)
  gine edge pass     x gathered, e streamed, g_e stored per slot:             E (12 C + 4) + 4 N C         (gout read)
  gine source pass   a gout row and an e row gathered per slot, t2f and col:  E (8 C + 8) + 12 N C         (x, gout root
                                                                                                            read, g_x written)
  resgated_*         tools/resgated_bench.py's model
  sum_fwd            a row per slot:                                          E (4 C + 4) + N (4 C + 4)
Each is reported as ms and as a fraction of 8 TB/s. e and g_e are E x C floats each (30.7 GB at L and C = 128): a width
runs only when three such matrices and the node-side operands fit the free memory, and the tool says which widths it
ran. Prints a table, then one JSON line.
Usage: python tools/gine_bench.py [--rounds R] [--workload L|S]"""
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

PEAK = 8e12  # HBM bytes / s
WIDTHS = [64, 128]
PAIRS = (("gine_fwd", "resgated_fwd"), ("gine_bwd_src", "resgated_bwd_src"))
KINDS = ("gine_", "resgated_", "sum_fwd")


def byte_model(kind, nnz, N, C):
    return {
        "gine_fwd": nnz * (8 * C + 4) + 8 * N * C + 4 * N,
        "gine_bwd_edge": nnz * (12 * C + 4) + 4 * N * C,
        "gine_bwd_src": nnz * (8 * C + 8) + 12 * N * C,
        "resgated_fwd": nnz * (8 * C + 4) + N * (2 * 4 * C + 4),
        "resgated_bwd_dst": nnz * (8 * C + 4) + N * (3 * 4 * C + 4),
        "resgated_bwd_src": nnz * (8 * C + 4) + N * (4 * 4 * C + 4),
        "sum_fwd": nnz * (4 * C + 4) + N * (4 * C + 4),
    }[kind]


def bytes_needed(nnz, N, C):
    """e, its gradient and one more [E, C] block the allocator may still hold, plus the node-side matrices."""
    return 3 * nnz * C * 4 + 12 * N * C * 4 + (2 << 30)


def run_width(C, N, graph, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, 3 * C, device=dev) * 0.5
    x = h[:, :C].contiguous()
    e = torch.randn(nnz, C, device=dev) * 0.5
    eps = torch.full((1,), 0.1, device=dev)
    cot = torch.randn(N, C, device=dev)
    h_g = h.clone().requires_grad_(True)
    x_g, e_g = x.clone().requires_grad_(True), e.requires_grad_(True)
    blocks = lambda t: (t[:, :C], t[:, C:2 * C], t[:, 2 * C:])

    def gine_eval():
        with torch.no_grad():
            ops.gine_aggregate(x, e, graph, eps)

    def gine_step():
        x_g.grad = e_g.grad = None
        ops.gine_aggregate(x_g, e_g, graph, eps).backward(cot)

    def rg_eval():
        with torch.no_grad():
            ops.resgated_aggregate(*blocks(h), graph)

    def rg_step():
        h_g.grad = None
        ops.resgated_aggregate(*blocks(h_g), graph).backward(cot)

    def plain_sum():
        with torch.no_grad():
            ops.propagate_sum(x, graph)

    forms = {"gine_eval": gine_eval, "gine_step": gine_step, "resgated_eval": rg_eval, "resgated_step": rg_step,
             "gine_eval'": gine_eval, "gine_step'": gine_step, "sum": plain_sum}
    for fn in forms.values():  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    times = {}
    for _ in range(rounds):  # alternately, so drift in clocks or neighbours hits all forms alike
        for form, fn in forms.items():
            sink = []
            ops.set_event_sink(sink)
            fn()
            ops.set_event_sink(None)
            torch.cuda.synchronize()
            for kind, s, t in sink:
                if str(kind).startswith(KINDS):
                    times.setdefault(f"{form}/{kind}", []).append(s.elapsed_time(t))
    print(f"--- C = {C}; slots {nnz}, rows {N}; every figure below measured in this run")
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        nb = byte_model(key.split("/", 1)[1], nnz, N, C)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:36s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"C{C}/{key}_ms"] = round(ms, 3)
        res[f"C{C}/{key}_frac_8TBs"] = round(frac, 3)
    for kind, form in (("gine_fwd", "eval"), ("gine_bwd_edge", "step"), ("gine_bwd_src", "step")):
        a, a2 = med[f"gine_{form}/{kind}"], med[f"gine_{form}'/{kind}"]
        print(f"A/A of {kind}: {a2 / a:.3f}")
        res[f"C{C}/{kind}_A_over_A"] = round(a2 / a, 3)
    for mine, theirs in PAIRS:
        form = "eval" if mine.endswith("fwd") else "step"
        a, a2, b = med[f"gine_{form}/{mine}"], med[f"gine_{form}'/{mine}"], med[f"resgated_{form}/{theirs}"]
        spread = abs(a2 / a - 1)
        verdict = "met" if a / b <= 1 + spread else "MISSED"
        print(f"{mine} / {theirs}: {a / b:.3f}   (expected: at most 1 + the A/A spread = {1 + spread:.3f}: {verdict}; "
              f"over sum_fwd: {a / med['sum/sum_fwd']:.2f}x)")
        res[f"C{C}/{mine}_over_{theirs}"] = round(a / b, 3)
        res[f"C{C}/{mine}_expectation"] = verdict
        res[f"C{C}/{mine}_over_sum_fwd"] = round(a / med["sum/sum_fwd"], 2)
    print(f"gine_bwd_edge over sum_fwd: {med['gine_step/gine_bwd_edge'] / med['sum/sum_fwd']:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gine_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f  # once per graph: not part of a step
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds, "widths_run": []}
    for C in WIDTHS:
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(dev)[0]
        need = bytes_needed(graph.fwd.nnz, N, C)
        if need > free:
            print(f"--- C = {C}: skipped, {need / 1e9:.1f} GB needed, {free / 1e9:.1f} GB free")
            continue
        print(f"--- C = {C}: {need / 1e9:.1f} GB needed, {free / 1e9:.1f} GB free")
        run_width(C, N, graph, args.rounds, dev, res)
        res["widths_run"].append(C)
    print(f"widths run: {res['widths_run']} of {WIDTHS}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
