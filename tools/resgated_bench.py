#!/usr/bin/env python3
"""ResGatedGraphConv's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at C = 64 and
C = 128, next to two yardsticks in the SAME run: TransformerConv's three kernels at (H = 1, C) — the same two-row gather
per slot, with strictly more arithmetic and a cross-lane reduction — and the plain weighted SpMM at width C (one row
per slot). The forms run alternately in one process; every launch is timed with HIP events on its stream
(ops.set_event_sink) and the median per launch kind is reported:
  resgated_fwd (no_grad form and the grad-recording one: the same kernel), resgated_bwd_dst, resgated_bwd_src,
  transformer_fwd / transformer_bwd_dst / transformer_bwd_src, spmm_weighted.
The transformer forms run TWICE per round under two names (A and A'): the ratio of their medians is the A/A spread a
ResGated / Transformer ratio has to be read against. k, q and v are the column blocks of one [N, 3 C] matrix, as the
layers hand them over. All forms take the edges as given (E slots).

Byte model (fp32, E slots, N rows; index traffic included):
  resgated forward      a q row and a v row per slot:     E (8 C + 4) + N (2 * 4 C + 4)    (k read, out written)
  resgated target pass  a q row and a v row per slot:     E (8 C + 4) + N (3 * 4 C + 4)    (k, gout read, g_k written)
  resgated source pass  a k row and a gout row per slot:  E (8 C + 4) + N (4 * 4 C + 4)    (q, v read, g_q, g_v written)
  transformer_*         tools/transformer_bench.py's model at H = 1, no dropout
  spmm_weighted         a row and a weight per slot:      E (4 C + 8) + N (4 C + 4)
Each is reported as ms and as a fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/resgated_bench.py [--rounds R] [--workload L|S]"""
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
PAIRS = (("resgated_fwd", "transformer_fwd"), ("resgated_bwd_dst", "transformer_bwd_dst"),
         ("resgated_bwd_src", "transformer_bwd_src"))


def byte_model(kind, nnz, N, C):
    return {
        "resgated_fwd": nnz * (8 * C + 4) + N * (2 * 4 * C + 4),
        "resgated_bwd_dst": nnz * (8 * C + 4) + N * (3 * 4 * C + 4),
        "resgated_bwd_src": nnz * (8 * C + 4) + N * (4 * 4 * C + 4),
        "transformer_fwd": nnz * (8 * C + 4) + N * (2 * 4 * C + 8 + 4),
        "transformer_bwd_dst": nnz * (8 * C + 4) + N * (4 * 4 * C + 16 + 4),
        "transformer_bwd_src": nnz * (8 * C + 8 + 4) + N * (4 * 4 * C + 4),
        "spmm_weighted": nnz * (4 * C + 8) + N * (4 * C + 4),
    }[kind]


def run_width(C, N, graph, rounds, dev, res):
    torch.manual_seed(0)
    h = torch.randn(N, 3 * C, device=dev) * 0.5
    cot = torch.randn(N, C, device=dev)
    out = torch.empty(N, C, device=dev)
    h_g = h.clone().requires_grad_(True)
    blocks = lambda t: (t[:, :C], t[:, C:2 * C], t[:, 2 * C:])

    def rg_eval():
        with torch.no_grad():
            ops.resgated_aggregate(*blocks(h), graph)

    def rg_step():
        h_g.grad = None
        ops.resgated_aggregate(*blocks(h_g), graph).backward(cot)

    def tf_eval():
        with torch.no_grad():
            ops.transformer_attend(*blocks(h), graph, 1, C, C ** -0.5)

    def tf_step():
        h_g.grad = None
        ops.transformer_attend(*blocks(h_g), graph, 1, C, C ** -0.5).backward(cot)

    forms = {"resgated_eval": rg_eval, "resgated_step": rg_step, "transformer_eval": tf_eval,
             "transformer_step": tf_step, "transformer_eval'": tf_eval, "transformer_step'": tf_step,
             "spmm": lambda: ops.spmm_raw(graph.fwd, graph.w, None, h[:, :C], out=out, kind="spmm_weighted")}
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
            for kind, s, e in sink:
                if str(kind).startswith(("resgated_", "transformer_", "spmm_weighted")):
                    times.setdefault(f"{form}/{kind}", []).append(s.elapsed_time(e))
    nnz = graph.fwd.nnz
    print(f"--- C = {C}; slots {nnz}, rows {N}")
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        nb = byte_model(key.split("/", 1)[1], nnz, N, C)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:42s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"C{C}/{key}_ms"] = round(ms, 3)
        res[f"C{C}/{key}_frac_8TBs"] = round(frac, 3)
    for mine, theirs in PAIRS:
        form = "eval" if mine.endswith("fwd") else "step"
        a, b, b2 = (med[f"resgated_{form}/{mine}"], med[f"transformer_{form}/{theirs}"],
                    med[f"transformer_{form}'/{theirs}"])
        print(f"{mine} / {theirs}: {a / b:.3f}   (A/A of {theirs}: {b2 / b:.3f}; over spmm_weighted: "
              f"{a / med['spmm/spmm_weighted']:.2f}x)")
        res[f"C{C}/{mine}_over_transformer"] = round(a / b, 3)
        res[f"C{C}/{theirs}_A_over_A"] = round(b2 / b, 3)
        res[f"C{C}/{mine}_over_spmm_weighted"] = round(a / med["spmm/spmm_weighted"], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resgated_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.w  # once per graph: not part of a step
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds}
    for C in WIDTHS:
        run_width(C, N, graph, args.rounds, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
