#!/usr/bin/env python3
"""GATv2's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at H = 8, C = 8, next to
GATConv's kernels at the same H, C on the same graph as the yardstick. The forms run alternately in one process; every
launch is timed with HIP events on its stream (ops.set_event_sink) and the median per launch kind is reported:
  gatv2_fwd (eval form, and the training form with attention dropout p = 0.5), gatv2_bwd_dst, gatv2_bwd_src,
  and whatever kinds ops.gat_attend launches for its forward and backward.

Byte model (fp32, F = H C, E' slots, N rows; index and per-(row, head) scalar traffic included):
  forward       one x_l row per slot:        E' (4 F + 4) + N (2 * 4 F + 8 H + 4)   -- the bytes of GAT's aggregation
  target pass   one x_l row per slot:        E' (4 F + 4) + N (4 * 4 F + 16 H + 4)
  source pass   two rows (x_r, gout) + the (shift, D) record per slot:  E' (8 F + 8 H + 4 [+ 4 with dropout]) + N (2 * 4 F + 4)
Each is reported as ms and as a fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/gatv2_bench.py [--rounds R] [--workload L|S]"""
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

PEAK = 8e12  # HBM bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gatv2_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    H, C, p = 8, 8, 0.5
    F = H * C
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_REMOVE_ADD)
    nnz = graph.fwd.nnz
    graph.t2f  # once per graph: not part of a step
    torch.manual_seed(0)
    xl = torch.randn(N, F, device=dev) * 0.5
    xr = torch.randn(N, F, device=dev) * 0.5
    att = torch.randn(1, H, C, device=dev) * 0.3
    att2 = torch.randn(1, H, C, device=dev) * 0.3
    bias = torch.zeros(F, device=dev)
    cot = torch.randn(N, F, device=dev)
    xl_g, xr_g, att_g = (t.clone().requires_grad_(True) for t in (xl, xr, att))
    att2_g = att2.clone().requires_grad_(True)

    def v2_eval():
        with torch.no_grad():
            ops.gatv2_attend(xl, xr, att, graph, H, C, bias=bias)

    def v2_step(training):
        for t in (xl_g, xr_g, att_g):
            t.grad = None
        out = ops.gatv2_attend(xl_g, xr_g, att_g, graph, H, C, bias=bias, training=training, p_drop=p)
        out.backward(cot)

    def gat_eval():
        with torch.no_grad():
            ops.gat_attend(xl, att, att2, graph, H, C, bias=bias)

    def gat_step():
        for t in (xl_g, att_g, att2_g):
            t.grad = None
        ops.gat_attend(xl_g, att_g, att2_g, graph, H, C, bias=bias).backward(cot)

    forms = {"gatv2_eval": v2_eval, "gatv2_step": lambda: v2_step(False), "gatv2_step_dropout": lambda: v2_step(True),
             "gat_eval": gat_eval, "gat_step": gat_step}
    for fn in forms.values():  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    times = {}
    for _ in range(args.rounds):  # alternately, so drift in clocks or neighbours hits all forms alike
        for form, fn in forms.items():
            sink = []
            ops.set_event_sink(sink)
            fn()
            ops.set_event_sink(None)
            torch.cuda.synchronize()
            for kind, s, e in sink:
                times.setdefault(f"{form}/{kind}", []).append(s.elapsed_time(e))
    model = {
        "gatv2_fwd": nnz * (4 * F + 4) + N * (2 * 4 * F + 8 * H + 4),
        "gatv2_bwd_dst": nnz * (4 * F + 4) + N * (4 * 4 * F + 16 * H + 4),
        "gatv2_bwd_src": nnz * (8 * F + 8 * H + 4) + N * (2 * 4 * F + 4),
    }
    res = {"workload": args.workload, "N": N, "nnz": nnz, "H": H, "C": C, "rounds": args.rounds}
    for key in sorted(times):
        v = times[key]
        ms = statistics.median(v)
        kind = key.split("/", 1)[1]
        nb = model.get(kind)
        if nb is not None and key.startswith("gatv2_step_dropout") and kind == "gatv2_bwd_src":
            nb += 4 * nnz  # the slot map
        frac = "" if nb is None else f"  {nb / 1e9:6.2f} GB  {nb / (ms * 1e-3) / PEAK:.3f} of 8 TB/s"
        print(f"{key:44s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)}){frac}")
        res[key + "_ms"] = round(ms, 3)
        if nb is not None:
            res[key + "_frac_8TBs"] = round(nb / (ms * 1e-3) / PEAK, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
