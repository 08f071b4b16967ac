#!/usr/bin/env python3
"""CGConv's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at C = 64, with and without
the edge term, next to two yardsticks in the SAME run: rgbx_resgated_fwd_f32 at the same C — the same 2 C floats gathered
per slot, ONE transcendental per channel and slot — and rgbx_gine_fwd_f32 — one gathered row and one streamed per-slot
row, no transcendental. The forms run alternately in one process; every launch is timed with HIP events on its stream
(ops.set_event_sink) and the median per launch kind, after one warm-up call of every form, is reported:
  cgconv_fwd (no_grad form and the grad-recording one: the same kernel), cgconv_bwd_dst (g_a and, with the edge term,
  g_c from the same registers), cgconv_bwd_src, each with (`edge`) and without (`plain`) c; resgated_fwd; gine_fwd.
The edge forward runs TWICE per round under two names (A and A'): the ratio of their medians is the tool's A/A spread,
which every ratio below has to be read against. a and b are the column blocks of one [N, 4 C] matrix (what the layer's
product yields), c one [E, 2 C] matrix in slot order, root one [N, C] matrix. aggr = "mean", so the in-kernel degree reads
are in the timing. All forms take the edges as given (E slots).

Byte model (fp32, E slots, N rows; index traffic included; `edge` forms; the `plain` forms drop the c and g_c terms):
  cgconv forward      both halves of b gathered, a c row streamed per slot:      E (8 C + 8 C + 4) + N (8 C + 4 C + 4 C + 4)
                                                                                  (a and root read, out written, rowptr)
  cgconv target pass  the same reads, a g_c row stored per slot:                 E (8 C + 8 C + 8 C + 4) + N (8 C + 4 C + 8 C + 4)
                                                                                  (a, gout read, g_a written)
  cgconv source pass  a, gout and c rows gathered per slot, col, t2f, 2 rowptr:  E (8 C + 4 C + 8 C + 16) + N (8 C + 8 C + 4)
                                                                                  (b read, g_b written)
  resgated_fwd        tools/resgated_bench.py's model: E (8 C + 4) + N (8 C + 4)
  gine_fwd            tools/gine_bench.py's model:     E (8 C + 4) + 8 N C + 4 N
Each is reported as ms and as a fraction of 8 TB/s. The transcendental work per channel and slot is two expf, one log1pf
and one division forward (a second division backward): whether that leaves the kernels memory-bound is what this tool
measures; nothing is assumed. c alone is E x 2 C floats (30.7 GB at L and C = 64) and g_c as much again: the tool prints
the footprint and runs only if it fits the free memory. Prints a table, then one JSON line.
Usage: python tools/cgconv_bench.py [--rounds R] [--workload L|S] [--channels C]"""
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
KINDS = ("cgconv_", "resgated_fwd", "gine_fwd")


def byte_model(kind, edge, nnz, N, C):
    c_row = 8 * C if edge else 0
    return {
        "cgconv_fwd": nnz * (8 * C + c_row + 4) + N * (16 * C + 4),
        "cgconv_bwd_dst": nnz * (8 * C + 2 * c_row + 4) + N * (20 * C + 4),
        "cgconv_bwd_src": nnz * (12 * C + c_row + 12 + (4 if edge else 0)) + N * (16 * C + 4),
        "resgated_fwd": nnz * (8 * C + 4) + N * (8 * C + 4),
        "gine_fwd": nnz * (8 * C + 4) + 8 * N * C + 4 * N,
    }[kind]


def bytes_needed(nnz, N, C):
    """c, g_c, gine's [E, C] row matrix and one more [E, 2C] block the allocator may still hold, plus the node side."""
    return 3 * nnz * 2 * C * 4 + nnz * C * 4 + 24 * N * C * 4 + (2 << 30)


def run(C, N, graph, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, 4 * C, device=dev) * 0.5
    c = torch.randn(nnz, 2 * C, device=dev) * 0.5
    root = torch.randn(N, C, device=dev)
    cot = torch.randn(N, C, device=dev)
    eps = torch.full((1,), 0.1, device=dev)
    h_g = h.clone().requires_grad_(True)
    c_g = c.requires_grad_(True)
    ab = lambda t: (t[:, :2 * C], t[:, 2 * C:])

    def cg_eval(edge):
        def fn():
            with torch.no_grad():
                ops.cgconv_aggregate(*ab(h), c if edge else None, graph, C, "mean", root=root)
        return fn

    def cg_step(edge):
        def fn():
            h_g.grad = c_g.grad = None
            ops.cgconv_aggregate(*ab(h_g), c_g if edge else None, graph, C, "mean", root=root).backward(cot)
        return fn

    def rg_eval():  # k, q, v: three C-wide column blocks of h
        with torch.no_grad():
            ops.resgated_aggregate(h[:, :C], h[:, C:2 * C], h[:, 2 * C:3 * C], graph)

    def gine_eval():  # x: a C-wide block of h; e: the f half of c (a column block of a wider matrix)
        with torch.no_grad():
            ops.gine_aggregate(h[:, :C], c[:, :C], graph, eps)

    forms = {"edge_eval": cg_eval(True), "edge_step": cg_step(True), "plain_eval": cg_eval(False),
             "plain_step": cg_step(False), "resgated_eval": rg_eval, "gine_eval": gine_eval, "edge_eval'": cg_eval(True)}
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
    print(f"--- C = {C}; slots {nnz}, rows {N}; aggr = mean; every figure below measured in this run")
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        form, kind = key.split("/", 1)
        nb = byte_model(kind, form.startswith("edge"), nnz, N, C)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:36s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"C{C}/{key}_ms"] = round(ms, 3)
        res[f"C{C}/{key}_frac_8TBs"] = round(frac, 3)
    aa = med["edge_eval'/cgconv_fwd"] / med["edge_eval/cgconv_fwd"]
    print(f"A/A of cgconv_fwd (edge): {aa:.3f}")
    res[f"C{C}/cgconv_fwd_A_over_A"] = round(aa, 3)
    rg, gi = med["resgated_eval/resgated_fwd"], med["gine_eval/gine_fwd"]
    for form in ("plain", "edge"):
        f = med[f"{form}_eval/cgconv_fwd"]
        print(f"cgconv_fwd ({form}) over resgated_fwd: {f / rg:.3f}x, over gine_fwd: {f / gi:.3f}x")
        res[f"C{C}/cgconv_fwd_{form}_over_resgated_fwd"] = round(f / rg, 3)
        res[f"C{C}/cgconv_fwd_{form}_over_gine_fwd"] = round(f / gi, 3)
    for kind in ("cgconv_fwd", "cgconv_bwd_dst", "cgconv_bwd_src"):
        form = "eval" if kind.endswith("fwd") else "step"
        e, p = med[f"edge_{form}/{kind}"], med[f"plain_{form}/{kind}"]
        print(f"{kind}: the c stream's share of the edge form's time: {1 - p / e:.3f}")
        res[f"C{C}/{kind}_c_share"] = round(1 - p / e, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--channels", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cgconv_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E, C = wl["N"], wl["E"], args.channels
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f  # once per graph: not part of a step
    nnz = graph.fwd.nnz
    res = {"workload": args.workload, "N": N, "slots": nnz, "rounds": args.rounds, "C": C, "ran": False}
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    need = bytes_needed(nnz, N, C)
    print(f"--- C = {C}: c is {nnz} x {2 * C} floats = {nnz * 2 * C * 4 / 1e9:.1f} GB, g_c as much again; "
          f"{need / 1e9:.1f} GB needed in all, {free / 1e9:.1f} GB free")
    if need > free:
        print(f"--- C = {C}: skipped, it does not fit")
    else:
        run(C, N, graph, args.rounds, dev, res)
        res["ran"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
