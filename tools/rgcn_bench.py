#!/usr/bin/env python3
"""RGCNConv's aggregation on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) with seeded edge types, at
R in {4, 32} relations, C = 64 channels and B in {2, 8} bases, next to two yardsticks in the SAME run: the GAT aggregation
forward at H = B heads of the same C — it gathers the same H * C row per slot and computes a softmax on top — and the
plain weighted SpMM at width C (one C-wide row per slot: what the select form's forward is). The forms run alternately in
one process; every launch is timed with HIP events on its stream (ops.set_event_sink) and the median per launch kind,
after one warm-up call of every form, is reported:
  rgcn_mix_fwd (no_grad form and the grad-recording one: the same kernel), rgcn_mix_bwd_src, rgcn_mix_bwd_coef,
  rgcn_comp_reduce, rgcn_select_fwd, rgcn_select_bwd, gat_fwd, spmm_w.
Every RGCN form runs TWICE per round under two names (A and A'): the ratio of their medians is the tool's A/A spread,
which an rgcn / gat ratio has to be read against.

Byte model (fp32, E slots, N rows; index traffic included; comp is cache-resident and not counted):
  rgcn_mix_fwd       a B * C row gathered per slot, col / type / weight:      E (4 B C + 12) + N (8 C + 4)   (y0 read, out
                                                                                                               written, rowptr)
  rgcn_mix_bwd_src   a gout row gathered per slot, col / type / weight:       E (4 C + 12) + N (4 B C + 4)
  rgcn_mix_bwd_coef  a B * C row gathered, B products stored per slot:        E (4 B C + 4 B + 8) + N (4 C + 4)
  rgcn_comp_reduce   the products read once, through the slot list:           E (4 B + 4)
  rgcn_select_fwd    a C row gathered per slot out of N * R rows:             E (4 C + 8) + N (8 C + 4)
  rgcn_select_bwd    the same over N * R rows:                                E (4 C + 8) + N R (4 C + 4)
  gat_fwd            an H * C row and H scores per slot:                      E (4 H C + 4 H + 4) + N (4 H C + 12 H + 4)
  spmm_w             a C row per slot, col / weight:                          E (4 C + 8) + N (4 C + 4)
Each is reported as ms and as a fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/rgcn_bench.py [--rounds R] [--workload L|S]"""
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
C = 64
RELATIONS = [4, 32]
BASES = [2, 8]
KINDS = ("rgcn_", "gat_fwd", "spmm_w")


def byte_model(kind, nnz, N, R, B):
    return {
        "rgcn_mix_fwd": nnz * (4 * B * C + 12) + N * (8 * C + 4),
        "rgcn_mix_bwd_src": nnz * (4 * C + 12) + N * (4 * B * C + 4),
        "rgcn_mix_bwd_coef": nnz * (4 * B * C + 4 * B + 8) + N * (4 * C + 4),
        "rgcn_comp_reduce": nnz * (4 * B + 4),
        "rgcn_select_fwd": nnz * (4 * C + 8) + N * (8 * C + 4),
        "rgcn_select_bwd": nnz * (4 * C + 8) + N * R * (4 * C + 4),
        "gat_fwd": nnz * (4 * B * C + 4 * B + 4) + N * (4 * B * C + 12 * B + 4),
        "spmm_w": nnz * (4 * C + 8) + N * (4 * C + 4),
    }[kind]


def measure(forms, rounds):
    for fn in forms.values():  # warm-up: code objects, allocator, the typed view's index sets
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
    return times


def report(times, nnz, N, R, B, tag, res):
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        nb = byte_model(key.split("/", 1)[1], nnz, N, R, B)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:36s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"{tag}/{key}_ms"] = round(ms, 3)
        res[f"{tag}/{key}_frac_8TBs"] = round(frac, 3)
    return med


def run_mix(R, B, N, graph, et, has_empty_rows, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, B * C, device=dev) * 0.5
    comp = torch.randn(R, B, device=dev) * 0.5
    y0 = torch.randn(N, C, device=dev)
    cot = torch.randn(N, C, device=dev)
    x = h[:, :C].contiguous()
    a_src, a_dst = torch.randn(N, B, device=dev), torch.randn(N, B, device=dev)
    h_g, comp_g = h.clone().requires_grad_(True), comp.clone().requires_grad_(True)
    view = ops.typed_view(graph, et, R)

    def mix_eval():
        with torch.no_grad():
            ops.rgcn_aggregate(h, graph, et, R, comp=comp, y0=y0)

    def mix_step():
        h_g.grad = comp_g.grad = None
        ops.rgcn_aggregate(h_g, graph, et, R, comp=comp_g, y0=y0).backward(cot)

    def gat_eval():
        with torch.no_grad():
            ops.gat_aggregate(h, a_src, a_dst, graph, B, C)

    def spmm_w():
        ops.spmm_raw(graph.fwd, view.w_f, None, x, kind="spmm_w")

    forms = {"mix_eval": mix_eval, "mix_step": mix_step, "mix_eval'": mix_eval, "mix_step'": mix_step, "spmm": spmm_w}
    if not has_empty_rows:  # the GAT kernels run on graphs with self-loops: every row has a slot
        forms["gat_eval"] = gat_eval
    tag = f"R{R}/B{B}"
    print(f"--- mix form, R = {R}, B = {B}, C = {C}; slots {nnz}, rows {N}; every figure below measured in this run")
    med = report(measure(forms, rounds), nnz, N, R, B, tag, res)
    spread = 0.0
    for kind, form in (("rgcn_mix_fwd", "eval"), ("rgcn_mix_bwd_src", "step"), ("rgcn_mix_bwd_coef", "step"),
                       ("rgcn_comp_reduce", "step")):
        a, a2 = med[f"mix_{form}/{kind}"], med[f"mix_{form}'/{kind}"]
        print(f"A/A of {kind}: {a2 / a:.3f}")
        res[f"{tag}/{kind}_A_over_A"] = round(a2 / a, 3)
        if kind == "rgcn_mix_fwd":
            spread = abs(a2 / a - 1)
    a = med["mix_eval/rgcn_mix_fwd"]
    print(f"rgcn_mix_fwd over spmm_w: {a / med['spmm/spmm_w']:.2f}x  (bytes: "
          f"{byte_model('rgcn_mix_fwd', nnz, N, R, B) / byte_model('spmm_w', nnz, N, R, B):.2f}x)")
    res[f"{tag}/rgcn_mix_fwd_over_spmm_w"] = round(a / med["spmm/spmm_w"], 2)
    if "gat_eval/gat_fwd" in med:
        b = med["gat_eval/gat_fwd"]
        verdict = "met" if a / b <= 1 + spread else "MISSED"
        print(f"rgcn_mix_fwd / gat_fwd: {a / b:.3f}   (expected: at most 1 + the A/A spread = {1 + spread:.3f}: {verdict})")
        res[f"{tag}/rgcn_mix_fwd_over_gat_fwd"] = round(a / b, 3)
        res[f"{tag}/rgcn_mix_fwd_expectation"] = verdict
    else:
        print("gat_fwd: not run (the graph has rows without in-edges)")


def run_select(R, N, graph, et, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, R * C, device=dev) * 0.5
    y0 = torch.randn(N, C, device=dev)
    cot = torch.randn(N, C, device=dev)
    h_g = h.clone().requires_grad_(True)

    def select_eval():
        with torch.no_grad():
            ops.rgcn_aggregate(h, graph, et, R, y0=y0)

    def select_step():
        h_g.grad = None
        ops.rgcn_aggregate(h_g, graph, et, R, y0=y0).backward(cot)

    forms = {"select_eval": select_eval, "select_step": select_step, "select_eval'": select_eval,
             "select_step'": select_step}
    tag = f"R{R}/select"
    print(f"--- select form, R = {R}, C = {C}: h holds N * R * C = {N * R * C * 4 / 1e9:.1f} GB")
    med = report(measure(forms, rounds), nnz, N, R, 0, tag, res)
    for kind, form in (("rgcn_select_fwd", "eval"), ("rgcn_select_bwd", "step")):
        a, a2 = med[f"select_{form}/{kind}"], med[f"select_{form}'/{kind}"]
        print(f"A/A of {kind}: {a2 / a:.3f}")
        res[f"{tag}/{kind}_A_over_A"] = round(a2 / a, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgcn_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f  # once per graph: not part of a step
    has_empty_rows = bool(((graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]) == 0).any().item())
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds, "C": C}
    for R in RELATIONS:
        et = torch.randint(0, R, (E,), generator=torch.Generator().manual_seed(100 + R)).to(dev)
        for B in BASES:
            torch.cuda.empty_cache()
            run_mix(R, B, N, graph, et, has_empty_rows, args.rounds, dev, res)
        torch.cuda.empty_cache()
        need = 3 * N * R * C * 4 + (4 << 30)
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            print(f"--- select form, R = {R}: skipped, {need / 1e9:.1f} GB needed, {free / 1e9:.1f} GB free")
            continue
        run_select(R, N, graph, et, args.rounds, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
