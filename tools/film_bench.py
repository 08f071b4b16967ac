#!/usr/bin/env python3
"""FiLMConv's aggregation on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) with seeded edge types, at
C = 64 channels and R in {1, 4} relations (R = 1: the call without edge types), next to three yardsticks in the SAME run
and process: the RGCN select-form forward (ops.rgcn_aggregate without comp: the same gather out of N * R rows, no film
rows), the plain weighted SpMM at width C, and the ResGatedGraphConv forward (a per-channel gate from two gathered rows).
The forms run alternately; every launch is timed with HIP events on its stream (ops.set_event_sink) and the median per
launch kind, after one warm-up call of every form, is reported:
  film_fwd (no_grad form and the grad-recording one: the same kernel), film_bwd_src, film_bwd_film,
  rgcn_select_fwd, spmm_w, resgated_fwd.
Every FiLM form runs TWICE per round under two names (A and A'): the ratio of their medians is the tool's A/A spread,
which a film / select ratio has to be read against.

Byte model (fp32, E slots, N rows; index traffic included; a target's film rows counted once):
  film_fwd        a C row gathered per slot, col / type / weight; per target R film rows, y0, out, rowptr:
                                                                     E (4 C + 12) + N (8 R C + 8 C + 4)
                  (without edge types no type and no weight is read: E (4 C + 4) + N (16 C + 4))
  film_bwd_src    gout and a film row gathered per slot, col / weight; per row h read, g_h written, rowptr:
                                                                     E (12 C + 8) + N R (8 C + 4)
  film_bwd_film   a C row gathered per slot, col; per row the film row read, (g_beta | g_gamma) written, rowptr;
                  gout read once per target:                         E (4 C + 4) + N R (16 C + 4) + N 4 C
  rgcn_select_fwd a C row gathered per slot out of N * R rows:       E (4 C + 8) + N (8 C + 4)
  spmm_w          a C row per slot, col / weight:                    E (4 C + 8) + N (4 C + 4)
  resgated_fwd    two C rows per slot, col; k read, out written:     E (8 C + 4) + N (8 C + 4)
Each is reported as ms and as a fraction of 8 TB/s. The one expectation: film_fwd takes no more than the select-form
forward of the same run times the ratio of their byte models, beyond the A/A spread; it is printed as met or MISSED.
Prints a table, then one JSON line; --out writes the same text to a file (profiles/film_bench_L.txt is such a run).
Usage: python tools/film_bench.py [--rounds R] [--workload L|S] [--out FILE]"""
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
RELATIONS = [1, 4]
KINDS = ("film_", "rgcn_select_fwd", "spmm_w", "resgated_fwd")


def byte_model(kind, nnz, N, R):
    return {
        "film_fwd": nnz * (4 * C + (12 if R > 1 else 4)) + N * (8 * R * C + 8 * C + 4),
        "film_bwd_src": nnz * (12 * C + 8) + N * R * (8 * C + 4),
        "film_bwd_film": nnz * (4 * C + 4) + N * R * (16 * C + 4) + N * 4 * C,
        "rgcn_select_fwd": nnz * (4 * C + 8) + N * (8 * C + 4),
        "spmm_w": nnz * (4 * C + 8) + N * (4 * C + 4),
        "resgated_fwd": nnz * (8 * C + 4) + N * (8 * C + 4),
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


def run(R, N, graph, et, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, R * C, device=dev) * 0.5
    fb = torch.randn(N, R * 2 * C, device=dev) * 0.5
    y0 = torch.randn(N, C, device=dev)
    cot = torch.randn(N, C, device=dev)
    k, q, v = (torch.randn(N, C, device=dev) * 0.5 for _ in range(3))
    h_g, fb_g = h.clone().requires_grad_(True), fb.clone().requires_grad_(True)
    view = ops.typed_view(graph, et, R)  # the select form's, and with R > 1 FiLM's
    film_et = et if R > 1 else None      # one relation: the call without edge types

    def film_eval():
        with torch.no_grad():
            ops.film_aggregate(h, fb, graph, film_et, R, y0=y0)

    def film_step():
        h_g.grad = fb_g.grad = None
        ops.film_aggregate(h_g, fb_g, graph, film_et, R, y0=y0).backward(cot)

    def select_eval():
        with torch.no_grad():
            ops.rgcn_aggregate(h, graph, et, R, y0=y0)

    def spmm_w():
        ops.spmm_raw(graph.fwd, view.w_f, None, k, kind="spmm_w")

    def resgated_eval():
        with torch.no_grad():
            ops.resgated_aggregate(k, q, v, graph)

    forms = {"film_eval": film_eval, "film_step": film_step, "select": select_eval, "spmm": spmm_w,
             "resgated": resgated_eval, "film_eval'": film_eval, "film_step'": film_step}
    tag = f"R{R}"
    print(f"--- R = {R}{' (no edge types)' if R == 1 else ''}, C = {C}; slots {nnz}, rows {N}; h and fb hold "
          f"N * R * 3 C = {N * R * 3 * C * 4 / 1e9:.1f} GB; every figure below measured in this run")
    times = measure(forms, rounds)
    med = {}
    for key in sorted(times):
        vals = times[key]
        med[key] = ms = statistics.median(vals)
        nb = byte_model(key.split("/", 1)[1], nnz, N, R)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:36s} {ms:9.3f} ms  (min {min(vals):.3f}, max {max(vals):.3f}, n {len(vals)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"{tag}/{key}_ms"] = round(ms, 3)
        res[f"{tag}/{key}_frac_8TBs"] = round(frac, 3)
    spread = 0.0
    for kind, form in (("film_fwd", "eval"), ("film_fwd", "step"), ("film_bwd_src", "step"), ("film_bwd_film", "step")):
        a, a2 = med[f"film_{form}/{kind}"], med[f"film_{form}'/{kind}"]
        print(f"A/A of {kind} ({form}): {a2 / a:.3f}")
        res[f"{tag}/{kind}_{form}_A_over_A"] = round(a2 / a, 3)
        if (kind, form) == ("film_fwd", "eval"):
            spread = abs(a2 / a - 1)
    a, b = med["film_eval/film_fwd"], med["select/rgcn_select_fwd"]
    ratio = byte_model("film_fwd", nnz, N, R) / byte_model("rgcn_select_fwd", nnz, N, R)
    bound = ratio * (1 + spread)
    verdict = "met" if a / b <= bound else "MISSED"
    print(f"film_fwd / rgcn_select_fwd: {a / b:.3f}   (bytes: {ratio:.3f}; expected: at most the byte ratio times 1 + the "
          f"A/A spread = {bound:.3f}: {verdict})")
    res[f"{tag}/film_fwd_over_select_fwd"] = round(a / b, 3)
    res[f"{tag}/film_fwd_byte_ratio"] = round(ratio, 3)
    res[f"{tag}/film_fwd_expectation"] = verdict
    for other, key in (("spmm_w", "spmm/spmm_w"), ("resgated_fwd", "resgated/resgated_fwd")):
        print(f"film_fwd over {other}: {a / med[key]:.2f}x  (bytes: "
              f"{byte_model('film_fwd', nnz, N, R) / byte_model(other, nnz, N, R):.2f}x)")
        res[f"{tag}/film_fwd_over_{other}"] = round(a / med[key], 2)


class _Tee:
    def __init__(self, *streams):
        self.streams = streams

    def write(self, text):
        for stream in self.streams:
            stream.write(text)

    def flush(self):
        for stream in self.streams:
            stream.flush()


def bench(args):
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f  # once per graph: not part of a step
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds, "C": C}
    for R in RELATIONS:
        et = torch.randint(0, R, (E,), generator=torch.Generator().manual_seed(100 + R)).to(dev)
        torch.cuda.empty_cache()
        run(R, N, graph, et, args.rounds, dev, res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("film_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    if args.out is None:
        return bench(args)
    with open(args.out, "w") as report:
        sys.stdout = _Tee(sys.__stdout__, report)
        try:
            bench(args)
        finally:
            sys.stdout = sys.__stdout__


if __name__ == "__main__":
    main()
