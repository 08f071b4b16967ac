#!/usr/bin/env python3
"""PNAConv's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at d = 16, 32, 64 with the
default four aggregators (mean, max, min, std) and three scalers (identity, amplification, attenuation), next to their
multi-aggregation counterparts in the SAME run: rgbx_spmm_csr_multi_f32 with the same four statistics of the bare source
rows (the forward's counterpart) and rgbx_multi_bwd_f32 with all its terms (the counterpart of both backward passes).
The forms run alternately in one process; every launch is timed with HIP events on its stream (ops.set_event_sink) and
the median per launch kind, after one warm-up call of every form, is reported:
  pna_fwd (inference form, with and without c), pna_fwd+kept (the training form: raw mean, std, argmax, argmin stored),
  pna_bwd_src (with and without c), pna_bwd_edge (with c), multi_fwd, multi_bwd.

Byte model (fp32, nnz slots, N rows, S * A = 12 blocks; index traffic included):
  pna_fwd        nnz (4 + 4 d [+ 4 d with c]) + N 4 d (S A + kept)          kept = 4 in the training form, 0 otherwise
  multi_fwd      nnz (4 + 4 d) + N 4 d A
  pna_bwd_src    nnz (8 + 4 d (6 [+ 1 with c])) + N 4 d 2                   A, B, gmax, argmax, gmin, argmin rows per slot;
                                                                            col + t2f; b read, g_b written
  pna_bwd_edge   nnz (4 + 4 d 3) + N 4 d 6                                  b gathered, c streamed, g_c stored; six term rows
  multi_bwd      nnz (8 + 4 d 6) + N 4 d 2
Expectation: time(pna pass) / time(counterpart) <= bytes(pna pass) / bytes(counterpart), with the spread of the
counterpart's own repeats in this run, (max - min) / median, as the margin. A missed expectation is reported, not tuned.
Prints a table, then one JSON line.
Usage: python tools/pna_bench.py [--rounds R] [--workload L|S]"""
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
WIDTHS = [16, 32, 64]
AGGR = ("mean", "max", "min", "std")
SCALERS = ("identity", "amplification", "attenuation")
S, A = len(SCALERS), len(AGGR)


def byte_model(key, nnz, N, d):
    return {
        "pna_fwd": nnz * (4 + 4 * d) + N * 4 * d * S * A,
        "pna_fwd+c": nnz * (4 + 8 * d) + N * 4 * d * S * A,
        "pna_fwd+kept": nnz * (4 + 4 * d) + N * 4 * d * (S * A + 4),
        "pna_fwd+c+kept": nnz * (4 + 8 * d) + N * 4 * d * (S * A + 4),
        "pna_bwd_src": nnz * (8 + 4 * d * 6) + N * 4 * d * 2,
        "pna_bwd_src+c": nnz * (8 + 4 * d * 7) + N * 4 * d * 2,
        "pna_bwd_edge+c": nnz * (4 + 4 * d * 3) + N * 4 * d * 6,
        "multi_fwd": nnz * (4 + 4 * d) + N * 4 * d * A,
        "multi_bwd": nnz * (8 + 4 * d * 6) + N * 4 * d * 2,
    }[key]


COUNTERPART = {"pna_fwd": "multi_fwd", "pna_fwd+c": "multi_fwd", "pna_bwd_src": "multi_bwd", "pna_bwd_src+c": "multi_bwd",
               "pna_bwd_edge+c": "multi_bwd"}


def run_width(d, N, graph, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    avg = ops.degree_averages(graph)
    a = torch.randn(N, d, device=dev) * 0.5
    b = torch.randn(N, d, device=dev) * 0.5
    c = torch.randn(nnz, d, device=dev) * 0.5
    cot = torch.randn(N, S * A * d, device=dev)
    cot_m = torch.randn(N, A * d, device=dev)
    b_g, c_g, x_g = b.clone().requires_grad_(True), c.requires_grad_(True), b.clone().requires_grad_(True)

    def pna_eval(with_c):
        def fn():
            with torch.no_grad():
                ops.pna_aggregate(a, b, c if with_c else None, graph, AGGR, SCALERS, avg, d)
        return fn

    def pna_step(with_c):
        def fn():
            b_g.grad = c_g.grad = None
            ops.pna_aggregate(a, b_g, c_g if with_c else None, graph, AGGR, SCALERS, avg, d).backward(cot)
        return fn

    def multi_eval():
        with torch.no_grad():
            ops.propagate_multi(b, graph, AGGR)

    def multi_step():
        x_g.grad = None
        ops.propagate_multi(x_g, graph, AGGR).backward(cot_m)

    forms = {"eval": pna_eval(False), "eval+c": pna_eval(True), "step": pna_step(False), "step+c": pna_step(True),
             "multi_eval": multi_eval, "multi_step": multi_step}
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
                kind = str(kind)
                if not kind.startswith(("pna_", "multi_")):
                    continue
                if form.startswith("multi"):
                    if form == "multi_step" and kind == "multi_fwd":
                        continue  # the training forward keeps args: only the inference form is the counterpart
                    key = kind
                else:
                    key = kind + ("+c" if form.endswith("+c") else "") + ("+kept" if kind == "pna_fwd" and "step" in form else "")
                times.setdefault(key, []).append(s.elapsed_time(t))
    print(f"--- d = {d}; slots {nnz}, rows {N}; {A} aggregators x {S} scalers; every figure below measured in this run")
    med, spread = {}, {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        spread[key] = (max(v) - min(v)) / ms
        nb = byte_model(key, nnz, N, d)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:18s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"d{d}/{key}_ms"] = round(ms, 3)
        res[f"d{d}/{key}_frac_8TBs"] = round(frac, 3)
    for mine, theirs in COUNTERPART.items():
        t_ratio = med[mine] / med[theirs]
        b_ratio = byte_model(mine, nnz, N, d) / byte_model(theirs, nnz, N, d)
        bound = b_ratio * (1 + spread[theirs])
        verdict = "met" if t_ratio <= bound else "MISSED"
        print(f"{mine} / {theirs}: time ratio {t_ratio:.3f}, byte-model ratio {b_ratio:.3f}, margin (spread of {theirs}) "
              f"{spread[theirs]:.3f}: {verdict}")
        res[f"d{d}/{mine}_over_{theirs}"] = round(t_ratio, 3)
        res[f"d{d}/{mine}_byte_ratio"] = round(b_ratio, 3)
        res[f"d{d}/{mine}_expectation"] = verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pna_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f, graph.inv_deg  # once per graph: not part of a step
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds, "widths": WIDTHS}
    for d in WIDTHS:
        torch.cuda.empty_cache()
        run_width(d, N, graph, args.rounds, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
