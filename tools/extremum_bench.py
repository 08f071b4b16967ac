#!/usr/bin/env python3
"""max aggregation on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M), timed with HIP events: 3 warm-ups,
the median of --runs (>= 10) single launches, everything in ONE process on the same graph, at d = 64 and d = 128:
  1. the forward (rgbx_spmm_csr_extremum_f32) with arg (training) and without it (inference);
  2. the backward over the transposed CSR (rgbx_extremum_bwd_f32);
  3. the yardsticks of the same run: the mean gather (rgbx_spmm_csr_f32 with the row scale 1/deg) and the transposed mean
     gather (the same kernel over the transposed CSR with one weight per slot) — the forward and backward of aggr='mean'.
Algorithmic bytes (every array once, gathered rows once per slot):
  gather          E' (4 d + 4) + N 4 d + 4 (N + 1)          (+ 4 N for the row scale, + 4 E' for per-slot weights)
  forward + arg   the gather + 4 N d
  backward        E' (8 d + 8) + N 4 d + 4 (N + 1): a gout row AND an arg row per transposed slot, col and t2f per slot —
                  about twice the transposed gather.
Prints a table, then one JSON line. Usage: python tools/extremum_bench.py [--workload L|S] [--runs R] [--out FILE]"""
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


def median_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 10:
        ap.error("--runs must be at least 10")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    g = get_graph(ei.to(dev), N, LOOPS_KEEP)
    g.bwd, g.t2f, g.inv_deg, g.w_mean_t  # the sort, the slot map and the mean's weights: once per graph, not timed
    nnz = g.fwd.nnz
    lines, res = [], {"workload": args.workload, "N": N, "E": E, "nnz": nnz, "runs": args.runs}
    for d in (64, 128):
        x, gout = torch.randn(N, d, device=dev), torch.randn(N, d, device=dev)
        out = torch.empty(N, d, device=dev)
        gather = nnz * (4 * d + 4) + N * 4 * d + 4 * (N + 1)
        nbytes = {"mean_fwd": gather + 4 * N, "mean_bwd": gather + 4 * nnz, "max_fwd": gather, "max_fwd_arg": gather + 4 * N * d,
                  "max_bwd": nnz * (8 * d + 8) + N * 4 * d + 4 * (N + 1)}
        _, arg = ops.spmm_extremum_raw(g.fwd, x, "max", True)
        t = {"mean_fwd": median_ms(lambda: ops.spmm_raw(g.fwd, None, g.inv_deg, x, out=out), args.runs),
             "mean_bwd": median_ms(lambda: ops.spmm_raw(g.bwd, g.w_mean_t, None, gout, out=out), args.runs),
             "max_fwd": median_ms(lambda: ops.spmm_extremum_raw(g.fwd, x, "max", False), args.runs),
             "max_fwd_arg": median_ms(lambda: ops.spmm_extremum_raw(g.fwd, x, "max", True), args.runs),
             "max_bwd": median_ms(lambda: ops.extremum_bwd_raw(g, gout, arg), args.runs)}
        for k, ms in t.items():
            res[f"{k}_d{d}_ms"], res[f"{k}_d{d}_bytes"] = ms, nbytes[k]
            lines.append(f"d = {d:3d}   {k:12s} {ms:8.3f} ms   {nbytes[k] / 1e9:6.2f} GB algorithmic, "
                         f"{nbytes[k] / (ms * 1e-3) / 1e12:5.2f} TB/s ({100 * nbytes[k] / (ms * 1e-3) / PEAK:4.1f} % of 8 TB/s)")
        ratios = {"max_fwd / mean_fwd": ("max_fwd", "mean_fwd"), "max_fwd_arg / mean_fwd": ("max_fwd_arg", "mean_fwd"),
                  "max_bwd / mean_bwd": ("max_bwd", "mean_bwd")}
        for label, (a, b) in ratios.items():
            res[f"{a}_over_{b}_d{d}"] = t[a] / t[b]
            lines.append(f"d = {d:3d}   {label:24s} time x{t[a] / t[b]:5.2f}   bytes x{nbytes[a] / nbytes[b]:5.2f}")
        del x, gout, out, arg
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
