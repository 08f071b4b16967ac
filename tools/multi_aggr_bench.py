#!/usr/bin/env python3
"""Four aggregates ['mean', 'max', 'min', 'std'] from ONE gather pass against the four composed gathers, on workload L's
synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at d = 64 and d = 128. Everything runs in ONE process on the same
graph; the forms ALTERNATE (one launch of each per round, 3 warm-up rounds, then --runs rounds), every launch is timed with
HIP events, and the median over the rounds is reported:
  multi_fwd / multi_fwd_arg   rgbx_spmm_csr_multi_f32 into the four column blocks of one [N, 4 d] tensor, without / with arg
  multi_bwd                   rgbx_multi_bwd_f32 with all four terms (a, b, gmax + argmax, gmin + argmin)
  composed forward            the mean gather on x and on x^2 (rgbx_spmm_csr_f32), max and min with arg
                              (rgbx_spmm_csr_extremum_f32): four gathers, four [N, d] outputs (the concatenation and the
                              elementwise x^2 / sqrt are NOT counted)
  composed backward           the transposed mean gather twice (rgbx_spmm_csr_f32 with one weight per slot) and
                              rgbx_extremum_bwd_f32 twice
Algorithmic bytes (every array once, gathered rows once per slot; E' slots, N rows):
  gather             E' (4 d + 4) + 4 N d + 4 (N + 1)        (+ 4 N row scale / + 4 E' per-slot weights; + 4 N d per arg)
  multi_fwd          E' (4 d + 4) + 4 * 4 N d + 4 (N + 1)    (+ 2 * 4 N d with both arg)
  extremum backward  E' (8 d + 8) + 4 N d + 4 (N + 1)
  multi_bwd          E' (6 * 4 d + 8) + 2 * 4 N d + 4 (N + 1): six rows per transposed slot, x[j] and gx[j] once per row
Prints a table, then one JSON line. Usage: python tools/multi_aggr_bench.py [--workload L|S] [--runs R] [--out FILE]"""
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
FOUR = ("mean", "max", "min", "std")


def alternate_ms(forms, runs, warmup=3):
    """{name: median ms}: one launch of every form per round, in turn, each between its own pair of HIP events."""
    times = {k: [] for k in forms}
    for r in range(warmup + runs):
        for k, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[k].append(s.elapsed_time(e))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 7:
        ap.error("--runs must be at least 7")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    g = get_graph(ei.to(dev), N, LOOPS_KEEP)
    g.bwd, g.t2f, g.inv_deg, g.w_mean_t  # the sort, the slot map and the mean's weights: once per graph, not timed
    nnz = g.fwd.nnz
    lines, res = [], {"workload": args.workload, "N": N, "E": E, "nnz": nnz, "runs": args.runs}
    for d in (64, 128):
        x, gy = torch.randn(N, d, device=dev), torch.randn(N, 4 * d, device=dev)
        x2, out = x * x, torch.empty(N, d, device=dev)
        blk = lambda s: gy[:, s * d:(s + 1) * d]
        _, amax, amin, _ = ops.spmm_multi_raw(g.fwd, x, FOUR, True)
        a, b = torch.randn(N, d, device=dev), torch.randn(N, d, device=dev)
        gather = nnz * (4 * d + 4) + 4 * N * d + 4 * (N + 1)
        ext_bwd = nnz * (8 * d + 8) + 4 * N * d + 4 * (N + 1)
        nbytes = {"multi_fwd": nnz * (4 * d + 4) + 16 * N * d + 4 * (N + 1),
                  "multi_fwd_arg": nnz * (4 * d + 4) + 24 * N * d + 4 * (N + 1),
                  "multi_bwd": nnz * (24 * d + 8) + 8 * N * d + 4 * (N + 1),
                  "mean_fwd_x": gather + 4 * N, "mean_fwd_x2": gather + 4 * N,
                  "max_fwd_arg": gather + 4 * N * d, "min_fwd_arg": gather + 4 * N * d,
                  "mean_bwd_1": gather + 4 * nnz, "mean_bwd_2": gather + 4 * nnz, "max_bwd": ext_bwd, "min_bwd": ext_bwd}
        forms = {"multi_fwd": lambda: ops.spmm_multi_raw(g.fwd, x, FOUR, False),
                 "mean_fwd_x": lambda: ops.spmm_raw(g.fwd, None, g.inv_deg, x, out=out),
                 "mean_fwd_x2": lambda: ops.spmm_raw(g.fwd, None, g.inv_deg, x2, out=out),
                 "max_fwd_arg": lambda: ops.spmm_extremum_raw(g.fwd, x, "max", True),
                 "min_fwd_arg": lambda: ops.spmm_extremum_raw(g.fwd, x, "min", True),
                 "multi_fwd_arg": lambda: ops.spmm_multi_raw(g.fwd, x, FOUR, True),
                 "multi_bwd": lambda: ops.multi_bwd_raw(g, a=a, b=b, x=x, gmax=blk(1), argmax=amax, gmin=blk(2), argmin=amin),
                 "mean_bwd_1": lambda: ops.spmm_raw(g.bwd, g.w_mean_t, None, blk(0), out=out),
                 "mean_bwd_2": lambda: ops.spmm_raw(g.bwd, g.w_mean_t, None, blk(3), out=out),
                 "max_bwd": lambda: ops.extremum_bwd_raw(g, blk(1), amax),
                 "min_bwd": lambda: ops.extremum_bwd_raw(g, blk(2), amin)}
        t = alternate_ms(forms, args.runs)
        for k, ms in t.items():
            res[f"{k}_d{d}_ms"], res[f"{k}_d{d}_bytes"] = ms, nbytes[k]
            lines.append(f"d = {d:3d}   {k:14s} {ms:8.3f} ms   {nbytes[k] / 1e9:6.2f} GB algorithmic, "
                         f"{nbytes[k] / (ms * 1e-3) / 1e12:5.2f} TB/s ({100 * nbytes[k] / (ms * 1e-3) / PEAK:4.1f} % of 8 TB/s)")
        sums = {"composed_fwd": ("mean_fwd_x", "mean_fwd_x2", "max_fwd_arg", "min_fwd_arg"),
                "composed_bwd": ("mean_bwd_1", "mean_bwd_2", "max_bwd", "min_bwd")}
        for k, parts in sums.items():
            t[k], nbytes[k] = sum(t[p] for p in parts), sum(nbytes[p] for p in parts)
            res[f"{k}_d{d}_ms"], res[f"{k}_d{d}_bytes"] = t[k], nbytes[k]
            lines.append(f"d = {d:3d}   {k:14s} {t[k]:8.3f} ms   {nbytes[k] / 1e9:6.2f} GB algorithmic (the sum of its four launches)")
        for label, (p, q) in {"multi_fwd_arg / composed_fwd": ("multi_fwd_arg", "composed_fwd"),
                              "multi_fwd / composed_fwd": ("multi_fwd", "composed_fwd"),
                              "multi_bwd / composed_bwd": ("multi_bwd", "composed_bwd")}.items():
            res[f"{p}_over_{q}_d{d}"] = t[p] / t[q]
            lines.append(f"d = {d:3d}   {label:30s} time x{t[p] / t[q]:5.2f}   bytes x{nbytes[p] / nbytes[q]:5.2f}")
        del x, x2, gy, out, amax, amin, a, b
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
