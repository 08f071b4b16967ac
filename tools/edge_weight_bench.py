#!/usr/bin/env python3
"""Edge weights on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M), timed with HIP events: 3 warm-ups,
the median of --runs (>= 10) single launches, everything in ONE process on the same graph:
  1. the weighted preparation (loop weights, slot weights of both CSRs, weighted degree, w and w_t) against the
     unweighted one (deg^-1/2 from the row counts, w and w_t); the CSR build is shared and not timed;
  2. the edge-dot kernel (rgbx_edge_dot_f32) at d = 128 and d = 64 against the row gather (rgbx_spmm_csr_f32) at the same
     width: both move the same neighbour rows, so the SpMM time is the yardstick;
  3. the backward of the normalisation (rgbx_gcn_norm_bwd_f32).
Algorithmic bytes of the edge dot: E' (4 d + 8) + N 4 d + 4 (N + 1). Prints a table, then one JSON line.
Usage: python tools/edge_weight_bench.py [--workload L|S] [--runs R] [--out FILE]"""
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
from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, WeightedGraph, get_graph

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
    ei = ei.to(dev)
    ew = (torch.rand(E, device=dev) * 3.75 + 0.25)
    base = get_graph(ei, N, LOOPS_ADD_REMAINING)
    base.bwd, base.t2f  # the sort and the slot map: shared by both preparations, once per graph
    nnz = base.fwd.nnz
    lines, res = [], {"workload": args.workload, "N": N, "E": E, "nnz": nnz, "runs": args.runs}

    def prep_unweighted():
        base._dis = base._w = base._w_t = None
        return base.w, base.w_t

    def prep_weighted():
        g = WeightedGraph(base, ew)  # includes the finiteness check (one pass over ew and a host read)
        return g.w, g.w_t

    t_u, t_w = median_ms(prep_unweighted, args.runs), median_ms(prep_weighted, args.runs)
    res["prep_unweighted_ms"], res["prep_weighted_ms"], res["prep_ratio"] = t_u, t_w, t_w / t_u
    lines.append(f"preparation (dis, w, w_t)   unweighted {t_u:8.3f} ms   weighted {t_w:8.3f} ms   ratio {t_w / t_u:5.2f}")

    wg = WeightedGraph(base, ew)
    wg.w, wg.w_t
    for d in (128, 64):
        a, b = torch.randn(N, d, device=dev), torch.randn(N, d, device=dev)
        out = torch.empty(N, d, device=dev)
        t_s = median_ms(lambda: ops.spmm_raw(wg.fwd, wg.w, None, b, out=out), args.runs)
        t_d = median_ms(lambda: ops.edge_dot_raw(wg.fwd, a, b), args.runs)
        nbytes = nnz * (4 * d + 8) + N * 4 * d + 4 * (N + 1)
        res[f"spmm_d{d}_ms"], res[f"edge_dot_d{d}_ms"], res[f"edge_dot_d{d}_ratio"] = t_s, t_d, t_d / t_s
        res[f"edge_dot_d{d}_bytes"], res[f"edge_dot_d{d}_frac_peak"] = nbytes, nbytes / (t_d * 1e-3) / PEAK
        lines.append(f"d = {d:3d}   spmm {t_s:8.3f} ms   edge dot {t_d:8.3f} ms   ratio {t_d / t_s:5.2f}   "
                     f"{nbytes / 1e9:6.2f} GB algorithmic, {nbytes / (t_d * 1e-3) / 1e12:5.2f} TB/s "
                     f"({100 * nbytes / (t_d * 1e-3) / PEAK:4.1f} % of 8 TB/s)")
        del a, b, out
    gs = torch.randn(nnz, device=dev)
    t_b = median_ms(lambda: ops.gcn_norm_bwd(wg, gs), args.runs)
    res["gcn_norm_bwd_ms"] = t_b
    lines.append(f"gcn_norm backward           {t_b:8.3f} ms")
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
