#!/usr/bin/env python3
"""The softmax aggregation's kernels (GENConv / DeeperGCN) on workload L's synthetic graph (bench.synth: |V| = 2 M,
|E| = 60 M) at C = 64 and C = 128, next to three yardsticks in the SAME run: propagate_max's forward (the same one-row
gather per slot, a per-channel maximum, no expf), ResGatedGraphConv's forward at the same C (twice the gather, one expf
and one division per element) and the plain weighted SpMM at width C. The forms run alternately in one process; every
launch is timed with HIP events on its stream (ops.set_event_sink) and the median per launch kind is reported:
  softmax_aggr_fwd      inference form (no lse) and training form (lse written),
  softmax_aggr_bwd      without g_t (t takes no gradient) and with it (records + reduction, inside the one label),
  max_fwd, resgated_fwd, spmm_weighted.
The two yardsticks that a ratio is read against run TWICE per round under two names (A and A'): the ratio of their
medians is the A/A spread. t is one value per channel, drawn from [0.5, 2]. All forms take the edges as given (E slots).

Byte model (fp32, E slots, N rows; index traffic included; t and the g_t records are C floats per workgroup: left out):
  softmax_aggr_fwd  inference  a message row per slot:              E (4 C + 4) + N (4 C + 4)       (out written)
  softmax_aggr_fwd  training   the same, and lse:                   E (4 C + 4) + N (8 C + 4)
  softmax_aggr_bwd             gout, out and lse rows per slot:     E (12 C + 4) + N (8 C + 4)      (m read, g_m written)
  max_fwd (inference)          a row per slot:                      E (4 C + 4) + N (4 C + 4)
  resgated_fwd                 a q row and a v row per slot:        E (8 C + 4) + N (8 C + 4)
  spmm_weighted                a row and a weight per slot:         E (4 C + 8) + N (4 C + 4)
Each is reported as ms and as a fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/softmax_aggr_bench.py [--rounds R] [--workload L|S]"""
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


def byte_model(key, nnz, N, C):
    return {
        "softmax_eval/softmax_aggr_fwd": nnz * (4 * C + 4) + N * (4 * C + 4),
        "softmax_step/softmax_aggr_fwd": nnz * (4 * C + 4) + N * (8 * C + 4),
        "softmax_step/softmax_aggr_bwd": nnz * (12 * C + 4) + N * (8 * C + 4),
        "softmax_step_t/softmax_aggr_fwd": nnz * (4 * C + 4) + N * (8 * C + 4),
        "softmax_step_t/softmax_aggr_bwd": nnz * (12 * C + 4) + N * (8 * C + 4),
        "max/max_fwd": nnz * (4 * C + 4) + N * (4 * C + 4),
        "resgated/resgated_fwd": nnz * (8 * C + 4) + N * (8 * C + 4),
        "spmm/spmm_weighted": nnz * (4 * C + 8) + N * (4 * C + 4),
    }[key.replace("'", "")]


def run_width(C, N, graph, rounds, dev, res):
    torch.manual_seed(0)
    h = torch.randn(N, 3 * C, device=dev) * 0.5
    m = torch.relu(torch.randn(N, C, device=dev)) + 1e-7          # what GENConv hands over
    t = torch.rand(C, device=dev) * 1.5 + 0.5
    cot = torch.randn(N, C, device=dev)
    out = torch.empty(N, C, device=dev)
    m_g = m.clone().requires_grad_(True)
    t_g = t.clone().requires_grad_(True)

    def sm_eval():
        with torch.no_grad():
            ops.softmax_aggregate(m, t, graph)

    def sm_step():
        m_g.grad = None
        ops.softmax_aggregate(m_g, t, graph).backward(cot)

    def sm_step_t():
        m_g.grad = t_g.grad = None
        ops.softmax_aggregate(m_g, t_g, graph).backward(cot)

    def mx():
        ops.spmm_extremum_raw(graph.fwd, m, "max", False)

    def rg():
        with torch.no_grad():
            ops.resgated_aggregate(h[:, :C], h[:, C:2 * C], h[:, 2 * C:], graph)

    forms = {"softmax_eval": sm_eval, "softmax_step": sm_step, "softmax_step_t": sm_step_t, "max": mx, "max'": mx,
             "resgated": rg, "resgated'": rg,
             "spmm": lambda: ops.spmm_raw(graph.fwd, graph.w, None, m, out=out, kind="spmm_weighted")}
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
                if str(kind).startswith(("softmax_aggr_", "max_fwd", "resgated_", "spmm_weighted")):
                    times.setdefault(f"{form}/{kind}", []).append(s.elapsed_time(e))
    nnz = graph.fwd.nnz
    print(f"--- C = {C}; slots {nnz}, rows {N}")
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        nb = byte_model(key, nnz, N, C)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:38s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"C{C}/{key}_ms"] = round(ms, 3)
        res[f"C{C}/{key}_frac_8TBs"] = round(frac, 3)
    fwd, fwd_t = med["softmax_eval/softmax_aggr_fwd"], med["softmax_step/softmax_aggr_fwd"]
    bwd, bwd_t = med["softmax_step/softmax_aggr_bwd"], med["softmax_step_t/softmax_aggr_bwd"]
    a_max, a_rg = med["max'/max_fwd"] / med["max/max_fwd"], med["resgated'/resgated_fwd"] / med["resgated/resgated_fwd"]
    spmm = med["spmm/spmm_weighted"]
    print(f"forward (inference) / max_fwd: {fwd / med['max/max_fwd']:.3f}   (A/A of max_fwd: {a_max:.3f})")
    print(f"forward (inference) / resgated_fwd: {fwd / med['resgated/resgated_fwd']:.3f}   (A/A of resgated_fwd: {a_rg:.3f})")
    print(f"forward training / inference: {fwd_t / fwd:.3f};  backward with g_t / without: {bwd_t / bwd:.3f}")
    print(f"over spmm_weighted: forward {fwd / spmm:.2f}x, backward {bwd / spmm:.2f}x")
    res[f"C{C}/fwd_over_max_fwd"] = round(fwd / med["max/max_fwd"], 3)
    res[f"C{C}/max_fwd_A_over_A"] = round(a_max, 3)
    res[f"C{C}/fwd_over_resgated_fwd"] = round(fwd / med["resgated/resgated_fwd"], 3)
    res[f"C{C}/resgated_fwd_A_over_A"] = round(a_rg, 3)
    res[f"C{C}/fwd_training_over_inference"] = round(fwd_t / fwd, 3)
    res[f"C{C}/bwd_g_t_over_plain"] = round(bwd_t / bwd, 3)
    res[f"C{C}/fwd_over_spmm_weighted"] = round(fwd / spmm, 2)
    res[f"C{C}/bwd_over_spmm_weighted"] = round(bwd / spmm, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_aggr_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
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
