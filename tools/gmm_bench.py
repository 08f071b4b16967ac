#!/usr/bin/env python3
"""GMMConv's aggregation on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) with seeded pseudo-coordinates,
at D = 2 coordinates, M = 64 channels and K in {2, 8} Gaussian kernels, next to its RGCN counterparts at B = K bases (R = 4
relations) in the SAME run: both families gather the same K * M row per slot (forward, edge / coefficient pass) and the same
gout row per slot (source pass); GMM trades the type and weight reads for D floats and K exponentials per slot. The forms
run alternately in one process; every launch is timed with HIP events on its stream (ops.set_event_sink) and the median per
launch kind, after one warm-up call of every form, is reported:
  gmm_fwd, gmm_bwd_src, gmm_bwd_edge (all stages: the table s, g_e, and the two-stage reduction to g_mu / g_sigma);
  rgcn_mix_fwd, rgcn_mix_bwd_src, rgcn_mix_bwd_coef (and rgcn_comp_reduce, its reduction, listed beside it).
Every form runs TWICE per round under two names (A and A'): the ratio of their medians is the tool's A/A spread, which a
gmm / rgcn ratio has to be read against.

Byte model (fp32, E slots, N rows; index traffic included; mu, sigma and comp are cache-resident and not counted):
  gmm_fwd            a K * M row gathered, D coordinates streamed per slot:   E (4 K M + 4 D + 4) + N (8 M + 8)
  gmm_bwd_src        a gout row and D coordinates gathered, col / t2f / w:    E (4 M + 4 D + 12) + N (4 K M + 4)
  gmm_bwd_edge       a K * M row gathered, D coordinates streamed, stores:    E (4 K M + 4 D + 4 + stores) + N (4 M + 4)
                     stores = 12 K + 12 D: the table s written once and read by each of the two second stages with the
                     coordinates, g_e written
  rgcn_mix_fwd       E (4 B M + 12) + N (8 M + 4)
  rgcn_mix_bwd_src   E (4 M + 12) + N (4 B M + 4)
  rgcn_mix_bwd_coef  E (4 B M + 4 B + 8) + N (4 M + 4)
  rgcn_comp_reduce   E (4 B + 4)
Each is reported as ms and as a fraction of 8 TB/s. Expectation: every gmm pass within the byte-model ratio of its rgcn
counterpart, times 1 + the A/A spread. Prints a table, then one JSON line.
Usage: python tools/gmm_bench.py [--rounds R] [--workload L|S]"""
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
M = 64
D = 2
R = 4
KERNELS = [2, 8]
KINDS = ("gmm_", "rgcn_")
PAIRS = (("gmm_fwd", "rgcn_mix_fwd", "eval"), ("gmm_bwd_src", "rgcn_mix_bwd_src", "step"),
         ("gmm_bwd_edge", "rgcn_mix_bwd_coef", "step"))


def byte_model(kind, nnz, N, K):
    return {
        "gmm_fwd": nnz * (4 * K * M + 4 * D + 4) + N * (8 * M + 8),
        "gmm_bwd_src": nnz * (4 * M + 4 * D + 12) + N * (4 * K * M + 4),
        "gmm_bwd_edge": nnz * (4 * K * M + 4 * D + 4 + 12 * K + 12 * D) + N * (4 * M + 4),
        "rgcn_mix_fwd": nnz * (4 * K * M + 12) + N * (8 * M + 4),
        "rgcn_mix_bwd_src": nnz * (4 * M + 12) + N * (4 * K * M + 4),
        "rgcn_mix_bwd_coef": nnz * (4 * K * M + 4 * K + 8) + N * (4 * M + 4),
        "rgcn_comp_reduce": nnz * (4 * K + 4),
    }[kind]


def measure(forms, rounds):
    for fn in forms.values():  # warm-up: code objects, allocator, the typed view, the slot-ordered coordinates
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


def run(K, N, graph, et, e_slot, rounds, dev, res):
    torch.manual_seed(0)
    nnz = graph.fwd.nnz
    h = torch.randn(N, K * M, device=dev) * 0.5
    y0 = torch.randn(N, M, device=dev)
    cot = torch.randn(N, M, device=dev)
    mu = torch.rand(K, D, device=dev)
    sigma = 0.5 + torch.rand(K, D, device=dev)
    comp = torch.randn(R, K, device=dev) * 0.5
    h_g = h.clone().requires_grad_(True)
    e_g = e_slot.clone().requires_grad_(True)
    mu_g, sigma_g, comp_g = (t.clone().requires_grad_(True) for t in (mu, sigma, comp))
    ops.typed_view(graph, et, R)

    def gmm_eval():
        with torch.no_grad():
            ops.gmm_aggregate(h, e_slot, mu, sigma, graph, y0=y0)

    def gmm_step():
        h_g.grad = e_g.grad = mu_g.grad = sigma_g.grad = None
        ops.gmm_aggregate(h_g, e_g, mu_g, sigma_g, graph, y0=y0).backward(cot)

    def rgcn_eval():
        with torch.no_grad():
            ops.rgcn_aggregate(h, graph, et, R, comp=comp, y0=y0)

    def rgcn_step():
        h_g.grad = comp_g.grad = None
        ops.rgcn_aggregate(h_g, graph, et, R, comp=comp_g, y0=y0).backward(cot)

    forms = {"gmm_eval": gmm_eval, "gmm_step": gmm_step, "rgcn_eval": rgcn_eval, "rgcn_step": rgcn_step,
             "gmm_eval'": gmm_eval, "gmm_step'": gmm_step, "rgcn_eval'": rgcn_eval, "rgcn_step'": rgcn_step}
    tag = f"K{K}"
    print(f"--- K = B = {K}, M = {M}, D = {D}, R = {R}; slots {nnz}, rows {N}; every figure below measured in this run")
    times = measure(forms, rounds)
    med = {}
    for key in sorted(times):
        v = times[key]
        med[key] = ms = statistics.median(v)
        nb = byte_model(key.split("/", 1)[1], nnz, N, K)
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:36s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"{tag}/{key}_ms"] = round(ms, 3)
        res[f"{tag}/{key}_frac_8TBs"] = round(frac, 3)
    for gmm, rgcn, form in PAIRS:
        spread = 0.0
        for fam, kind in (("gmm", gmm), ("rgcn", rgcn)):
            a, a2 = med[f"{fam}_{form}/{kind}"], med[f"{fam}_{form}'/{kind}"]
            print(f"A/A of {kind}: {a2 / a:.3f}")
            res[f"{tag}/{kind}_A_over_A"] = round(a2 / a, 3)
            spread = max(spread, abs(a2 / a - 1))
        ratio = med[f"gmm_{form}/{gmm}"] / med[f"rgcn_{form}/{rgcn}"]
        bytes_ratio = byte_model(gmm, nnz, N, K) / byte_model(rgcn, nnz, N, K)
        verdict = "met" if ratio <= bytes_ratio * (1 + spread) else "MISSED"
        print(f"{gmm} / {rgcn}: {ratio:.3f}   (bytes: {bytes_ratio:.3f}; expected: at most the byte ratio times 1 + the "
              f"A/A spread = {bytes_ratio * (1 + spread):.3f}: {verdict})")
        res[f"{tag}/{gmm}_over_{rgcn}"] = round(ratio, 3)
        res[f"{tag}/{gmm}_over_{rgcn}_bytes"] = round(bytes_ratio, 3)
        res[f"{tag}/{gmm}_expectation"] = verdict
    both = med["rgcn_step/rgcn_mix_bwd_coef"] + med["rgcn_step/rgcn_comp_reduce"]
    print(f"gmm_bwd_edge / (rgcn_mix_bwd_coef + rgcn_comp_reduce): {med['gmm_step/gmm_bwd_edge'] / both:.3f}")
    res[f"{tag}/gmm_bwd_edge_over_coef_plus_reduce"] = round(med["gmm_step/gmm_bwd_edge"] / both, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    graph = get_graph(ei.to(dev), N, LOOPS_KEEP)
    graph.bwd, graph.t2f, graph.inv_deg, graph.w_mean_t  # once per graph: not part of a step
    et = torch.randint(0, R, (E,), generator=torch.Generator().manual_seed(100 + R)).to(dev)
    ea = torch.rand(E, D, generator=torch.Generator().manual_seed(200)).to(dev)
    e_slot = ops.edge_rows_to_slots(ea, graph)
    res = {"workload": args.workload, "N": N, "slots": graph.fwd.nnz, "rounds": args.rounds, "M": M, "D": D, "R": R}
    for K in KERNELS:
        torch.cuda.empty_cache()
        run(K, N, graph, et, e_slot, args.rounds, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
