#!/usr/bin/env python3
"""TransformerConv's kernels on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at (8 heads x 16) and
(1 x 128), next to GATv2's kernels at the same H, C in the SAME run as the yardstick. The forms run alternately in one
process; every launch is timed with HIP events on its stream (ops.set_event_sink) and the median per launch kind is
reported:
  transformer_fwd (eval form, and the training form with attention dropout p = 0.5), transformer_bwd_dst,
  transformer_bwd_src, and gatv2_fwd / gatv2_bwd_dst / gatv2_bwd_src.
q, k and v are the column blocks of one [N, 3 F] matrix, as TransformerConv hands them over (k and v of a source side by
side). TransformerConv takes the edges as given (E slots), GATv2 rewrites the self-loops (E' slots): each model uses its
own count.

Byte model (fp32, F = H C, E slots, N rows; index and per-(row, head) scalar traffic included):
  forward       a k row and a v row per slot:  E (8 F + 4) + N (2 * 4 F + 8 H + 4)      -- twice GATv2's gather
  target pass   a k row and a v row per slot:  E (8 F + 4) + N (4 * 4 F + 16 H + 4)     (q, gout, out read, g_q written)
  source pass   q_i, gout_i and the (shift, D) record per slot:
                                               E (8 F + 8 H + 4 [+ 4 with dropout]) + N (4 * 4 F + 4)   (k, v read, g_k, g_v written)
Each is reported as ms and as a fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/transformer_bench.py [--rounds R] [--workload L|S]"""
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
from rgb_experiment_amd.graph import LOOPS_KEEP, LOOPS_REMOVE_ADD, get_graph

PEAK = 8e12  # HBM bytes / s
SHAPES = [(8, 16), (1, 128)]


def byte_model(kind, nnz, N, H, C, dropout):
    F = H * C
    return {
        "transformer_fwd": nnz * (8 * F + 4) + N * (2 * 4 * F + 8 * H + 4),
        "transformer_bwd_dst": nnz * (8 * F + 4) + N * (4 * 4 * F + 16 * H + 4),
        "transformer_bwd_src": nnz * (8 * F + 8 * H + 4 + (4 if dropout else 0)) + N * (4 * 4 * F + 4),
        "gatv2_fwd": nnz * (4 * F + 4) + N * (2 * 4 * F + 8 * H + 4),
        "gatv2_bwd_dst": nnz * (4 * F + 4) + N * (4 * 4 * F + 16 * H + 4),
        "gatv2_bwd_src": nnz * (8 * F + 8 * H + 4 + (4 if dropout else 0)) + N * (2 * 4 * F + 4),
    }.get(kind)


def run_shape(H, C, N, graph_tf, graph_v2, rounds, dev, res):
    F, p = H * C, 0.5
    scale = C ** -0.5
    torch.manual_seed(0)
    h = torch.randn(N, 3 * F, device=dev) * 0.5
    att = torch.randn(1, H, C, device=dev) * 0.3
    cot = torch.randn(N, F, device=dev)
    h_g = h.clone().requires_grad_(True)
    att_g = att.clone().requires_grad_(True)
    blocks = lambda t: (t[:, :F], t[:, F:2 * F], t[:, 2 * F:])

    def tf_eval():
        with torch.no_grad():
            ops.transformer_attend(*blocks(h), graph_tf, H, C, scale)

    def tf_step(training):
        h_g.grad = None
        ops.transformer_attend(*blocks(h_g), graph_tf, H, C, scale, training=training, p_drop=p).backward(cot)

    def v2_eval():
        with torch.no_grad():
            ops.gatv2_attend(h[:, :F], h[:, F:2 * F], att, graph_v2, H, C)

    def v2_step(training):
        h_g.grad = att_g.grad = None
        ops.gatv2_attend(h_g[:, :F], h_g[:, F:2 * F], att_g, graph_v2, H, C, training=training, p_drop=p).backward(cot)

    forms = {"transformer_eval": tf_eval, "transformer_step": lambda: tf_step(False),
             "transformer_step_dropout": lambda: tf_step(True), "gatv2_eval": v2_eval,
             "gatv2_step": lambda: v2_step(False), "gatv2_step_dropout": lambda: v2_step(True)}
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
                if str(kind).startswith(("transformer_", "gatv2_")):
                    times.setdefault(f"{form}/{kind}", []).append(s.elapsed_time(e))
    print(f"--- H = {H}, C = {C} (F = {F}); slots: transformer {graph_tf.fwd.nnz}, gatv2 {graph_v2.fwd.nnz}")
    for key in sorted(times):
        v = times[key]
        ms = statistics.median(v)
        form, kind = key.split("/", 1)
        nnz = graph_tf.fwd.nnz if kind.startswith("transformer") else graph_v2.fwd.nnz
        nb = byte_model(kind, nnz, N, H, C, form.endswith("dropout"))
        frac = nb / (ms * 1e-3) / PEAK
        print(f"{key:50s} {ms:9.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, n {len(v)})  {nb / 1e9:6.2f} GB  "
              f"{frac:.3f} of 8 TB/s")
        res[f"{H}x{C}/{key}_ms"] = round(ms, 3)
        res[f"{H}x{C}/{key}_frac_8TBs"] = round(frac, 3)
    for a, b in (("transformer_eval/transformer_fwd", "gatv2_eval/gatv2_fwd"),
                 ("transformer_step/transformer_bwd_dst", "gatv2_step/gatv2_bwd_dst"),
                 ("transformer_step/transformer_bwd_src", "gatv2_step/gatv2_bwd_src")):
        ratio = statistics.median(times[a]) / statistics.median(times[b])
        print(f"{a} / {b}: {ratio:.2f}x")
        res[f"{H}x{C}/{a.split('/')[1]}_over_gatv2"] = round(ratio, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer_bench: no GPU; a timing taken anywhere else says nothing (not measured)")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    ei = ei.to(dev)
    graph_tf = get_graph(ei, N, LOOPS_KEEP)
    graph_v2 = get_graph(ei, N, LOOPS_REMOVE_ADD)
    graph_tf.t2f, graph_v2.t2f  # once per graph: not part of a step
    res = {"workload": args.workload, "N": N, "slots_transformer": graph_tf.fwd.nnz, "slots_gatv2": graph_v2.fwd.nnz,
           "rounds": args.rounds}
    for H, C in SHAPES:
        run_shape(H, C, N, graph_tf, graph_v2, args.rounds, dev, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
