#!/usr/bin/env python3
"""FAConv on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at C = 64, forms run alternately in
one process, timed with HIP events, medians reported:
  1. the fused forward (rgbx_faconv_fwd_f32) in eval and in training mode (dropout 0.5);
  2. the two fused backward passes (rgbx_faconv_bwd_dst_f32, rgbx_faconv_bwd_src_f32), training mode;
  3. the composed path: forward (edge coefficients + weighted gather) and forward + backward;
  4. the yardstick: the plain GCN-weighted gather (rgbx_spmm_csr_f32) at the same width on the same graph;
  5. the default experiment(model=FAGCN(**defaults)) epoch (training forward + backward + Adam step, eval forward).
Per launch: ms, algorithmic bytes, fraction of 8 TB/s. Prints a table, then one JSON line.
Usage: python tools/fagcn_bench.py [--rounds R] [--reps K] [--workload L|S] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import WORKLOADS, synth
from rgb_experiment_amd import InitialParameters, _lib, ops
from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
from rgb_experiment_amd.models import FAGCN

PEAK = 8e12  # HBM bytes / s


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    wl = WORKLOADS[args.workload]
    N, E, F = wl["N"], wl["E"], wl["d"]
    C, n_cls, p, eps = 64, 16, 0.5, 0.3
    dev = torch.device("cuda:0")
    ei, x, y = synth(N, E, F)
    ei, x, y = ei.to(dev), x.to(dev), (y % n_cls).to(dev)
    g = get_graph(ei, N, LOOPS_ADD_REMAINING)
    nnz = g.fwd.nnz
    g.w, g.w_t, g.t2f  # once per graph: not part of a step
    lib = _lib.load()
    torch.manual_seed(0)
    h = torch.randn(N, C, device=dev)
    h0 = torch.randn(N, C, device=dev)
    gout = torch.randn(N, C, device=dev)
    att = torch.randn(2, C, device=dev) / C ** 0.5
    seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
    alr = torch.empty(N, 2, device=dev)
    g_alr = torch.empty(N, 2, device=dev)
    out = torch.empty(N, C, device=dev)
    g_x = torch.empty(N, C, device=dev)
    P, st = _lib.ptr, _lib.stream_ptr
    fs, fs_keep = g.fwd.split_arg(C + 1, dev)
    bs, bs_keep = g.bwd.split_arg(C + 1, dev)
    ref = lambda s: None if s is None else ctypes.byref(s)

    def scores():
        _lib.check(lib.rgbx_faconv_scores_f32(P(h), C, att[0].data_ptr(), att[1].data_ptr(), P(alr), N, C, st()), "scores")

    def fwd(sd):
        _lib.check(lib.rgbx_faconv_fwd_f32(P(g.fwd.rowptr), P(g.fwd.col), P(g.w), P(h), C, P(alr), P(h0), C, eps, P(out), C,
                                           N, C, P(sd), p, ref(fs), st()), "fwd")

    def bwd_dst():
        _lib.check(lib.rgbx_faconv_bwd_dst_f32(P(g.fwd.rowptr), P(g.fwd.col), P(g.w), P(h), C, P(alr), P(gout), C, P(g_alr),
                                               N, C, P(seed), p, ref(fs), st()), "bwd_dst")

    def bwd_src():
        _lib.check(lib.rgbx_faconv_bwd_src_f32(P(g.bwd.rowptr), P(g.bwd.col), P(g.w_t), P(g.t2f), P(h), C, P(alr), P(gout),
                                               C, att[0].data_ptr(), att[1].data_ptr(), P(g_alr), P(g_x), C, N, C, P(seed), p,
                                               ref(bs), st()), "bwd_src")

    hg = h.clone().requires_grad_(True)
    al, ar = (att[i:i + 1].clone().requires_grad_(True) for i in (0, 1))

    def composed_fwd():
        with torch.no_grad():
            ops.faconv(h, h0, al, ar, g, eps=eps, form="composed")

    def step(form):
        hg.grad = None
        (ops.faconv(hg, h0, al, ar, g, eps=eps, training=True, p_drop=p, form=form) * gout).sum().backward()

    model = FAGCN(input_dim=F, output_dim=n_cls, **InitialParameters.defaults_for("FAGCN")).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    train_mask = torch.rand(N, device=dev) < 0.6

    def epoch():
        model.train()
        opt.zero_grad()
        ops.ce_from_logits(model(x, ei)["emb"], y, train_mask)[0].backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            model(x, ei)

    scores()
    forms = {"scores": scores, "fused_fwd_eval": lambda: fwd(None), "fused_fwd_train": lambda: fwd(seed),
             "fused_bwd_dst": bwd_dst, "fused_bwd_src": bwd_src,
             "gcn_gather": lambda: ops.spmm_raw(g.fwd, g.w, None, h, out=out),
             "composed_fwd_eval": composed_fwd, "fused_layer_step": lambda: step("fused"),
             "composed_layer_step": lambda: step("composed"), "fagcn_epoch": epoch}
    for fn in forms.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.rounds):  # alternately, so drift in clocks or neighbours hits all forms alike
        for k, fn in forms.items():
            times[k].append(timed(fn, args.reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    row = C * 4
    # algorithmic bytes per launch: per slot the gathered row + col + w + the 4-byte score; per node what is read / stored
    nbytes = {
        "scores": N * (row + 8),
        "fused_fwd_eval": nnz * (row + 12) + N * (2 * row + 4 + 4),          # x0 row in, out row, ar, rowptr
        "fused_fwd_train": nnz * (row + 12) + N * (2 * row + 4 + 4),
        "fused_bwd_dst": nnz * (row + 12) + N * (row + 4 + 4 + 4),           # gout row in, ar, g_ar out, rowptr
        "fused_bwd_src": nnz * (row + 16) + N * (2 * row + 4 + 4 + 4 + 4),   # + t2f; x row in, g_x row out, al, g_ar, g_al
        "gcn_gather": nnz * (row + 8) + N * (row + 4),
        "composed_fwd_eval": nnz * (12 + 4) + nnz * (row + 8) + N * (2 * row + 4) + N * (row + 8),
    }
    lines = [f"FAConv at workload {args.workload}: N = {N}, E' = {nnz}, C = {C}, dropout {p}; median of {args.rounds} "
             f"rounds x {args.reps} launches"]
    res = {"workload": args.workload, "N": N, "nnz": nnz, "C": C}
    for k, ms in med.items():
        res[f"{k}_ms"] = round(ms, 3)
        tail = ""
        if k in nbytes:
            res[f"{k}_GB"] = round(nbytes[k] / 1e9, 3)
            res[f"{k}_frac_8TBs"] = round(nbytes[k] / (ms * 1e-3) / PEAK, 3)
            tail = f"  {nbytes[k] / 1e9:7.3f} GB  {res[f'{k}_frac_8TBs']:.3f} of 8 TB/s"
        lines.append(f"{k:22s} {ms:9.3f} ms{tail}")
    res["fused_fwd_over_gcn_gather"] = round(med["fused_fwd_eval"] / med["gcn_gather"], 3)
    res["composed_over_fused_step"] = round(med["composed_layer_step"] / med["fused_layer_step"], 3)
    lines.append(f"fused eval forward / plain GCN gather: {res['fused_fwd_over_gcn_gather']:.3f}")
    lines.append(f"composed / fused layer step (fwd + bwd, training): {res['composed_over_fused_step']:.3f}")
    lines.append(json.dumps(res))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
