#!/usr/bin/env python3
"""The row gather with the gathered table stored as bfloat16 (rgbx_spmm_csr_bf16) against the fp32 gather
(rgbx_spmm_csr_f32), on workload L's synthetic graph (bench.synth: |V| = 2 M, |E| = 60 M) at d = 16, 32, 64, 128.
Everything runs in ONE process on the same graph; the forms ALTERNATE (one launch of each per round, 3 warm-up rounds,
then --runs rounds), every launch is timed with HIP events, and the median over the rounds is reported:
  fwd / fwd_w     forward CSR, one scale per row (the mean) / one weight per slot
  bwd / bwd_w     transposed CSR, no weights / one weight per slot (the mean's backward)
  f32_* / bf16_*  the fp32 entry on the fp32 table / the bf16 entry on the rounded table, same CSR, same fp32 output
  cvt             rgbx_rows_f32_to_bf16 over the [N, d] table (what a training step pays in front of each bf16 gather)
Byte model (every array once, gathered rows once per slot; per target row of degree deg, summed over the graph):
  fp32   deg 4 d + deg (4 [+ 4 with w]) + 4 d        bf16   deg 2 d + the same index and output bytes
  cvt    4 d read + 2 d written per row
Per width the measured time ratio bf16 / f32 stands beside the ratio of the two byte counts (the expectation if both
kernels moved their bytes at the same rate); a width that misses it by more than 5 % is marked. Before timing, every bf16
form is compared with the fp32 kernel run on the WIDENED table (same values, same sums up to summation order).
--alt LIB[,LIB...]: further builds of the library (say with another -DRGBX_BF16_UNROLL) whose bf16 entry runs in the same
rounds, reported as bf16@<n>_*.
Prints a table, then one JSON line. Usage: python tools/bf16_gather_bench.py [--workload L|S] [--runs R] [--out FILE]"""
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
from rgb_experiment_amd import _lib, ops
from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph

PEAK = 8e12  # HBM bytes / s
WIDTHS = (16, 32, 64, 128)


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


def bf16_call(lib, csr, w, rs, xb, out):
    """rgbx_spmm_csr_bf16 through `lib` (the in-tree build or an --alt one), fp32 output."""
    N, d = csr.N, xb.size(1)
    split, _scratch = csr.split_arg(d, xb.device)
    _lib.check(lib.rgbx_spmm_csr_bf16(csr.rowptr.data_ptr(), csr.col.data_ptr(), _lib.ptr(w), _lib.ptr(rs), xb.data_ptr(), d,
                                      None, 0, None, out.data_ptr(), d, None, 0, N, d, 1.0, 0.0,
                                      None if split is None else ctypes.byref(split), _lib.stream_ptr()),
               "rgbx_spmm_csr_bf16")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="L", choices=sorted(WORKLOADS))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--alt", default="", help="comma-separated paths of further builds of librgbx_hip.so")
    ap.add_argument("--out", default=None, help="also write the table and the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 7:
        ap.error("--runs must be at least 7")
    wl = WORKLOADS[args.workload]
    N, E = wl["N"], wl["E"]
    dev = torch.device("cuda:0")
    ei, _, _ = synth(N, E, 4)
    g = get_graph(ei.to(dev), N, LOOPS_KEEP)
    g.bwd, g.inv_deg, g.w_mean_t  # the sort and the mean's weights: once per graph, not timed
    nnz = g.fwd.nnz
    w_fwd = torch.rand(nnz, device=dev) + 0.5
    alts = [(f"bf16@{i + 1}", _lib.bind(p, strict=False)) for i, p in enumerate(a for a in args.alt.split(",") if a)]
    lines = [f"workload {args.workload}: N = {N}, E' = {nnz} slots (mean degree {nnz / N:.1f}), {args.runs} rounds, medians"]
    for i, p in enumerate(a for a in args.alt.split(",") if a):
        lines.append(f"bf16@{i + 1} = {p}")
    res = {"workload": args.workload, "N": N, "E": E, "nnz": nnz, "runs": args.runs}
    cases = {"fwd": (g.fwd, None, g.inv_deg, 0), "fwd_w": (g.fwd, w_fwd, None, 4),
             "bwd": (g.bwd, None, None, 0), "bwd_w": (g.bwd, g.w_mean_t, None, 4)}
    for d in WIDTHS:
        x = torch.randn(N, d, device=dev)
        xb = ops.to_bf16_rows(x)
        xw = xb.float()  # the widened table: what the bf16 kernel sums, as fp32 rows
        out32, out16 = torch.empty(N, d, device=dev), torch.empty(N, d, device=dev)
        forms, nbytes = {}, {}
        for name, (csr, w, rs, wb) in cases.items():
            ref = ops.spmm_raw(csr, w, rs, xw).clone()
            got = ops.spmm_bf16_raw(csr, w, rs, xb)
            diff = (got - ref).abs().max().item()
            res[f"{name}_d{d}_max_abs_diff_vs_f32_on_widened"] = diff
            if not diff <= 1e-4 * max(1.0, ref.abs().max().item()):
                raise SystemExit(f"d = {d} {name}: bf16 gather differs from the fp32 gather on the widened table by {diff}")
            side = nnz * (4 + wb) + 4 * N * d + 4 * (N + 1) + (4 * N if rs is not None else 0)
            nbytes[f"f32_{name}"], nbytes[f"bf16_{name}"] = nnz * 4 * d + side, nnz * 2 * d + side
            forms[f"f32_{name}"] = lambda csr=csr, w=w, rs=rs: ops.spmm_raw(csr, w, rs, x, out=out32)
            forms[f"bf16_{name}"] = lambda csr=csr, w=w, rs=rs: ops.spmm_bf16_raw(csr, w, rs, xb, out=out16)
            for tag, lib in alts:
                nbytes[f"{tag}_{name}"] = nbytes[f"bf16_{name}"]
                forms[f"{tag}_{name}"] = lambda csr=csr, w=w, rs=rs, lib=lib: bf16_call(lib, csr, w, rs, xb, out16)
        forms["cvt"], nbytes["cvt"] = (lambda: ops.to_bf16_rows(x)), 6 * N * d
        t = alternate_ms(forms, args.runs)
        for k, ms in t.items():
            res[f"{k}_d{d}_ms"], res[f"{k}_d{d}_bytes"] = ms, nbytes[k]
            lines.append(f"d = {d:3d}   {k:12s} {ms:8.3f} ms   {nbytes[k] / 1e9:6.2f} GB algorithmic, "
                         f"{nbytes[k] / (ms * 1e-3) / 1e12:5.2f} TB/s ({100 * nbytes[k] / (ms * 1e-3) / PEAK:4.1f} % of 8 TB/s)")
        for tag in ["bf16"] + [a for a, _ in alts]:
            for name in cases:
                ratio, expect = t[f"{tag}_{name}"] / t[f"f32_{name}"], nbytes[f"{tag}_{name}"] / nbytes[f"f32_{name}"]
                res[f"{tag}_over_f32_{name}_d{d}"], res[f"bytes_{tag}_over_f32_{name}_d{d}"] = ratio, expect
                miss = "" if ratio <= 1.05 * expect else f"   MISSES the byte model by {100 * (ratio / expect - 1):.0f} %"
                lines.append(f"d = {d:3d}   {tag}_{name} / f32_{name:6s} time x{ratio:5.2f}   bytes x{expect:5.2f}{miss}")
            name = "fwd"
            with_cvt = (t[f"{tag}_{name}"] + t["cvt"]) / t[f"f32_{name}"]
            res[f"{tag}_plus_cvt_over_f32_{name}_d{d}"] = with_cvt
            lines.append(f"d = {d:3d}   ({tag}_{name} + cvt) / f32_{name}   time x{with_cvt:5.2f}   (a training step converts in front "
                         "of every gather)")
        del x, xb, xw, out32, out16
    text = "\n".join(lines) + "\n" + json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
