#!/usr/bin/env python3
"""bench.py — the reference's hot loop (itexperiments.py:417-473) on synthetic graphs, MI355X.

One STEP = one epoch of the reference loop body for a 2-layer GCN at d = 128: 1 train forward +
backward + Adam step, then 2 eval forwards (val, test) = 7 aggregations over all E' edges (6 forward, 1
transposed: the input layer aggregates first, so its weight gradient needs no pass through A_hat^T), each
fused with its layer's dense transform (fp32 MFMA) where the shapes allow, + the weight-gradient GEMMs,
BatchNorm and the loss. `value` counts the edges actually aggregated (7 * E' per step), not the 8 propagates
of the transform-first formulation. Nothing of the epoch is skipped or cached across steps; two things are
computed in a different FORM than the reference writes them, with the same values: the eval-mode BatchNorm is
folded into the preceding layer's weights, and loss / accuracy / loss gradient are taken from the logits
(cross-entropy = NLLLoss o log_softmax) so the log-probabilities are never written out — for the conv stacks inside
the last layer's kernel, whose logits then go from the MFMA tiles into the loss (training: into the loss gradient) without a
round trip through HBM.
The five numbers the reference reads with .item() inside the loop body are read once, at the end of the step.
Inputs are resident in HBM before the timed region.

Metric (BASELINE.json): "aggregated edges/sec + training epochs/sec, full-graph GCN d=128".
  value            = edges aggregated per second over the WHOLE step = 7 * E' * steps / wall time
  epochs_per_s     = steps / wall time
  spmm_edges_per_s = E' / mean aggregation kernel time (HIP events on the launch stream)
  roofline         = algorithmic bytes of one aggregation launch / its mean duration vs 8 TB/s HBM

A plain run sets up, warms up, times --steps steps and prints the line; `--full` adds, on one GPU, every secondary leg
after the headline (yardstick, parity checks, CPU baseline, training-step-only and hipGraph timings and, for the GCN on
workload L, the other graphs, sizes and shapes). `--dump-outputs DIR` writes what the last timed step computed as .npy
files (dump_outputs).

Launch: `python bench.py [--gpus 1]`; `python bench.py --gpus N` starts N ranks (one per GPU) as child
processes under torch.distributed.run; the driver's own `python -m torch.distributed.run ... bench.py --gpus N`
(RANK / LOCAL_RANK / WORLD_SIZE in the environment) runs the ranks directly. The graph is then 1-D
node-partitioned over the ranks with RCCL all-to-all exchanges per propagate (strong scaling: total work fixed).
`--emulate-rank P` runs exactly rank 0's kernel launches of a P-rank job on ONE GPU (exchanges replaced by
stand-in rows) and reports its compute time per epoch next to the bytes every xGMI link would carry.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# dmabuf IPC for RCCL between the ranks of one node: must be in the environment before the HIP runtime starts
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch
import torch.distributed as dist

WORKLOADS = {
    # BASELINE.json configs[1] / the north-star target size (S and L); T = the CLI test's toy size
    "T": dict(N=3_000, E=40_000, d=32, name="toy |V|=3k |E|=40k d=32, 2-layer GCN"),
    "S": dict(N=200_000, E=4_000_000, d=128, name="synthetic |V|=200k |E|=4M d=128, 2-layer GCN"),
    "L": dict(N=2_000_000, E=60_000_000, d=128, name="synthetic |V|=2M |E|=60M d=128, 2-layer GCN"),
}
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec

# event kind (ops._Timed) -> the HIP kernel that launch is
KERNEL_OF_KIND = {
    "gcn_linear_fwd": "spmm_linear_kernel", "mean_linear_fwd": "spmm_linear_kernel",
    "gcn_linear_bwd": "spmm_linear_kernel", "mean_linear_bwd": "spmm_linear_kernel",
    "sum_linear_fwd": "spmm_linear_kernel", "sum_linear_bwd": "spmm_linear_kernel",
    # replicate scheme (dist.ReplicaGraph): first layer on all N rows, second on the [n_local x N] rectangular CSR
    "replica_gcn_linear_fwd": "spmm_linear_kernel", "tail_gcn_linear_fwd": "spmm_linear_kernel",
    "tail_gcn_linear_bwd": "spmm_linear_kernel", "tail_gcn_bwd": "spmm_csr_kernel", "replica_fwd": "spmm_csr_kernel",
    "tail_fwd": "spmm_csr_kernel", "tail_bwd": "spmm_csr_kernel",
    "gcn_fwd": "spmm_csr_kernel", "gcn_bwd": "spmm_csr_kernel", "mean_fwd": "spmm_csr_kernel",
    "sum_fwd": "spmm_csr_kernel", "sum_bwd": "spmm_csr_kernel",
    "mean_bwd": "spmm_csr_kernel", "appnp_fwd": "spmm_csr_kernel (K launches)",
    "appnp_bwd": "spmm_csr_kernel (K launches)", "gat_fwd": "gat_fwd_kernel", "gat_bwd_src": "gat_bwd_src_kernel",
    "gat_bwd_prep": "gat_bwd_prep_kernel",
    # single-head GATConv run aggregate-first (ops.gat_attend_linear): coefficients per edge, then the fused kernel
    "gat_linear_fwd": "spmm_linear_kernel", "gat_edge_softmax": "gat_edge_softmax_kernel",
    "dist_fwd_local": "spmm_csr_kernel", "dist_fwd_remote": "spmm_csr_kernel", "dist_bwd_local": "spmm_csr_kernel",
    "dist_bwd_remote": "spmm_csr_kernel", "dist_fwd_resident": "spmm_csr_kernel",
    "dist_fwd_colshard": "spmm_csr_kernel", "dist_bwd_colshard": "spmm_csr_kernel",
    # fused per-rank schedule (dist/stack.py): the return stage's dense launches carry no aggregation bytes
    "dist_fwd_appnp_colshard": "spmm_csr_kernel (K launches)", "dist_bwd_appnp_colshard": "spmm_csr_kernel (K launches)",
}
AGG_KINDS = tuple(KERNEL_OF_KIND)
KERNEL_SOURCES = {  # files whose text decides what the kernel does: a PMC figure is only valid for this hash
    "spmm_linear_kernel": ("spmm_linear.hip", "spmm_internal.h", "rgbx_common.h"),
    "spmm_csr_kernel": ("spmm.hip", "spmm_internal.h", "rgbx_common.h"),
    "gat_fwd_kernel": ("gat.hip", "spmm_internal.h", "rgbx_common.h"),
    "gat_bwd_src_kernel": ("gat.hip", "spmm_internal.h", "rgbx_common.h"),
}


def powerlaw_endpoints(N, E, seed, exponent=2.0):
    """E node ids with a Zipf-like popularity: id = perm[floor(N u^exponent)], u uniform — node k of the popularity
    order is drawn with density ~ k^(1/exponent - 1) (exponent 2: the top node collects E / sqrt(N) entries, 42 k of
    60 M at N = 2 M, the order of the hubs of ogbn-products / Reddit); `perm` scatters the popular nodes over the id
    range as real datasets do."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(E, generator=g, dtype=torch.float64)
    rank = (u.pow(exponent) * N).long().clamp_(max=N - 1)
    return torch.randperm(N, generator=g)[rank]


def synth(N, E, d, degree="uniform"):
    """directed iid-uniform endpoints (self-loops / duplicates left in), N(0,1) features,
    uniform labels over d classes; fixed seeds. degree="powerlaw" (secondary runs, never the headline): sources AND
    targets follow independent Zipf-like popularities, so both the forward and the transposed CSR have hub rows."""
    if degree == "powerlaw":
        ei = torch.stack([powerlaw_endpoints(N, E, 1234561), powerlaw_endpoints(N, E, 1234562)])
    else:
        ei = torch.randint(0, N, (2, E), generator=torch.Generator().manual_seed(1234567), dtype=torch.int64)
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(1234568))
    y = torch.randint(0, d, (N,), generator=torch.Generator().manual_seed(1234569))
    return ei, x, y


_MASKS = {}


def split_masks(y):
    """The reference's default split: get_whole_mask(y, '6-2-2', 123456789) (itexperiments.py:47-49,215), the
    product's bit-exact restatement (golden G4). Seconds at 2M nodes (a Python-list shuffle), outside the timing."""
    from rgb_experiment_amd.utils import get_whole_mask
    key = (y.data_ptr(), y.numel(), y._version)
    if _MASKS.get("key") != key:  # the secondary legs of a line split the same labels again
        _MASKS["key"], _MASKS["val"] = key, list(get_whole_mask(y, "6-2-2", 123456789))
    return list(_MASKS["val"])


def kernel_source_hash(kernel):
    base = kernel.split(" ")[0]
    files = KERNEL_SOURCES.get(base)
    if not files:
        return None
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, "rgb_experiment_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_traffic(workload, model, kernel, world):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE x2 +
    WRITE_SIZE, gfx950 correction; profiles/pmc_traffic_<workload>_<model>.json, written by tools/profile_summary.py).
    PMC counters cannot be read from inside this process, so this is the last profiled value — returned only when
    the file was measured on the SAME kernel sources (hash stamp); otherwise None plus the reason."""
    path = os.path.join(ROOT, "profiles", f"pmc_traffic_{workload}_{model}.json")
    if world != 1:
        return None, "single-GPU figure only"
    if not os.path.exists(path):
        return None, "no PMC pass committed for this workload / model"
    with open(path) as f:
        rec = json.load(f)
    base = kernel.split(" ")[0]
    if rec.get("kernel") != base:
        return None, f"committed PMC pass is for {rec.get('kernel')}, the dominant kernel now is {base}"
    if rec.get("source_hash") != kernel_source_hash(kernel):
        return None, "kernel sources changed since the committed PMC pass (stale)"
    return rec["traffic_bytes_per_launch"], f"rocprofv3 PMC, {rec.get('measured', '?')}"


def gat_launch_bytes(n_rows, nnz, H, C):
    """Algorithmic bytes per launch of the GAT kernels of ONE layer (H heads of C channels), from the passes that exist
    (rgb_experiment_amd/ops.py _GATAttend, csrc/gat.hip): {"fwd_infer", "fwd_train", "bwd_src", "bwd_prep"}.
    Heads spanning <= 8 lanes (ops._scores_in_kernel) form both score products inside the aggregation kernels from rows
    they hold anyway; wider heads gather a_src[j] (4H bytes per edge) and read a_dst.
      forward  : per edge col + the source row (+ a_src); per target the out row, max and 1/sum (+ its own row for
                 a_dst in-kernel, else a_dst); the training form also stores out_pos [HC], a_pos [H] and a_dst [H]
      bwd_src  : per edge col + the target's gout row + its 16-byte-per-head record (+ a_src); per source its own
                 row, the g_hfeat row, g_a_src, g_a_dst
      bwd_prep : streaming: out, gout, out_pos rows + (a_dst, max, 1/sum, a_pos) in, records + g_a_dst out
    No per-edge tensor is written by any pass (round 2 removed the ds [E', H] store and its width-H segment sum)."""
    from rgb_experiment_amd.ops import _scores_in_kernel
    d = H * C
    inside = _scores_in_kernel(C)
    edge = nnz * (4 + 4 * d + (0 if inside else 4 * H))
    fwd = edge + n_rows * (4 * d + 8 * H + (4 * d if inside else 4 * H)) + 4 * (n_rows + 1)
    return {"fwd_infer": fwd, "fwd_train": fwd + n_rows * (4 * d + 8 * H),
            "bwd_src": nnz * (4 + 4 * d + 16 * H + (0 if inside else 4 * H)) + n_rows * (8 * d + 8 * H)
            + 4 * (n_rows + 1),
            "bwd_prep": n_rows * (12 * d + 36 * H)}


def gat_single_head_linear(d):
    """The bench model's last layer (one head, d -> d classes) runs aggregate-first (ops.gat_linear_ok)."""
    return d in (64, 128, 256) and d <= 128


def gat_linear_launch_bytes(n_rows, nnz, d):
    """The single-head layer run aggregate-first (ops._GATAttendLinear), per launch:
      edge_softmax : per edge col + the a_src gather + the alpha store (training: + alpha_pos); per target rowptr, a_dst,
                     max, 1/sum (training: + a_pos)
      fwd          : rgbx_fused_layer_f32 with w = alpha and the loss epilogue: per edge col + alpha + the source row;
                     per target rowptr, label and mask; inference stores nothing (statistics only); training reads
                     alpha_pos per edge and stores the aggregate, its positive-score part and the loss gradient"""
    soft = nnz * 12 + n_rows * 12 + 4 * (n_rows + 1)
    fwd = nnz * (8 + 4 * d) + n_rows * 9 + 4 * (n_rows + 1)
    return {"edge_softmax_infer": soft, "edge_softmax_train": soft + nnz * 4 + n_rows * 4,
            "fwd_infer": fwd, "fwd_train": fwd + nnz * 4 + n_rows * 12 * d}


def gat_alg_bytes(n_rows, nnz, d, H=8):
    """Mean algorithmic bytes per propagate of a 2-layer GAT epoch (layer 1: H heads of d/H channels, layer 2: one head
    of d): 4 inference-form forwards (two eval forwards), 2 training-form forwards, 2 backward source passes with
    their streaming prep pass — 8 propagates. Layer 2's forwards are the aggregate-first launches where they apply."""
    l1, l2 = gat_launch_bytes(n_rows, nnz, H, d // H), gat_launch_bytes(n_rows, nnz, 1, d)
    tot = sum(2 * l["fwd_infer"] + l["fwd_train"] + l["bwd_src"] + l["bwd_prep"] for l in (l1, l2))
    if gat_single_head_linear(d):
        lin = gat_linear_launch_bytes(n_rows, nnz, d)
        tot += (2 * (lin["fwd_infer"] + lin["edge_softmax_infer"]) + lin["fwd_train"] + lin["edge_softmax_train"]
                - 2 * l2["fwd_infer"] - l2["fwd_train"])
    return tot / 8


def gat_fwd_launch_bytes(n_rows, nnz, d, H=8):
    """Mean over the `gat_fwd` launches of an epoch (per layer: 2 inference-form, 1 training-form): both layers, or
    layer 1 alone when the single-head layer 2 runs aggregate-first (kinds gat_edge_softmax + gat_linear_fwd)."""
    l1, l2 = gat_launch_bytes(n_rows, nnz, H, d // H), gat_launch_bytes(n_rows, nnz, 1, d)
    layers = (l1,) if gat_single_head_linear(d) else (l1, l2)
    return sum(2 * l["fwd_infer"] + l["fwd_train"] for l in layers) / (3 * len(layers))


def spmm_alg_bytes(n_rows, nnz, d):
    """gathered rows + col + weight per edge, output row + rowptr per node."""
    return nnz * (4 * d + 8) + n_rows * 4 * d + 4 * (n_rows + 1)


def spmm_compulsory_bytes(n_rows, nnz, d):
    """every feature row read once and written once, the CSR stream, rowptr."""
    return 2 * n_rows * 4 * d + nnz * 8 + 4 * (n_rows + 1)


def cpu_model():
    """Model name of the host CPU the baseline ran on (SURVEY 8d asks for it beside the core count)."""
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def host_cores():
    """Cores this process may actually use: the cgroup CPU quota if there is one (a one-GPU box grants
    a share of the host, not all of os.cpu_count()), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


MODELS = {
    # name: (constructor kwargs, propagates per epoch = 3 forwards + 1 backward, loops_mode, weighting kind)
    # gcn: 2 + 2 + 2 forward SpMMs and ONE transposed SpMM (layer 2); layer 1's weight gradient is taken
    # against A_hat x, so nothing flows back through A_hat^T there (nn/conv.py GCNConv)
    "gcn": (dict(num_layers=2, hidden_unit=128, dropout_rate=0.5), 7, 1, "gcn"),
    "graphsage": (dict(num_layers=2, hidden_unit=128, dropout_rate=0.5), 7, 2, "mean"),
    "graphsage2": (dict(num_layers=2, hidden_unit=128, dropout_rate=0.5), 7, 0, "mean"),
    "gat": (dict(num_layers=2, hidden_unit=16, heads=8, dropout_rate=0.5), 8, 2, "gat"),
    "appnpstack": (dict(hidden_unit=64, K=10, alpha=0.1, dropout_rate=0.5), 40, 1, "gcn"),
    # SURVEY 8(f) "next" rows: callers of the same propagate kernels
    # sgc: K = 2 propagates of the static features per forward, nothing flows back through them (cached=False: the
    # reference's cached=True would leave an epoch without any propagate after the first)
    "sgc": (dict(K=2, cached=False), 6, 1, "gcn"),
    # gin: unweighted sum over the edges as given, 2 blocks per forward; layer 1's input needs no gradient
    "gin": (dict(num_layers=2, hidden_unit=128, dropout_rate=0.5), 7, 0, "sum"),
    # dagnn: K = 10 gcn-normalised hops of the MLP output per forward, all 10 transposed in the backward
    "dagnn": (dict(hidden_dim=64, K=10, dropout_rate=0.5), 40, 1, "gcn"),
}
DEEP = {"appnpstack": 2, "dagnn": 2}  # K hops cover the whole graph: the sampled logit check runs these at K = 2


def model_class(name):
    from rgb_experiment_amd import models as M
    return {"gcn": M.GCN, "graphsage": M.GraphSAGE, "graphsage2": M.GraphSAGE2, "gat": M.GAT,
            "appnpstack": M.APPNPStack, "sgc": M.SGC, "gin": M.GIN, "dagnn": M.DAGNN}[name]


# ---------------------------------------------------------------------------------------------------------------
# CPU legs: the oracle as the checker of THIS run's results and as the timed CPU baseline (rank 0, one GPU only)

def cpu_baseline(ei, x, N, budget_s=20.0, fused=None):
    """The oracle timed on the host cores, one GCN propagate at d = 128 (rank 0, N = 1 only).
    Primary: the C/OpenMP restatement (oracle/propagate_ref.c, per-target CSR sums over all host threads)
    on the WHOLE rewritten edge list — the strongest plain CPU form of the same arithmetic.
    Also reported: the PyG-style dataflow of the Python oracle (index_select -> multiply -> index_add_,
    which materialises [E, d]) on a bounded 8 M-edge sample, which is what the reference's CPU path does.
    `fused` = (out, W, b): the result of the TIMED kernel (ops.propagate_linear = rgbx_spmm_linear_f32: aggregate +
    transform of the whole workload with the model's first-layer weights), checked here against the C restatement's
    propagate followed by a CPU matmul: the full-size parity of this very run rides along on the line."""
    from oracle import ref_cpu as O
    cores = host_cores()
    torch.set_num_threads(cores)
    rei, w = O.gcn_norm(ei, None, N)
    M = min(rei.size(1), 8_000_000)
    sub, wsub = rei[:, :M].contiguous(), w[:M].contiguous()
    O.propagate(sub[:, :100_000], x, N, wsub[:100_000], "add")  # warm-up
    times = []
    t_end = time.perf_counter() + budget_s / 2
    while len(times) < 3 or (time.perf_counter() < t_end and len(times) < 6):
        t0 = time.perf_counter()
        O.propagate(sub, x, N, wsub, "add")
        times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    dataflow = {"value": M / med, "unit": "edges/s", "cores": torch.get_num_threads(), "seconds_per_run": med,
                "what": f"oracle.propagate (index_select*w -> index_add_, the PyG dataflow) over the first {M} of "
                        f"the {rei.size(1)} rewritten edges, median of {len(times)} runs"}
    try:
        rowptr, col, perm = O.csr_from_edges(rei[1], rei[0], torch.arange(rei.size(1)), N)
        ws = w[perm.long()].contiguous()
        threads = min(O.c_threads(), cores)
        cpu_out = O.propagate_c_csr(rowptr, col, ws, x, "add", threads)  # warm-up (page faults, thread pool)
        parity = None
        if fused is not None:
            hip_out, W, b = fused
            want = cpu_out @ W.t() + b
            parity = {"kernel": "rgbx_spmm_linear_f32 (ops.propagate_linear, the launch the timed region makes)",
                      "checker": "oracle_propagate_csr_f32 (C restatement) then a CPU matmul with the same weights",
                      "max_abs_diff_hip_vs_cpu": (hip_out - want).abs().max().item(),
                      "max_abs_value": want.abs().max().item(), "rows": N, "width_in": x.size(1),
                      "width_out": W.size(0)}
            del want
        del cpu_out
        t2 = []
        t_end = time.perf_counter() + budget_s / 2
        while len(t2) < 3 or (time.perf_counter() < t_end and len(t2) < 20):
            t0 = time.perf_counter()
            O.propagate_c_csr(rowptr, col, ws, x, "add", threads)
            t2.append(time.perf_counter() - t0)
        t2.sort()
        m2 = t2[len(t2) // 2]
        return {"value": rei.size(1) / m2, "unit": "edges/s", "cores": threads, "kind": "port",
                "sample": f"oracle/propagate_ref.c oracle_propagate_csr_f32 (C + OpenMP, {threads} threads) over all "
                          f"{rei.size(1)} rewritten edges of one GCN propagate, d=128, median of {len(t2)} runs",
                "seconds_per_run": m2, "cpu_model": cpu_model(), "pyg_dataflow_variant": dataflow,
                "parity_at_full_size": parity}
    except Exception as exc:  # C restatement not built: fall back to the Python oracle's number
        dataflow.update({"kind": "port", "sample": dataflow.pop("what"), "cpu_model": cpu_model(),
                         "c_restatement_error": repr(exc)})
        return dataflow


def sampled_logit_parity(name, model, ei, x, x_d, ei_d, n_targets=None):
    """Whole-model logits of this run's (trained) model at sampled target rows against the UNCHANGED oracle forward
    on the targets' L-hop in-neighbourhood (oracle/sampled.py). APPNP: K = 10 hops cover the whole graph, so the
    sampled check runs the same weights with K = 2 (the K = 10 recurrence itself is pinned by golden G3 and by the
    linearity / adjoint tests at full size)."""
    from oracle import sampled as S
    kw = dict(MODELS[name][0])
    for k in ("dropout_rate", "hidden_unit", "hidden_dim", "cached"):
        kw.pop(k, None)
    N = x.size(0)
    if n_targets is None:  # gcn_norm models complete the outer in-degrees with dummy edges: keep those bounded
        n_targets = 96 if name in ("gcn", "appnpstack", "sgc", "dagnn") else 768
    targets = S.pick_targets(N, n_targets)
    was_training = model.training
    model.eval()
    run = model
    if name in DEEP:
        kw["K"] = DEEP[name]
        run = model_class(name)(input_dim=x.size(1), output_dim=model.lin2.out_features,
                                **{**MODELS[name][0], "K": DEEP[name]})
        run.load_state_dict(model.state_dict())
        run.to(x_d.device).eval()
    with torch.no_grad():
        got = run(x_d, ei_d)["emb"][targets.to(x_d.device)].cpu()
    model.train(was_training)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    t0 = time.perf_counter()
    want, info = S.sampled_logits(name, sd, x, ei, targets, **kw)
    info.update({"max_abs_diff_hip_vs_oracle": (got - want).abs().max().item(),
                 "max_abs_logit": want.abs().max().item(), "tolerance": 1e-4, "oracle_seconds": time.perf_counter() - t0,
                 "what": f"eval-mode {name} logits of {targets.numel()} sampled nodes: HIP forward over the whole graph vs "
                         "oracle.ref_cpu forward on their in-neighbourhood" + (" (K=2 instance of the same weights)"
                                                                                if name in DEEP else "")})
    return info


def gradient_parity_S(dev, name="gcn"):
    """BACKWARD parity at BASELINE workload S (|V| = 200 k, |E| = 4 M, d = 128; reference itexperiments.py:439): one
    train-mode forward + backward of the benchmark's model on the GPU — loss inside the last conv's kernel, as the timed
    region runs it — against the FULL oracle (oracle.ref_cpu: the PyG dataflow under torch autograd, 2 GB edge-sized
    temporaries), every parameter's gradient. The L-size statement of the same check runs in `-m gpu`
    (tests/test_gpu_fullsize.py::test_model_gradients_at_benchmark_size_L, against oracle/large.py)."""
    from oracle import large as OL
    from oracle import ref_cpu as O
    from rgb_experiment_amd.graph import clear_cache
    from rgb_experiment_amd.models._stack import masked_ce
    t0 = time.perf_counter()
    wl = WORKLOADS["S"]
    ei, x, y = synth(wl["N"], wl["E"], wl["d"])
    mask = split_masks(y)[0]
    torch.manual_seed(14530529)
    model = model_class(name)(input_dim=wl["d"], output_dim=wl["d"], **MODELS[name][0])
    with torch.no_grad():  # biases / BatchNorm affine off their initial 0 / 1
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.to(dev).train()
    loss = masked_ce(model, {"x": x.to(dev), "edge_index": ei.to(dev)}, y.to(dev), mask.to(dev))[0]
    loss.backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters()}
    del model
    clear_cache()
    ref_sd = {k: v.clone().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in sd.items()}
    torch.set_num_threads(host_cores())
    ref_loss = OL.masked_nll(O.gcn_forward(ref_sd, x, ei, 2, True), y, mask)
    ref_loss.backward()
    rep = OL.compare_grads(grads, {k: ref_sd[k].grad for k in grads})
    return {"workload": wl["name"], "loss_hip": float(loss.item()), "loss_oracle": float(ref_loss.item()),
            "max_abs_grad_diff": rep["max_abs"], "max_grad_diff_over_max_1_ginf": rep["max_vs_bound"],
            "max_rel_to_gradient_scale": rep["max_rel"], "worst_parameter": rep["worst"],
            "tolerance": {"abs_over_max(1,|g|inf)": 1e-4, "relative": 2e-3}, "parameters": len(grads),
            "seconds": time.perf_counter() - t0,
            "what": "every parameter gradient of one training forward + backward (masked NLL on the G4 train split): "
                    "HIP kernels vs oracle.ref_cpu under torch autograd on the CPU"}


def appnp_full_graph_parity(model, ei, x, x_d, ei_d):
    """BASELINE config 5 as stated (APPNP K = 10, alpha = 0.1): eval-mode logits of ALL nodes of this run's trained
    APPNPStack against the same model on the CPU — dense layers in torch, the K propagates + teleport in the C
    restatement (oracle/propagate_ref.c; recurrence: reference models/pta.py:79-84). Ten hops cover the whole graph, so
    this check is on the whole graph, not on a sampled neighbourhood."""
    from oracle import ref_cpu as O
    N = x.size(0)
    K, alpha = model.conv.K, model.conv.alpha
    t0 = time.perf_counter()
    was_training = model.training
    model.eval()
    with torch.no_grad():
        got = model(x_d, ei_d)["emb"].cpu()
    model.train(was_training)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    rei, w = O.gcn_norm(ei, None, N)
    rowptr, col, perm = O.csr_from_edges(rei[1], rei[0], torch.arange(rei.size(1)), N)
    ws = w[perm.long()].contiguous()
    threads = min(O.c_threads(), host_cores())
    h = O.batch_norm(x @ sd["lin1.weight"].t() + sd["lin1.bias"], sd, "bn.", False) @ sd["lin2.weight"].t() + sd["lin2.bias"]
    z = h
    for _ in range(K):
        z = (1 - alpha) * O.propagate_c_csr(rowptr, col, ws, z, "add", threads) + alpha * h
    return {"max_abs_diff_hip_vs_cpu": (got - z).abs().max().item(), "max_abs_logit": z.abs().max().item(),
            "tolerance": 1e-4, "K": K, "alpha": alpha, "rows": N, "cpu_seconds": time.perf_counter() - t0,
            "what": f"eval-mode APPNPStack logits of all {N} nodes, K = {K}: rgbx_appnp_f32 vs {K} iterations of "
                    "oracle_propagate_csr_f32 + teleport on the CPU"}


# ---------------------------------------------------------------------------------------------------------------
# one-GPU step

def build_single_gpu(model, ei, x, y, masks, dev, loops_mode, kind, N, d):
    """One-GPU step function = the reference loop body (itexperiments.py:417-473): train forward +
    backward + Adam, then the val and test eval forwards. Returns (step, E' per propagate, algorithmic
    bytes of one aggregation launch)."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import get_graph
    model.to(dev)
    ei_d, x_d, y_d = ei.to(dev), x.to(dev), y.to(dev)
    tm, vm, sm = (m.to(dev) for m in masks)
    # torch.optim.Adam as the reference builds it (itexperiments.py:391), in its fused form: one multi-tensor launch per
    # step instead of seven. The fused step writes the parameters without moving their version counters: the package's
    # global optimizer post-hook (ops.note_weights_changed) retires what is cached per parameter state (ops.weight_t).
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=0.01, fused=True)
    torch.cuda.synchronize()
    t_ing = time.perf_counter()
    graph = get_graph(ei_d, N, loops_mode)  # graph preparation happens once per edge_index, outside the loop
    _ = graph.bwd
    if kind == "gcn":
        _ = graph.w, graph.w_t
    torch.cuda.synchronize()
    # int64 edge_index -> self-loop rewrite -> forward and transposed CSR (rgbx_csr_build: int32 radix
    # sort) -> normalisation weights, once per edge_index (the reference redoes the rewrite + gcn_norm in every conv call)
    ingest = {"csr_build_ms": (time.perf_counter() - t_ing) * 1e3,
              "what": "rgbx_csr_build forward + transposed (stable int32 radix sort of E + N slots each) + degree "
                      "normalisation + per-slot weights, wall clock with a device sync on both sides"}
    nnz_total = graph.fwd.nnz
    if kind == "gat":  # SURVEY §8d per-launch bytes, averaged over the 6 forward + 2 backward propagates
        alg = gat_alg_bytes(N, nnz_total, d)
    elif kind == "sum":  # no per-edge weight
        alg = spmm_alg_bytes(N, nnz_total, d) - 4 * nnz_total
    else:
        alg = spmm_alg_bytes(N, nnz_total, d)

    from rgb_experiment_amd.models._stack import masked_ce, masked_ce_pair
    fwd = {"x": x_d, "edge_index": ei_d}

    def evaluate(mask):
        """An eval forward reduced to what the loop reads of it: device [nll sum, count, correct] = NLLLoss on
        log_softmax(logits)[mask] + arg-max accuracy. The conv stacks take these inside the last layer's kernel (the
        logits of an eval forward are read by nobody and are not written); other models from their logits."""
        model.eval()
        with torch.no_grad():
            return masked_ce(model, fwd, y_d, mask)[1]

    def step():
        """The numbers the reference reads with .item() at three points of the loop body (itexperiments.py:437,
        467, 472) are only used after the epoch (early stopping, curves): they stay on the device and come back in
        ONE copy at the end, so the GPU queue does not drain three times per epoch."""
        model.train()
        opt.zero_grad()
        loss = masked_ce(model, fwd, y_d, tm)[0]  # = NLLLoss(log_softmax(model(x)['emb'])[mask], y[mask])
        loss.backward()
        opt.step()
        val, tst = evaluate(vm), evaluate(sm)
        s = torch.cat([loss.detach().double().reshape(1), val, tst]).tolist()  # the one host sync of the epoch
        return s[0], s[1] / s[2], s[3] / s[2], s[4] / s[5], s[6] / s[5]

    def train_only():
        """SURVEY 8d secondary number: the training step alone (forward + backward + Adam, itexperiments.py:427-440)."""
        model.train()
        opt.zero_grad()
        loss = masked_ce(model, fwd, y_d, tm)[0]
        loss.backward()
        opt.step()
        return loss.detach()  # not the loss itself: a kept autograd graph would outlive the step (and the later capture)

    def graphed():
        """The same epoch captured once as a hipGraph and replayed (rgb_experiment_amd.epoch_graph): needs a
        fresh capturable Adam; returns a run() callable."""
        from rgb_experiment_amd.epoch_graph import GraphedEpoch
        gopt = torch.optim.Adam(model.parameters(), lr=0.01, capturable=True)
        return GraphedEpoch(model, gopt, {"x": x_d, "edge_index": ei_d}, y_d, (tm, vm, sm)).capture().run

    def step_identical():
        """The same epoch's five numbers with the two result-identical shortcuts experiment() takes by default
        (share_eval_forward: val and test statistics from ONE eval forward — the reference's second eval forward,
        itexperiments.py:470, recomputes the very same outputs; cache_input_aggregate is set on the model by the caller)."""
        model.train()
        opt.zero_grad()
        loss = masked_ce(model, fwd, y_d, tm)[0]
        loss.backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            val, tst = masked_ce_pair(model, fwd, y_d, vm, sm).unbind(0)  # one forward, both statistics sets
        s = torch.cat([loss.detach().double().reshape(1), val, tst]).tolist()
        return s[0], s[1] / s[2], s[3] / s[2], s[4] / s[5], s[6] / s[5]

    def yardstick(reps=5):
        """Box-speed yardstick: the PLAIN aggregation kernel (spmm_csr_kernel, no transform, no epilogue) over the same
        forward CSR at the same width, timed with the same HIP events — a figure no fused-kernel change can move."""
        w, rs = (graph.w, None) if kind == "gcn" else (None, graph.inv_deg) if kind == "mean" else (None, None)
        sink = []
        ops.spmm_raw(graph.fwd, w, rs, x_d, kind="yardstick")
        ops.set_event_sink(sink)
        for _ in range(reps):
            ops.spmm_raw(graph.fwd, w, rs, x_d, kind="yardstick")
        ops.set_event_sink(None)
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) for _, a, b in sink)
        return {"kernel": "spmm_csr_kernel", "avg_ms": sum(t) / len(t), "min_ms": t[0], "launches": len(t),
                "what": "plain SpMM (no transform, no epilogue) over the same forward CSR, width d, same HIP-event timing"}

    step.graphed = graphed
    step.train_only = train_only
    step.identical = step_identical
    step.yardstick = yardstick
    step.ingest = ingest
    step.device_inputs = (x_d, ei_d)
    return step, nnz_total, alg


SLOW_STEPS = []  # (time_steps call #, step index, ms, median ms of the call, host-side counters): see _cgroup_cpu


def _cgroup_cpu():
    """The cgroup's CPU throttling counters (a one-GPU box grants 16 of the host's 256 CPUs; a throttled period parks every
    thread of the cgroup for up to 100 ms). Read once before and once after a timed loop, never per step: the read makes the
    kernel fold the per-CPU statistics of 256 CPUs and took 15-60 ms now and then when it sat between the steps (round 5:
    profiles/r05_host_gc_stall.txt)."""
    out = {}
    try:
        for line in open("/sys/fs/cgroup/cpu.stat"):
            k, v = line.split()
            if k in ("nr_throttled", "throttled_usec"):
                out[k] = int(v)
    except (OSError, ValueError):
        pass
    return out


def time_steps(step, steps, warmup, fence=None, tick=None, per_step=True):
    """(seconds for exactly `steps` steps between two fences, the last step's result, per-step milliseconds).
    Every step ends with its own host read of the epoch's five numbers (one copy), so the wall clock between two
    returns IS that step's duration: the per-step list costs no extra synchronisation. A step beyond 1.5 x the call's
    median is recorded in SLOW_STEPS with the full garbage collections that ran during it and the loop's cgroup throttling
    (the line's `slow_steps`)."""
    import gc
    fence = fence or torch.cuda.synchronize
    last = None
    for _ in range(warmup):
        step()
    # CPython's FULL garbage collection walks every container object of the process: 100-180 ms with torch loaded (measured:
    # profiles/r05_host_gc_stall.txt). It runs when enough NEW long-lived objects have piled up — i.e. once, some steps after
    # a leg's set-up (models, graphs, caches), and then not again in steady state (400 steps without one). Which step it
    # lands on follows the allocation count, so with other --steps / --warmup values it lands inside the timed region.
    # Collect now, and move what survives to the permanent generation: the timed steps then see only their own garbage.
    gc.collect()
    gc.freeze()
    before = _cgroup_cpu()
    fence()
    marks = [time.perf_counter()]
    full = [gc.get_stats()[2]["collections"]]
    for i in range(steps):
        last = step()
        marks.append(time.perf_counter())
        full.append(gc.get_stats()[2]["collections"])
        if tick is not None:
            tick(f"timed step {i + 1}/{steps}")
    fence()
    total = time.perf_counter() - marks[0]
    after = _cgroup_cpu()
    per = [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]
    time_steps.calls = getattr(time_steps, "calls", 0) + 1
    med = median(per)
    for i, ms in enumerate(per):
        if med and ms > 1.5 * med:
            SLOW_STEPS.append({"timed_loop": time_steps.calls, "step": i, "ms": ms, "median_ms": med,
                               "gc_full_collections": full[i + 1] - full[i],
                               "loop_throttled_periods": after.get("nr_throttled", 0) - before.get("nr_throttled", 0),
                               "loop_throttled_ms": (after.get("throttled_usec", 0) - before.get("throttled_usec", 0)) / 1e3})
    return total, last, per


DUMP_LIMIT_BYTES = 64 * 10**6  # --dump-outputs: all files together


def dump_outputs(out_dir, last, model):
    """--dump-outputs: what the last timed step handed back — the epoch's five numbers (train loss, val loss, val accuracy,
    test loss, test accuracy; float64) — and what it left in the model: parameters after the optimizer step, their
    gradients, the floating-point buffers (BatchNorm running statistics); float32. Should the arrays together exceed
    DUMP_LIMIT_BYTES, every array above an equal share of it is cut to a fixed, seeded sample of its elements (file
    `<name>.sample.npy`); with the same arguments every run writes the same names."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = [("epoch_stats", np.asarray([float(v) for v in last], dtype=np.float64))]
    grads = []
    for name, p in model.named_parameters():
        arrays.append((f"param.{name}", p.detach().float().cpu().numpy()))
        if p.grad is not None:
            grads.append((f"grad.{name}", p.grad.detach().float().cpu().numpy()))
    arrays += grads
    arrays += [(f"buffer.{name}", b.detach().float().cpu().numpy()) for name, b in model.named_buffers()
               if b.is_floating_point()]
    share = DUMP_LIMIT_BYTES // len(arrays) - 4096  # (4 KB per file for the .npy header)
    over = sum(a.nbytes for _, a in arrays) > DUMP_LIMIT_BYTES - 4096 * len(arrays)
    for name, a in arrays:
        if over and a.nbytes > share:
            keep = share // a.itemsize
            idx = torch.randperm(a.size, generator=torch.Generator().manual_seed(1234572))[:keep].sort().values.numpy()
            a, name = a.reshape(-1)[idx], f"{name}.sample"
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def median(v):
    v = sorted(v)
    n = len(v)
    return None if not n else (v[n // 2] if n % 2 else 0.5 * (v[n // 2 - 1] + v[n // 2]))


def time_graphed(step, steps, warmup):
    """ms per epoch of the hipGraph replay of the same epoch (secondary number; `value` stays on the eager
    loop, whose launches carry the per-kernel HIP events the roofline needs)."""
    try:
        run = step.graphed()
        dt, _, per = time_steps(run, steps, warmup)
        return {"ms_per_step": dt / steps * 1e3, "median_ms_per_step": median(per), "epochs_per_s": steps / dt}
    except Exception as exc:
        return {"error": repr(exc)}


def gcn_block(name, ei, x, y, dev, steps, warmup, d, note=None, replay=True, cache_input_aggregate=False,
              identical=False):
    """A 2-layer GCN epoch on another graph in the same process (secondary blocks of the line).
    `cache_input_aggregate`: the opt-in that keeps A_hat x of the static input features (4 aggregations per epoch, not
    7); `value` of that block counts the aggregations actually run."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import clear_cache
    N = x.size(0)
    torch.manual_seed(14530529)
    model = model_class("gcn")(input_dim=d, output_dim=d, **MODELS["gcn"][0])
    model.cache_input_aggregate = cache_input_aggregate
    step, nnz, alg = build_single_gpu(model, ei, x, y, split_masks(y), dev, 1, "gcn", N, d)
    ingest = step.ingest
    if identical:  # share_eval_forward as well: one eval forward per epoch
        step = step.identical
    for _ in range(warmup):
        step()
    events = []
    ops.set_event_sink(events)
    elapsed, _, per_step = time_steps(step, steps, 0)
    ops.set_event_sink(None)
    n_prop = MODELS["gcn"][1] - (3 if cache_input_aggregate else 0) - (1 if identical and cache_input_aggregate else
                                                                        2 if identical else 0)
    spmm_s = sum(s.elapsed_time(e) for k, s, e in events if k in AGG_KINDS) * 1e-3 / (n_prop * steps)
    out = {"workload": name, "edges_in": int(ei.size(1)), "edges_aggregated_per_propagate": nnz,
           "value": n_prop * nnz * steps / elapsed, "unit": "edges/s", "ms_per_step": elapsed / steps * 1e3,
           "median_ms_per_step": median(per_step), "epochs_per_s": steps / elapsed, "spmm_ms": spmm_s * 1e3,
           "roofline_frac_algorithmic": alg / spmm_s / 1e9 / HBM_PEAK_GBS,
           "aggregations_per_step": n_prop, "per_step_ms": [round(v, 3) for v in per_step], "ingest_ms": ingest}
    if replay and not identical:
        out["hip_graph_replay"] = time_graphed(step, steps, warmup)
        if "ms_per_step" in out["hip_graph_replay"]:
            # what experiment() runs up to 20 M edges (use_hip_graph=True): the block's primary figure; the eager loop's
            # (ms_per_step above) depends on the host it runs on
            out["primary_ms_per_step"] = out["hip_graph_replay"]["ms_per_step"]
            out["primary"] = "hip_graph_replay"
    if note:
        out["note"] = note
    del step, model
    clear_cache()
    torch.cuda.empty_cache()
    return out


def cora_shaped(dev, epochs=60):
    """BASELINE.json configs[0] as SURVEY §8d states it (Cora itself is not shipped): N=2708, 5278 mirrored random
    pairs, F=1433 bag-of-words rows (18 ones, row-normalised), C=7, 2-layer GCN hidden 64 — ms per epoch of the
    reference loop body, eager and replayed as a hipGraph."""
    n, pairs, f, c = 2708, 5278, 1433, 7
    gen = torch.Generator().manual_seed(1234567)
    a = torch.randint(0, n, (pairs,), generator=gen)
    b = (a + 1 + torch.randint(0, n - 1, (pairs,), generator=gen)) % n
    ei = torch.cat([torch.stack([a, b]), torch.stack([b, a])], dim=1)
    x = torch.zeros(n, f)
    x.scatter_(1, torch.randint(0, f, (n, 18), generator=gen), 1.0)
    x = x / x.sum(1, keepdim=True)
    y = torch.randint(0, c, (n,), generator=gen)
    torch.manual_seed(14530529)
    model = model_class("gcn")(input_dim=f, output_dim=c, num_layers=2, hidden_unit=64, dropout_rate=0.5)
    step, _, _ = build_single_gpu(model, ei, x, y, split_masks(y), dev, 1, "gcn", n, c)
    dt, _, _ = time_steps(step, epochs, 10)
    out = {"workload": "Cora-shaped synthetic (N=2708, E=10556, F=1433, C=7), gcn num_layers=2 hidden_unit=64",
           "eager_ms_per_epoch": dt / epochs * 1e3}
    try:
        run = step.graphed()
        dt, _, _ = time_steps(run, epochs, 10)
        out["hip_graph_ms_per_epoch"] = dt / epochs * 1e3
        out["primary_ms_per_epoch"], out["primary"] = out["hip_graph_ms_per_epoch"], "hip_graph (what experiment() runs)"
    except Exception as exc:
        out["hip_graph_error"] = repr(exc)
    from rgb_experiment_amd.graph import clear_cache
    clear_cache()
    return out


def real_shape_block(dev, ei, N, F, C, names, steps, warmup, features="dense", sparse_ok=True):
    """The epoch on the shapes the reference actually ships (initial_params.py:25-29: 2 layers, hidden 64; F > hidden > C
    with C = 7 on Cora, 40 on ogbn-arxiv — 最终结果.csv), on the graph of workload L: every layer transforms first and
    gathers at its OUTPUT width (64, then C padded to a multiple of 4), BatchNorm's column sums and the masked
    cross-entropy come out of the gather kernel (rgbx_spmm_csr_epilogue_f32). Per model: ms per reference epoch (train
    fwd + bwd + Adam + 2 eval fwd) and per identical-results epoch (one shared eval forward), the launches by kind and
    form (HIP events on the launch stream), peak HBM, and the row-gather kernels' algorithmic-byte roofline by width."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import clear_cache, get_graph
    gen = torch.Generator(device=dev).manual_seed(1234570)
    if features == "bag_of_words":  # SURVEY 8d config 1's Cora-shaped features at this size: 18 ones per row, row-normalised
        x = torch.zeros((N, F), device=dev)
        x.scatter_(1, torch.randint(0, F, (N, 18), generator=gen, device=dev), 1.0)
        x = x / x.sum(1, keepdim=True)
    else:
        x = torch.randn((N, F), generator=gen, device=dev)
    # as experiment() lays the features out: 16-byte rows; non-zeros as a CSR when they are few (ops.prepare_features)
    x = ops.prepare_features(x) if sparse_ok else ops.align_rows(x)
    y = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(1234571))
    masks = split_masks(y)
    out = {"nodes": N, "edges_in": int(ei.size(1)), "features": F, "hidden": 64, "classes": C,
           "feature_values": features, "features_multiplied_over_nonzeros": getattr(x, "_rgbx_sparse", None) is not None,
           "what": "reference default hyper-parameters (initial_params.py:25-29) on workload L's graph; features drawn on the "
                   "device: 'bag_of_words' = 18 ones per row, row-normalised (what the reference's citation datasets look "
                   "like; experiment() multiplies such features over their non-zeros), 'dense' ~ N(0, 1)", "models": {}}
    for name in names:
        torch.manual_seed(14530529)
        kwargs, n_prop, loops_mode, kind = MODELS[name]
        # initial_params.py:25-37: hidden 64 everywhere but GAT (8 heads of 8); APPNP K = 10, alpha = 0.1; SGC K = 2
        kwargs = dict(kwargs, **({"hidden_unit": 8, "heads": 8} if name == "gat" else
                                 {"hidden_dim": 64} if name == "dagnn" else {} if name == "sgc" else {"hidden_unit": 64}))
        model = model_class(name)(input_dim=F, output_dim=C, **kwargs)
        torch.cuda.reset_peak_memory_stats(dev)
        step, nnz, _ = build_single_gpu(model, ei, x, y, masks, dev, loops_mode, kind, N, C)
        rec = {}
        for label, fn in (("reference_epoch", step), ("identical_results_epoch", step.identical)):
            events = []
            ops.set_event_sink(events)  # (before the warm-up: the first step that records events pays for their creation)
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            events.clear()
            dt, last, per = time_steps(fn, steps, 0)
            ops.set_event_sink(None)
            by = {}
            for k, s, e in events:
                key = f"{k}[{k.variant}]" if getattr(k, "variant", None) is not None else str(k)
                by.setdefault(key, []).append(s.elapsed_time(e))
            table = {k: {"n_per_epoch": len(v) / steps, "avg_ms": sum(v) / len(v), "ms_per_epoch": sum(v) / steps}
                     for k, v in sorted(by.items())}
            rec[label] = {"ms_per_epoch": dt / steps * 1e3, "median_ms_per_epoch": median(per), "per_epoch_ms": per,
                          "epochs_per_s": steps / dt,
                          "timed_launches_ms_per_epoch": sum(t["ms_per_epoch"] for t in table.values()),
                          "launches": table, "final_train_loss": last[0]}
        # the row-gather kernels by width: algorithmic bytes (SURVEY 8d formula; 'mean' / 'sum' carry no per-edge weight)
        roof = {}
        for key, t in rec["reference_epoch"]["launches"].items():
            if "[rows+" not in key and "[shortrows+" not in key:
                continue
            d = int(key.split("+d")[-1].rstrip("]"))
            if key.startswith("features"):
                # the feature matrix's own non-zeros (ops.SparseRows): x W^T gathers rows of W^T [F, d] (L2-resident) into N
                # output rows, dW gathers rows of dY [N, d] into F output rows; the feature values are the per-entry weights
                sp = x._rgbx_sparse
                alg = spmm_alg_bytes(N if key.startswith("features_fwd") else F, sp.nnz, d)
            else:
                alg = spmm_alg_bytes(N, nnz, d) - (0 if key.startswith("gcn") else 4 * nnz)  # per-edge weights: A_hat only
            roof[key] = {"width": d, "algorithmic_bytes": alg, "avg_ms": t["avg_ms"],
                         "achieved_gbs": alg / (t["avg_ms"] * 1e-3) / 1e9,
                         "frac_of_8TBs": alg / (t["avg_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS}
        rec["row_gather_roofline"] = roof
        rec["hbm_allocated_peak_gb"] = torch.cuda.max_memory_allocated(dev) / 1e9
        rec["edges_aggregated_per_propagate"] = nnz
        out["models"][name] = rec
        del step, model
        clear_cache()
        torch.cuda.empty_cache()
    return out


# ---------------------------------------------------------------------------------------------------------------
# N > 1

def launch_ranks(n):
    """`python bench.py --gpus N` as typed: start N rank processes (one per GPU) with torch.distributed.run as a CHILD
    process group — exactly the command the driver would type — wait for it with a deadline, and return its exit
    status. Each rank process supervises its own worker (rgb_experiment_amd/dist/supervise.py: heartbeats, a
    deadline, fresh workers with more conservative flags when an attempt fails); rank 0's supervisor prints the JSON
    line on the inherited stdout. Called before anything in this process has touched the GPU; this process never execs
    and never makes a GPU call."""
    import socket
    import subprocess
    from rgb_experiment_amd.dist import supervise as sv
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(max(1, host_cores() // n)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    attempts = int(os.environ.get("RGBX_LAUNCH_ATTEMPTS", len(sv.ATTEMPTS)))
    # backstop only: the supervisors keep the run's budget themselves (supervise.total_budget: every attempt together at most
    # 540 s, rank 0's line — benchmark or diagnostic — out before the driver's 600 s)
    total = sv.total_budget() + 45
    import signal
    # the ranks live in their own process group: whoever ends THIS process (the driver's own timeout, Ctrl-C) must take
    # them along — by the handlers below, or, if this process is killed outright, by the parent-death signal
    proc = subprocess.Popen(cmd, env=env, start_new_session=True, preexec_fn=sv.die_with_parent(signal.SIGTERM))

    def on_signal(signum, _frame):
        sv.kill_group(proc, grace=8.0)
        sys.exit(128 + signum)

    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, on_signal)
    try:
        return proc.wait(timeout=total)
    except subprocess.TimeoutExpired:
        sv.kill_group(proc)
        print(json.dumps({"metric": "aggregated edges/sec (multi-GPU run killed by the launcher)", "value": None,
                          "unit": "edges/s", "n_gpus": n, "higher_is_better": True,
                          "error": f"the ranks did not finish within {total:g} s",
                          "launcher": {"supervised": True, "attempts_allowed": attempts}}), flush=True)
        return 1
    except KeyboardInterrupt:
        sv.kill_group(proc)
        raise


def dist_alg_bytes(dgraph, kind, d, N, n_loc, world, K=10, replica=None):
    """Algorithmic bytes PER LAUNCH of every aggregation kind this rank can record (SURVEY 8d formula on the rows /
    edges / width that launch covers)."""
    out = {}
    rst = replica._st.get(kind) if replica is not None else None
    if rst is not None:
        full = spmm_alg_bytes(N, rst["nnz_total"], d)
        tail = spmm_alg_bytes(n_loc, rst["nnz_tail"], d)
        tail_t = spmm_alg_bytes(N, rst["nnz_tail"], d)  # transposed: a row per source
        out.update({"replica_gcn_linear_fwd": full, "replica_fwd": full, "tail_gcn_linear_fwd": tail, "tail_fwd": tail,
                    "tail_gcn_linear_bwd": tail_t, "tail_gcn_bwd": tail_t, "tail_bwd": tail_t})
    st = dgraph._kinds.get(kind)
    if st is not None:
        f, b = st["plan"].fwd, st["plan"].bwd
        cnt = lambda t: 0 if t is None else int(t.numel())
        nl, nr = cnt(f.loc_agg), cnt(f.rem_agg)
        b_res = spmm_alg_bytes(n_loc, nl + nr, d)
        out.update({"dist_fwd_resident": b_res, "gcn_linear_fwd": b_res, "mean_linear_fwd": b_res,
                    "dist_fwd_local": spmm_alg_bytes(n_loc, nl, d),
                    "dist_fwd_remote": spmm_alg_bytes(n_loc, nr, d) + n_loc * 4 * d,
                    "dist_bwd_local": spmm_alg_bytes(n_loc, cnt(b.loc_agg), d),
                    "dist_bwd_remote": spmm_alg_bytes(n_loc, cnt(b.rem_agg), d) + n_loc * 4 * d})
    for key, gst in dgraph._grid.items():
        k, C, pieces = key[:3]
        src_pieces = key[4] if len(key) > 3 else 1  # fused schedule: one launch per (target piece, source piece)
        if k != kind:
            continue
        plan = gst["plan"]
        dc = d // C
        if pieces == 1 and C == world:  # the APPNP plan: K whole-graph launches at width d / P (K - 1 when the last
            # step returns in pieces: those launches are recorded as dist_*_colshard, below)
            steps = K - 1 if getattr(dgraph, "_appnp_return_pieces", 1) > 1 else K
            per = steps * (spmm_alg_bytes(N, plan.fwd.nnz, dc) + N * 4 * dc)
            out.update({"dist_fwd_appnp_colshard": per, "dist_bwd_appnp_colshard": per})
        else:
            for direction, half in (("fwd", plan.fwd), ("bwd", plan.bwd)):
                out[f"dist_{direction}_colshard"] = spmm_alg_bytes(half.n_group / pieces, half.nnz / pieces / src_pieces,
                                                                   dc)
    return out


def link_model(log, steps_logged, gbs=(50.0, 60.0, 76.8)):
    """Link arithmetic on the emulated rank's exchange log: per epoch, the bytes the busiest link carries per direction
    summed over all exchanges (`serial`: what a schedule without any overlap would wait for), and the exchanges by tag.
    How much of that the schedule HIDES is not decided by rules about tags (round 2 and the first builds of round 3
    did that) but by replaying the recorded schedule: replay_schedule."""
    tot = 0
    by_tag = {}
    for tag, b_out, b_in in log:
        b = max(b_out, b_in)
        tot += b
        t = (tag or "?")
        by_tag.setdefault(t, [0, 0])
        by_tag[t][0] += 1
        by_tag[t][1] += b
    per = lambda v: v / max(steps_logged, 1)
    return {"link_bytes_per_epoch_serial": per(tot),
            "exchanges_per_epoch": {t: {"n": c / max(steps_logged, 1), "link_bytes_each": b / c}
                                    for t, (c, b) in sorted(by_tag.items())},
            "exchange_ms_per_epoch_serial": {f"{g:g} GB/s per link and direction": per(tot) / g / 1e6 for g in gbs}}


def replay_schedule(trace, steps, gbs=(50.0, 60.0, 76.8), latency_us=0.0):
    """The emulated rank's schedule replayed against a link model. `trace` = what the instrumented steps recorded IN
    HOST ORDER: (kind, start event, end event) per timed launch, ("@issue", id, tag, bytes on the busiest link) where an
    exchange was handed to the communicator, ("@wait", id) where the compute stream was made to wait for it. Model: ONE
    compute stream runs the launches back to back in that order; the communicator's stream carries the exchanges one
    after the other (FIFO), each starting no earlier than the launches enqueued before its issue have finished and
    taking bytes / rate (+ latency); a wait holds the compute stream until its exchange has finished. What the compute
    stream stands still for is the EXPOSED exchange time — whatever schedule produced the trace (sequential evals, the
    interleaved pair, the training step computed ahead). Launches without events (BatchNorm's small kernels, optimizer)
    are not in the trace: time they would cover is counted as exposed (conservative)."""
    out = {}
    n_x = sum(1 for r in trace if r[0] == "@issue")
    durs = {}
    for g in gbs:
        t = link = busy = stall = 0.0
        done, tags, by_tag = {}, {}, {}
        for r in trace:
            if r[0] == "@issue":
                start = max(t, link)
                link = start + r[3] / (g * 1e6) + latency_us * 1e-3
                done[r[1]] = link
                tags[r[1]] = r[2]
            elif r[0] == "@wait":
                fin = done.get(r[1])
                if fin is not None and fin > t:
                    stall += fin - t
                    by_tag[tags[r[1]]] = by_tag.get(tags[r[1]], 0.0) + (fin - t) / max(steps, 1)
                    t = fin
            else:
                d = durs.get(id(r))
                if d is None:
                    d = durs[id(r)] = r[1].elapsed_time(r[2])
                t += d
                busy += d
        out[f"{g:g} GB/s per link and direction"] = {
            "exposed_ms_per_epoch": stall / max(steps, 1), "replayed_ms_per_epoch": t / max(steps, 1),
            "stalls_by_exchange_ms": {k: round(v, 4) for k, v in sorted(by_tag.items(), key=lambda kv: -kv[1])[:8]}}
    return {"what": "timed launches and exchange issue / wait points of the instrumented steps, replayed: one compute "
                    "stream, one FIFO communicator stream (bench.replay_schedule)",
            "timed_launch_ms_per_epoch": busy / max(steps, 1), "exchanges_per_epoch": n_x / max(steps, 1),
            "latency_us_per_exchange": latency_us, "by_link_rate": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="L")
    ap.add_argument("--model", choices=sorted(MODELS), default="gcn",
                    help="gcn is the BASELINE.json headline; the others are its configs 3-5")
    ap.add_argument("--exchange", default="auto",
                    help="auto | halo | reshard | RxC (row groups x column slices) | replicate (first conv layer on all "
                         "rows by every rank, no activation exchange)")
    ap.add_argument("--pieces", type=int, default=None, help="pieces of the outbound exchange (default 4)")
    ap.add_argument("--no-interleave", action="store_true", help="val and test forward one after the other")
    ap.add_argument("--task-split", choices=("auto", "on", "off"), default="auto",
                    help="N > 1: training steps on half of the ranks, eval forwards on the other half, each half with the "
                         "whole graph (dist/tasksplit.py); auto = where the slice width of N ranks falls below the 128-byte "
                         "line (APPNP stacks at N >= 4)")
    ap.add_argument("--emulate-role", choices=("train", "eval"), default="train",
                    help="--emulate-rank with task split: which group's rank 0 this process stands for")
    ap.add_argument("--no-ahead", action="store_true",
                    help="fused schedule: do NOT compute the next epoch's training forward + backward during this epoch's "
                         "eval forwards (DistRunner.epoch(more=True))")
    ap.add_argument("--no-fused", action="store_true",
                    help="N > 1: conv stacks through the modules (separate pack / GEMM / BatchNorm / loss launches) instead "
                         "of the fused per-rank schedule of rgb_experiment_amd/dist/stack.py — the conservative setting")
    ap.add_argument("--pieces-in", type=int, default=2,
                    help="fused schedule: row pieces the first layer is launched in; each piece's slices leave for their "
                         "consumers while the next piece is computed (1 = one launch, the whole inbound exchange exposed)")
    ap.add_argument("--src-split", action="store_true",
                    help="fused schedule: aggregate the sources of inbound piece k while piece k + 1 is on the links (one "
                         "CSR per source piece): less exposed exchange for more aggregation time — for slow links")
    ap.add_argument("--cache-input-aggregate", action="store_true",
                    help="SECONDARY runs only: keep the first layer's aggregate of the static input features across "
                         "forwards and epochs (experiment(cache_input_aggregate=True)); the line says so in its metric")
    ap.add_argument("--share-eval-forward", action="store_true",
                    help="N > 1 / --emulate-rank: val and test statistics from ONE eval forward per epoch (experiment()'s "
                         "default; the headline keeps the reference's two eval forwards). A SECONDARY line.")
    ap.add_argument("--plan-from-slices", action="store_true",
                    help="N > 1: every rank builds its halo / grid plans from its own 1/N of the edge list and one all-to-all "
                         "of edge records per direction (RGBX_PLAN_FROM_SLICES=1, dist/plan.py subsets_from_slices) instead of "
                         "scanning the whole list; the same plans bit for bit")
    ap.add_argument("--emulate-rank", type=int, default=0, metavar="P",
                    help="one GPU: rank 0's launches of a P-rank job, exchanges replaced by stand-in rows")
    ap.add_argument("--emulate-contend", type=float, default=60.0, metavar="GBS",
                    help="--emulate-rank: after the compute-only timing, time the same steps again with every exchange's "
                         "bytes actually MOVED on this GPU at GBS per link and direction by a paced copy on a second stream "
                         "and WAITED for (HBM / cache / CU contention and exposed exchange time inside the measured step); "
                         "0 = skip")
    ap.add_argument("--degree", choices=("uniform", "powerlaw"), default="uniform",
                    help="powerlaw: secondary run on a hub-heavy graph of the same size (row-split plans at work)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--real-shape", default=None, metavar="MODEL:F:C[:bag_of_words|dense]",
                    help="run ONLY the real-shape block (bench.real_shape_block) for one model on workload L's graph, "
                         "e.g. gcn:1433:7 — the command profiled under rocprofv3 for profiles/r05_real_shape_*")
    ap.add_argument("--primary-only", action="store_true",
                    help="with --full: skip the secondary legs (hipGraph replay, configs[0]/[1] blocks, undirected run): "
                         "clean rocprofv3 runs")
    ap.add_argument("--full", action="store_true",
                    help="one GPU: after the headline, also run every secondary leg (yardstick, parity checks, CPU baseline, "
                         "training-step-only and hipGraph timings, the other graphs, sizes and shapes of workload L). Off: "
                         "the run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (the epoch's five numbers, the "
                         "parameters, buffers and gradients of the model) as DIR/<name>.npy, float32 / float64")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # typed as `python bench.py --gpus N`: this process has made no GPU call yet; it only starts the N ranks
        # as children (one per GPU) and leaves with their status — it never replaces itself
        sys.exit(launch_ranks(args.gpus))
    if args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    from rgb_experiment_amd.dist import supervise as sv
    if world > 1 and not os.environ.get("RGBX_SUPERVISED") and os.environ.get("RGBX_NO_SUPERVISOR") != "1":
        # a rank process as torch.distributed.run (ours or the driver's) started it: it makes no GPU call, runs the
        # actual worker as a child and watches it (deadline, heartbeats, fresh workers with conservative flags on
        # failure) — so that a hang or an error in one rank ends in a JSON line, not in silence
        sys.exit(sv.supervise(os.path.abspath(__file__), sys.argv[1:], rank, world))
    t_start = time.perf_counter()
    if args.plan_from_slices:
        os.environ["RGBX_PLAN_FROM_SLICES"] = "1"
    if torch.get_num_threads() > host_cores():
        # host side of the set-up (synthetic graph, oracle legs): torch sizes its pool by the CPUs the HOST has (256 on a box
        # of the pool whose cgroup grants 16); threads beyond the quota are throttled, not run
        torch.set_num_threads(host_cores())
    sv.beat("worker started, torch imported")
    backend = os.environ.get("RGBX_DIST_BACKEND", "nccl")
    test_backend = None
    if backend == "gloo" and not torch.cuda.is_available():
        # CPU rehearsal of the N > 1 host logic (tests/test_bench_cli.py): gloo collectives and an aggregator the TEST
        # injects; the product has no CPU aggregation path of its own, so without one this is an error
        spec = os.environ.get("RGBX_TEST_AGGREGATOR")
        if world == 1 or not spec:
            sys.exit("bench.py: no MI355X visible; the only CPU mode is the gloo rehearsal of --gpus N > 1 with "
                     "RGBX_TEST_AGGREGATOR=module:Class set by a test")
        mod, cls_name = spec.split(":")
        test_backend = getattr(__import__(mod, fromlist=[cls_name]), cls_name)()
        dev = torch.device("cpu")
    else:
        local_rank %= max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    on_gpu = dev.type == "cuda"
    shared_devices = False
    if world > 1:
        # RGBX_DIST_BACKEND=gloo rehearses the N>1 code path with several ranks on ONE GPU (host-staged
        # collectives) or on the CPU (above); the real runs use RCCL ("nccl").
        if backend == "nccl":
            from rgb_experiment_amd.dist import sharing
            # two ranks on the SAME device (a one-GPU box; told from the PCI identities the ranks publish, not from counts):
            # RCCL over its socket transport, a different NCCL_HOSTID per rank (dist/sharing.py) — the product's backend and
            # code path, NOT a scaling measurement; the line says so
            shared_devices = sharing.init_rccl(dev)
        else:
            dist.init_process_group(backend)
        sv.beat("process group up")

    from rgb_experiment_amd import ops

    wl = WORKLOADS[args.workload]
    N, E, d = wl["N"], wl["E"], wl["d"]
    setup = {"imports_and_process_group_s": time.perf_counter() - t_start}
    t_mark = time.perf_counter()
    ei, x, y = synth(N, E, d, args.degree)
    sv.beat("synthetic graph drawn")
    if args.real_shape:
        name, F, C, *kind = args.real_shape.split(":")
        del x
        print(json.dumps({"real_shape": real_shape_block(dev, ei, N, int(F), int(C), [name], args.steps, args.warmup,
                                                         features=kind[0] if kind else "dense"),
                          "slow_steps": SLOW_STEPS}), flush=True)
        return
    train_mask, val_mask, test_mask = split_masks(y)
    sv.beat("masks split")
    setup["synthetic_graph_and_masks_s"] = time.perf_counter() - t_mark
    kwargs, n_prop, loops_mode, kind = MODELS[args.model]

    torch.manual_seed(14530529)  # the reference's reappear_seed (itexperiments.py:57)
    model = model_class(args.model)(input_dim=d, output_dim=d, **kwargs)
    wl_name = wl["name"].replace("2-layer GCN", {"gcn": "2-layer GCN", "graphsage": "2-layer GraphSAGE",
                                                 "graphsage2": "2-layer GraphSAGE2", "gat": "2-layer GAT 8 heads",
                                                 "appnpstack": "APPNP K=10", "sgc": "SGC K=2 (cached=False)",
                                                 "gin": "2-block GIN", "dagnn": "DAGNN K=10"}[args.model])

    if args.degree != "uniform":
        wl_name += " [SECONDARY: power-law in- and out-degree, same |V| and |E|]"
    if args.cache_input_aggregate:
        model.cache_input_aggregate = True
        n_prop -= 3 if args.model in ("gcn", "graphsage", "graphsage2") else 0  # aggregations actually run per epoch
        wl_name += " [SECONDARY: cache_input_aggregate=True, the first layer's aggregate of the static features kept]"
    emu = args.emulate_rank if world == 1 else 0
    parts = max(world, emu)  # ranks the graph is partitioned over
    if args.share_eval_forward and parts > 1:
        n_prop -= kwargs.get("K", 2) if args.model in ("appnpstack", "dagnn", "sgc") else 2  # one eval forward's propagates
        wl_name += " [SECONDARY: share_eval_forward=True, one eval forward per epoch serves the val and the test statistics]"
    comm_obj = None
    scheme, alg_by_kind, runner = "single GPU", None, None
    group = parts  # ranks ONE copy of the graph is partitioned over (task split: half of them)
    task_split = False
    if parts > 1:
        from rgb_experiment_amd.dist import DistRunner, TaskSplitRunner
        from rgb_experiment_amd.dist import tasksplit
        from rgb_experiment_amd.dist.comm import Comm, EmulatedComm
        comm_obj = EmulatedComm(emu, 0) if emu else Comm()
        t_mark = time.perf_counter()
        common = dict(lr=0.01, comm=comm_obj, backend=test_backend, exchange=args.exchange, pieces=args.pieces,
                      interleave_evals=not args.no_interleave, fused=not args.no_fused, pieces_in=args.pieces_in,
                      cache_input_aggregate=args.cache_input_aggregate, src_split=args.src_split,
                      share_eval_forward=args.share_eval_forward)
        # auto: where it pays; on two ranks (whole graph on both GPUs: no memory scaling) only when one GPU can hold it
        task_split = args.task_split == "on" or (args.task_split == "auto" and tasksplit.pays(model, parts, d) and (
            parts != 2 or bool(emu) or tasksplit.whole_graph_fits(N, E, [d], dev)))
        if task_split:
            # training steps on ranks [0, P/2), eval forwards on ranks [P/2, P), each group with the whole graph
            # (dist/tasksplit.py); an emulated run stands for rank 0 of the group --emulate-role names
            group = parts // 2
            runner = TaskSplitRunner(model, ei, x, y, (train_mask, val_mask, test_mask), 0 if emu else rank, parts, dev,
                                     role=args.emulate_role if emu else None, **common)
            comm_obj = getattr(runner.inner, "comm", comm_obj)  # the exchanges (and their log) are the group's
        else:
            runner = DistRunner(model, ei, x, y, (train_mask, val_mask, test_mask), 0 if emu else rank, parts, dev,
                                **common)
        dgraph = runner.graphs[loops_mode] if runner.graphs is not None else None  # None: a group of ONE rank
        ahead = not args.no_ahead and (task_split or (not args.no_interleave and runner.engine is not None))
        step = (lambda: runner.epoch(more=True)) if ahead else runner.epoch
        n_loc = runner.hi - runner.lo
        sv.beat("runner built (link rate measured)")
        setup["runner_and_link_probe_s"] = time.perf_counter() - t_mark
        t_mark = time.perf_counter()
        sv.test_fault("first_epoch", rank)
        step()  # builds every structure this model uses (outside the timing) ...
        if on_gpu:
            torch.cuda.synchronize()
        setup["first_epoch_plans_and_csr_build_s"] = time.perf_counter() - t_mark
        sv.beat("first epoch done: plans and CSRs built")
        runner.release_edge_list()  # ... after which the global edge list leaves HBM
        replica = runner.replicas[loops_mode] if runner.replicated else None
        if dgraph is not None:
            scheme = "replicate" if replica is not None else (dgraph.scheme(d) if kind != "gat" else "halo")
        if dgraph is None:  # task split over 2 ranks: each rank holds the whole graph and runs the single-GPU kernels
            from rgb_experiment_amd.graph import get_graph
            scheme = "whole graph per rank (no partition, no exchange)"
            nnz_total = get_graph(runner.inner.fwd["edge_index"], N, loops_mode).fwd.nnz
            alg = gat_alg_bytes(N, nnz_total, d) if kind == "gat" else spmm_alg_bytes(N, nnz_total, d) - (
                4 * nnz_total if kind == "sum" else 0)
        elif replica is not None:
            nnz_total = replica._st[kind]["nnz_total"]
            alg_by_kind = dist_alg_bytes(dgraph, kind, d, N, n_loc, group, K=kwargs.get("K", 10), replica=replica)
            alg = spmm_alg_bytes(n_loc, nnz_total / group, d)  # an ideal 1/P share of one propagate
        elif kind == "gat":
            plan = dgraph._kinds["gat"]["plan"]
            nnz_total = plan.nnz_total
            alg = gat_alg_bytes(n_loc, plan.nnz_local, d)
        else:
            plans = [st["plan"] for st in list(dgraph._kinds.values()) + list(dgraph._grid.values())]
            nnz_total = plans[0].nnz_total
            alg_by_kind = dist_alg_bytes(dgraph, kind, d, N, n_loc, group, K=kwargs.get("K", 10))
            alg = spmm_alg_bytes(n_loc, nnz_total / group, d)  # an ideal 1/P share of one propagate
    else:
        step, nnz_total, alg = build_single_gpu(model, ei, x, y, (train_mask, val_mask, test_mask), dev, loops_mode,
                                                kind, N, d)

    def fence():
        if world > 1:
            dist.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    tick = sv.Ticker()
    for i in range(args.warmup):
        step()
        tick(f"warm-up step {i + 1}/{args.warmup}")
    sv.test_fault("timed_region", rank)
    events = []
    # Per-launch HIP events (two event records around every aggregation launch and every exchange wait) separate
    # consecutive kernels by a few microseconds each. One GPU: 7 fused launches per epoch, every step is instrumented.
    # A partitioned rank makes ~40 such launches of 0.15 ms per epoch: there every third step carries events, and the
    # per-launch averages come from those steps (same launches in every step).
    every = 3 if parts > 1 else 1
    timed_steps_with_events = len(range(0, args.steps, every))
    timed_step = step
    if on_gpu:
        calls = [0]

        def timed_step():
            ops.set_event_sink(events if calls[0] % every == 0 else None)
            calls[0] += 1
            return step()
    if comm_obj is not None:
        comm_obj.bytes_sent, comm_obj.exchanges = 0, 0
        runner.host_enqueue_s = 0.0
        if emu:
            comm_obj.log.clear()
    elapsed, last, step_ms = time_steps(timed_step, args.steps, 0, fence, tick=tick)
    ops.set_event_sink(None)
    sv.beat("timed region done")
    if world > 1 and not all(v == v and abs(v) != float("inf") for v in last):
        # numbers that are not finite after real exchanges mean the run is wrong, not slow: fail, so that the
        # supervisors start the next, more conservative attempt instead of relaying this line
        raise RuntimeError(f"bench.py: non-finite results after the timed region: {last}")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    hbm_peak_gb = torch.cuda.max_memory_allocated(dev) / 1e9 if on_gpu else None  # structures + one epoch's tensors
    if args.dump_outputs and rank == 0:
        # before any secondary leg (--full) moves the weights further
        dump_outputs(args.dump_outputs, last, getattr(runner, "model", model))
    trace, events = events, [r for r in events if not r[0].startswith("@")]  # "@issue" / "@wait": the emulated comm's marks
    by_kind, by_variant = {}, {}
    for k, s, e in events:
        ms = s.elapsed_time(e)
        by_kind.setdefault(str(k), []).append(ms)
        if getattr(k, "variant", None) is not None:  # which form of the fused launch (ops.Kind)
            by_variant.setdefault(f"{k}[{k.variant}]", []).append(ms)
    agg_total_ms = sum(sum(v) for k, v in by_kind.items() if k in AGG_KINDS)
    agg_total_ms *= args.steps / timed_steps_with_events  # scaled from the instrumented steps to all of them
    agg_avg_s = agg_total_ms * 1e-3 / (n_prop * args.steps)  # aggregation kernel time per propagate (this rank)
    dominant = max((k for k in by_kind if k in AGG_KINDS), key=lambda k: sum(by_kind[k]), default=None)
    kernel = KERNEL_OF_KIND.get(dominant, "none recorded")
    achieved, roofline_launches = None, None
    if alg_by_kind and agg_total_ms:  # partitioned run: launches of different shapes, sum bytes over those made
        done = sum(alg_by_kind[k] * len(v) for k, v in by_kind.items() if k in alg_by_kind)
        achieved = done / (agg_total_ms * timed_steps_with_events / args.steps * 1e-3) / 1e9
    elif dominant is not None:
        # the DOMINANT kernel's own launches: its algorithmic bytes per launch / its mean launch duration
        launches_per_event = kwargs.get("K", 1) if dominant.startswith("appnp") else 1
        if dominant == "gat_fwd":  # the forward launches alone (gat_fwd_launch_bytes), inference and training form
            whole = parts == 1 or dgraph is None
            rows_here, nnz_here = (N, nnz_total) if whole else (n_loc, plan.nnz_local)
            alg = gat_fwd_launch_bytes(rows_here, nnz_here, d, kwargs.get("heads", 8))
            if not whole:  # partitioned GAT runs every layer on the halo scheme's own kernels
                l1, l2 = gat_launch_bytes(rows_here, nnz_here, kwargs.get("heads", 8), d // kwargs.get("heads", 8)), \
                    gat_launch_bytes(rows_here, nnz_here, 1, d)
                alg = sum(2 * l["fwd_infer"] + l["fwd_train"] for l in (l1, l2)) / 6
        elif dominant == "gat_linear_fwd":
            lin = gat_linear_launch_bytes(N, nnz_total, d)
            alg = (2 * lin["fwd_infer"] + lin["fwd_train"]) / 3
        # ONE convention for the dominant kernel's launch duration: the mean over EVERY launch of that kernel in the
        # timed region (forward forms and the transposed launch alike: same kernel, same algorithmic bytes per launch),
        # which for the conv stacks is what `spmm_ms` reports too
        same_kernel = [k for k in by_kind if KERNEL_OF_KIND.get(k) == KERNEL_OF_KIND.get(dominant)
                       and not dominant.startswith("gat")] or [dominant]
        pooled = [v for k in same_kernel for v in by_kind[k]]
        dom_s = sum(pooled) / len(pooled) / launches_per_event * 1e-3
        achieved = alg / dom_s / 1e9
        roofline_launches = {"kinds": sorted(same_kernel), "launches_averaged": len(pooled)}
    stat = lambda v: {"n": len(v), "avg_ms": sum(v) / len(v), "min_ms": min(v), "max_ms": max(v)}
    by_kind = {k: {"n": len(v), "avg_ms": sum(v) / len(v)} for k, v in sorted(by_kind.items())}
    by_variant = {k: stat(v) for k, v in sorted(by_variant.items())}
    traffic, traffic_note = pmc_traffic(args.workload, args.model, kernel, parts)
    if args.degree != "uniform":
        traffic, traffic_note = None, "the committed PMC passes were taken on the uniform graph"

    result = {
        "metric": "aggregated edges/sec (full-graph GCN d=128, reference epoch = train fwd+bwd+Adam + 2 eval fwd)"
                  if args.model == "gcn" else f"aggregated edges/sec (full-graph {args.model} d=128, reference epoch)",
        "value": n_prop * nnz_total * args.steps / elapsed,
        "unit": "edges/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        # median of the per-step times beside the mean (`value` and ms_per_step stay the contract's
        # total-time figures); a step ends with its own host read, so these cost no extra synchronisation
        "median_ms_per_step": median(step_ms),
        "min_ms_per_step": min(step_ms) if step_ms else None,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": wl_name, "nodes": N, "edges_in": E, "edges_aggregated_per_propagate": nnz_total,
                   "width": d, "propagates_per_step": n_prop,
                   "parallelism": "single GPU" if parts == 1 else
                   (f"epoch split by task over 2 groups of {group} rank(s): training steps (the next one computed ahead) "
                    f"on one group, val and test forwards on the other; within a group: {scheme}") if task_split else
                   ("1-D node partition x%d, replicate scheme: first conv layer on all rows by every rank, second on "
                    "its own targets, no activation exchange (RCCL all-reduces of loss / gradients only)" % parts)
                   if scheme == "replicate" else
                   f"1-D node partition x{parts}, RCCL all-to-all ({scheme} exchange; boundary rows of the static "
                   "input features resident in HBM)",
                   "plans_from_edge_list_slices": bool(args.plan_from_slices and parts > 1)},
        "epochs_per_s": args.steps / elapsed,
        "spmm_edges_per_s": nnz_total / agg_avg_s if parts == 1 and agg_avg_s else None,
        "spmm_ms": agg_avg_s * 1e3,
        "kernel_ms_by_kind": by_kind,
        # the fused kernel's launches by FORM (template instantiation + what the launch also writes): z = the aggregate
        # is stored for the weight gradient (+ N d 4 bytes), stats = BatchNorm column sums, pre = BatchNorm applied to
        # the aggregate, ce_stats = loss statistics only (no output write), ce_grad = loss gradient written
        "kernel_ms_by_variant": by_variant,
        "final_losses": {"train": last[0], "val": last[1], "test": last[3]},
        "hbm_allocated_peak_gb": hbm_peak_gb,
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS if achieved else None,
                     "traffic": traffic, "traffic_source": traffic_note,
                     "kernel": kernel, "kernel_source_hash": kernel_source_hash(kernel),
                     "algorithmic_bytes_per_launch": alg, "duration_over": roofline_launches,
                     "compulsory_bytes_per_launch": spmm_compulsory_bytes(N if parts == 1 else n_loc,
                                                                          nnz_total / group, d),
                     "note": ("an ideal 1/P share of one propagate" if parts > 1 and dgraph is not None
                              else "whole graph, one propagate")
                     + "; `achieved` = ALGORITHMIC bytes (SURVEY 8d formula, every gathered row counted once per edge) / "
                     "mean launch duration, `frac` = that over the 8 TB/s spec peak. It is not an HBM-pin fraction: "
                     "FETCH_SIZE counts at the L2's fabric side, and about a quarter of the gathered rows of a 1 GB "
                     "table are served by the 256 MiB Infinity Cache (at workload S all of them)"},
    }
    if parts > 1:
        mine = {"rank": rank, "scheme": scheme, "fused_schedule": runner.engine is not None,
                "exchange_mb_per_step": comm_obj.bytes_sent / args.steps / 1e6,
                "exchanges_per_step": comm_obj.exchanges / args.steps, "aggregation_ms_per_step": agg_total_ms / args.steps,
                # time the compute streams stood still in exchange waits (HIP events around every work.wait()): the
                # exposed part of the exchanges, measured; RCCL runs only
                "exposed_exchange_ms_per_step": (by_kind.get("exchange_wait", {"n": 0, "avg_ms": 0.0})["n"]
                                                 * by_kind.get("exchange_wait", {"n": 0, "avg_ms": 0.0})["avg_ms"]
                                                 / timed_steps_with_events),
                "rows": n_loc, "device": str(dev),
                # host time to enqueue one epoch's launches and exchanges (before the read-back that waits for the GPU)
                "host_enqueue_ms_per_step": runner.host_enqueue_s / args.steps * 1e3,
                # where this rank's time went BEFORE the timed region (seconds): the partition plans are index arithmetic
                # over the global edge list on every rank, the CSRs come from rgbx_csr_build
                "setup_s": {k: round(v, 3) for k, v in setup.items()}}
        per_rank = [mine]
        if world > 1:
            per_rank = [None] * world
            dist.all_gather_object(per_rank, mine)
        result["ranks_seen"] = len(per_rank)
        result["scheme"] = scheme
        result["fused_schedule"] = runner.engine is not None
        result["next_step_ahead"] = ahead
        result["task_split"] = ({"groups": 2, "ranks_per_group": group, "role_of_rank_0": runner.role,
                                 "what": "ranks [0, P/2) run the training steps (the next one computed ahead while) ranks "
                                         "[P/2, P) run the val and test forwards; each group holds the whole graph"}
                                if task_split else None)
        result["interleaved_evals"] = {"on": runner.interleave_evals, "decision": runner.interleave_decision}
        result["per_rank"] = per_rank
        result["exchange_mb_per_rank_per_step"] = max(r["exchange_mb_per_step"] for r in per_rank)
        result["modelled_seconds_per_propagate"] = None if dgraph is None else (dgraph._choice.get(("costs", d)) or next(
            (v for k, v in dgraph._choice.items() if isinstance(k, tuple) and k[0] == "costs"), None))
        result["modelled_seconds_per_epoch_first_two_layers"] = getattr(runner, "replicate_costs", None)
        result["link_gbs_measured"] = getattr(comm_obj, "link_gbs", None)  # 16 MB-per-peer all-to-all at start-up
        result["small_all_to_all_us_measured"] = getattr(comm_obj, "link_latency_us", None)  # one row per peer
    if shared_devices:
        result["ranks_share_devices"] = {
            "ranks": world, "visible_gpus": torch.cuda.device_count(),
            "what": "RCCL with a different NCCL_HOSTID per rank (rgb_experiment_amd/dist/sharing.py): the ranks time-slice the "
                    "visible GPU(s) and exchange through RCCL's socket transport on the loopback interface — the product's "
                    "backend and code path end to end, NOT a scaling measurement; `value` says nothing about N GPUs"}
        result["metric"] = f"REHEARSAL ({world} ranks on {torch.cuda.device_count()} GPU), not a benchmark value: " + result["metric"]
    if emu:
        result["n_gpus"] = 1
        result["emulated"] = {"rank": 0, "of": emu, "scheme": scheme,
                              "what": "rank 0's structures and kernel launches of the partitioned job on one GPU; every "
                                      "exchange delivers stand-in rows, so ms_per_step is the rank's COMPUTE per epoch and "
                                      "`value` is what the job would reach if the exchanges were free",
                              **link_model(comm_obj.log, args.steps)}
        if on_gpu:
            result["emulated"]["schedule_replay"] = replay_schedule(trace, timed_steps_with_events)
            result["emulated"]["schedule_replay_30us_per_exchange"] = replay_schedule(
                trace, timed_steps_with_events, latency_us=30.0)["by_link_rate"]
            result["emulated"]["next_step_ahead"] = ahead
        result["metric"] = "EMULATED rank compute, not a benchmark value: " + result["metric"]
        if on_gpu and args.emulate_contend > 0:
            def contended_leg(nontemporal=False, sync_only=False):
                # the PESSIMISTIC one-GPU figure (round 4): the same steps with the exchanges' bytes moved on this GPU at
                # the assumed link rate x (P - 1) peers while the rank computes, and waited for where the schedule
                # depends on them — what the step costs including exposed exchange time and the contention for HBM,
                # caches and CUs that bench.replay_schedule's link model leaves out
                cal = comm_obj.enable_contention(dev, args.emulate_contend, nontemporal=nontemporal, sync_only=sync_only)
                warm = []
                for i in range(4):  # (the first instrumented step under contention pays one-off event / stream set-up)
                    ops.set_event_sink(warm if i == 0 else None)
                    step()
                ops.set_event_sink(None)
                del warm
                ev = []
                calls2 = [0]

                def step2():
                    ops.set_event_sink(ev if calls2[0] % every == 0 else None)
                    calls2[0] += 1
                    return step()
                dt, _, per = time_steps(step2, args.steps, 0, fence)
                ops.set_event_sink(None)
                waits = [a.elapsed_time(b) for k, a, b in [r for r in ev if not r[0].startswith("@")] if k == "exchange_wait"]
                n_ev = len(range(0, args.steps, every))
                free_ms = elapsed / args.steps * 1e3
                return {"assumed_link_gbs_per_direction": args.emulate_contend, "paced_copy": cal,
                        "ms_per_step": dt / args.steps * 1e3, "median_ms_per_step": median(per),
                        "per_step_ms": [round(v, 3) for v in per], "compute_only_ms_per_step": free_ms,
                        "compute_only_median_ms_per_step": median(step_ms),
                        "exposed_exchange_wait_ms_per_step": sum(waits) / max(n_ev, 1),
                        "contention_and_exposure_over_compute": median(per) / median(step_ms),
                        "value_edges_per_s_with_exchanges": n_prop * nnz_total / (median(per) * 1e-3),
                        "what": "rank 0's epoch with every exchange's bytes copied device-to-device on a second stream at "
                                "the assumed link rate x (P - 1) while the compute stream runs, consumers waiting for the "
                                "copy: compute + exposed exchange + contention, measured on ONE GPU; no RCCL, no real link"}
            for key, nt, so in (("contended", False, False), ("contended_cache_bypassing_traffic", True, False),
                                ("contended_control_sync_only", False, True)):
                # plain loads / stores (allocating in L2 / Infinity Cache: pessimistic), non-temporal ones (optimistic), and
                # a CONTROL that keeps every stream hand-over and launch of the emulation but moves 4 KB per exchange: what
                # of the slowdown is cross-stream synchronisation rather than traffic
                try:
                    result["emulated"][key] = contended_leg(nt, so)
                except Exception as exc:  # noqa: BLE001
                    result["emulated"][key] = {"error": repr(exc)}
                    torch.cuda.synchronize()

    def secondary(key, fn):
        """A leg after the timed region must never cost the line its headline: its failure is recorded under its key
        (a checker that throws is a finding to read on the line, not a reason to print nothing)."""
        try:
            result[key] = fn()
        except Exception as exc:  # noqa: BLE001
            result[key] = {"error": repr(exc)}
            if on_gpu:
                torch.cuda.synchronize()

    if parts == 1 and on_gpu:
        result["ingest_ms"] = step.ingest

        def yardstick_leg():
            y = step.yardstick()
            if y["avg_ms"] > 0:  # every form of the fused launch relative to the plain SpMM of the same box and run
                y["launch_over_yardstick"] = {k: v["avg_ms"] / y["avg_ms"] for k, v in
                                              {**by_kind, **by_variant}.items()
                                              if KERNEL_OF_KIND.get(k.split("[")[0]) == "spmm_linear_kernel"}
            return y
        if kind in ("gcn", "mean", "sum") and args.full:
            secondary("yardstick", yardstick_leg)

    if rank == 0 and parts == 1 and on_gpu and args.full and not args.no_cpu_baseline:
        x_d, ei_d = step.device_inputs

        def fused_output():
            if args.model != "gcn":
                return None
            # the kernel the timed region launches, on the whole workload, model's first layer
            from rgb_experiment_amd.graph import get_graph
            conv = model.convs[0]
            with torch.no_grad():
                out = ops.propagate_linear(x_d, get_graph(ei_d, N, 1), "gcn", conv.lin.weight, conv.bias).cpu()
            return out, conv.lin.weight.detach().cpu(), conv.bias.detach().cpu()

        secondary("parity", lambda: {"sampled_logits": sampled_logit_parity(args.model, model, ei, x, x_d, ei_d)})
        if args.model == "appnpstack":
            secondary("parity_k10_whole_graph", lambda: appnp_full_graph_parity(model, ei, x, x_d, ei_d))
        secondary("cpu_baseline", lambda: cpu_baseline(ei, x, N, fused=fused_output()))
        if args.model == "gcn" and args.workload in ("L", "S") and not args.primary_only:
            secondary("parity_gradients_at_S", lambda: gradient_parity_S(dev))

    if parts == 1 and on_gpu and args.full and not args.primary_only:
        # SURVEY 8d secondary: the training step without the two eval forwards (after the headline: it moves the
        # weights further, which the timed epochs above must not see)
        def train_only_leg():
            t_train, _, _ = time_steps(step.train_only, args.steps, 1)
            return {"ms_per_step": t_train / args.steps * 1e3, "steps_per_s": args.steps / t_train,
                    "what": "train forward + backward + Adam, no eval forwards (itexperiments.py:427-440)"}
        secondary("train_step_only", train_only_leg)
        secondary("hip_graph_replay", lambda: time_graphed(step, args.steps, args.warmup))
    if parts == 1 and on_gpu and args.full and args.workload == "L" and args.model == "gcn" and not args.primary_only:
        del step, model
        from rgb_experiment_amd.graph import clear_cache
        from rgb_experiment_amd.utils import to_undirected
        clear_cache()
        torch.cuda.empty_cache()

        def undirected_leg():
            # SURVEY 8d secondary run: the mirrored / coalesced variant of the same graph (itexperiments.py:235-238)
            ei_dev = ei.to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ei_u = to_undirected(ei_dev, N)  # rgbx_coalesce_keys_i64 (mirror, 64-bit radix sort, unique) + split
            torch.cuda.synchronize()
            t_und = (time.perf_counter() - t0) * 1e3
            ei_u = ei_u.cpu()
            del ei_dev
            out = gcn_block(wl["name"] + ", to_undirected", ei_u, x, y, dev, args.steps, args.warmup, d, replay=False)
            out["ingest_ms"] = dict(out["ingest_ms"], to_undirected_ms=t_und, edges_out=int(ei_u.size(1)))
            return out

        def configs_1_leg():
            s = WORKLOADS["S"]
            ei_s, x_s, y_s = synth(s["N"], s["E"], s["d"])
            return gcn_block(s["name"], ei_s, x_s, y_s, dev, args.steps, args.warmup, s["d"],
                             note="X fits the Infinity Cache at this size: the fraction is cache-served, not HBM")

        def powerlaw_leg():
            # hub-heavy graph of the same |V| and |E| (Zipf-like in- and out-popularity): the row-split plans at work
            ei_p, _, _ = synth(N, E, 4, "powerlaw")
            return gcn_block(wl["name"] + ", power-law in- and out-degree", ei_p, x, y, dev, args.steps, args.warmup, d,
                             replay=False)

        def cached_leg():
            # OPT-IN, never the headline: A_hat x of the static input features kept across forwards and epochs
            # (experiment(cache_input_aggregate=True)): 4 aggregations per epoch instead of 7
            out = gcn_block(wl["name"] + ", cache_input_aggregate=True", ei, x, y, dev, args.steps, args.warmup, d,
                            replay=False, cache_input_aggregate=True)
            out["note"] = ("opt-in secondary number: the first layer's aggregate of the static features is formed once, "
                           "an epoch then runs 4 aggregations (value counts 4 E' per step); the headline recomputes it "
                           "in all three forwards as the reference does")
            return out

        def identical_leg():
            # what experiment() runs BY DEFAULT (round 4): the two shortcuts whose results are bit-identical to the
            # reference-shaped epoch (tests test_shared_eval_forward_changes_nothing_but_the_forward_count,
            # test_cached_input_aggregate_changes_nothing_but_the_aggregation_count): A_hat x of the static features kept,
            # val and test statistics from one eval forward — 3 aggregations per epoch instead of 7. `value` of the line
            # stays on the reference-equivalent 7-propagate epoch.
            out = gcn_block(wl["name"] + ", cache_input_aggregate + share_eval_forward (experiment() defaults)", ei, x, y,
                            dev, args.steps, args.warmup, d, replay=False, cache_input_aggregate=True, identical=True)
            out["note"] = ("same five numbers per epoch as the headline's epoch, bit for bit; 3 aggregations per epoch "
                           "(training layer 2, its transposed backward, the one eval forward's layer 2)")
            return out

        def real_shape_leg():
            # the reference's own shapes (in > out, small odd class counts): never the fused aggregate+transform kernel
            names = ("gcn", "graphsage", "graphsage2")
            k = max(3, args.steps // 2)
            return {"F1433_C7_bag_of_words": real_shape_block(dev, ei, N, 1433, 7, names, k, 2, "bag_of_words"),
                    "F1433_C7_dense": real_shape_block(dev, ei, N, 1433, 7, ("gcn",), k, 2, "dense"),
                    "F128_C40_dense": real_shape_block(dev, ei, N, 128, 40, names, k, 2, "dense")}

        secondary("identical_results_same_run", identical_leg)
        if isinstance(result.get("identical_results_same_run"), dict) and "epochs_per_s" in result["identical_results_same_run"]:
            result["epochs_per_s_identical_results"] = result["identical_results_same_run"]["epochs_per_s"]
        secondary("cached_input_aggregate_same_run", cached_leg)
        secondary("undirected_same_run", undirected_leg)
        secondary("powerlaw_same_run", powerlaw_leg)
        secondary("configs_1_same_run", configs_1_leg)
        secondary("configs_0_same_run", lambda: cora_shaped(dev))
        secondary("real_shape_same_run", real_shape_leg)
    # steps beyond 1.5 x their loop's median, in any timed loop of this run (loop 1 = the headline's), with the full garbage
    # collections during the step and the loop's cgroup throttling: what can hold the HOST thread
    result["slow_steps"] = SLOW_STEPS
    if rank == 0:
        print(json.dumps(result), flush=True)
    # from here on only the teardown is left: a supervisor that has to end this worker later (a process group that does
    # not come down) still counts the run — the line is out
    sv.beat("done")
    sv.test_fault("teardown", rank)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
