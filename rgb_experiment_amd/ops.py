"""Autograd wrappers around the HIP aggregation kernels (C ABI: include/rgbx_hip.h).

Each Function is one ``MessagePassing.propagate`` of the reference: forward runs on the
target-grouped CSR, backward runs the SAME kernel on the source-grouped (transposed) CSR, so no
[E', d] tensor is ever materialised (cf. the gather -> multiply -> scatter temporaries of the
PyG path the reference uses, models/gcn.py:27).
"""
import ctypes

import torch

from . import _lib

# Optional per-launch timing hook used by bench.py: when set to a list, every aggregation launch
# appends (kind, start_event, end_event) recorded on the launch stream.
_EVENT_SINK = None


def set_event_sink(sink):
    global _EVENT_SINK
    _EVENT_SINK = sink


class Kind(str):
    """Event kind that also says WHICH FORM of the launch it was (`variant`: the epilogues / extra outputs that select
    the kernel's template instantiation and add to its bytes); equal to, and hashed as, the plain kind string."""
    variant = None


class _Timed:
    def __init__(self, kind, variant=None):
        if variant is not None and _EVENT_SINK is not None:
            kind = Kind(kind)
            kind.variant = variant
        self.kind = kind

    def __enter__(self):
        if _EVENT_SINK is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if _EVENT_SINK is not None:
            self.e.record()
            _EVENT_SINK.append((self.kind, self.s, self.e))
        return False


def _launch(kind, name, *args, variant=None):
    """Launch the entry point `name` on the current stream inside a `_Timed(kind, variant)` bracket (_lib.launch): the
    arguments are marshalled BEFORE the bracket opens, so its start event sits directly in front of the launch, and the
    return code is checked after it has closed. Without an event sink the bracket would do nothing and is not made."""
    _lib.launch(name, *args, bracket=None if _EVENT_SINK is None else _Timed(kind, variant))


def spmm_raw(csr, w, rs, x, y=None, a=1.0, b=0.0, out=None, kind="spmm", bias=None):
    """out[i] = a*rs[i]*sum_p w[p]*x[col[p]] + b*y[i] + bias over `csr` (no autograd)."""
    _lib.require_device(x, y, bias)
    x = x if x.stride(-1) == 1 else x.contiguous()
    xm = _lib.mat(x, "x")
    N, d = csr.N, x.size(1)
    if out is None:
        out = torch.empty((N, d), dtype=torch.float32, device=x.device)
    split, _scratch = csr.split_arg(d, x.device)
    _launch(kind, "rgbx_spmm_csr_f32", csr.rowptr, csr.col, w, rs, xm, _lib.mat_opt(y, "y"), bias,
            _lib.mat(out, "out"), N, d, float(a), float(b), split,
            variant=f"rows+d{d}" if _EVENT_SINK is not None else None)
    return out


class _PropagateGCN(torch.autograd.Function):
    """A_hat x with A_hat = D^-1/2 (A + I) D^-1/2 (dagnn.py:12-31, message dagnn.py:57-59)."""

    @staticmethod
    def forward(ctx, x, graph, bias):
        ctx.graph, ctx.has_bias = graph, bias is not None
        b = None if bias is None else bias.detach().contiguous()
        return spmm_raw(graph.fwd, graph.w, None, x, kind="gcn_fwd", bias=b)

    @staticmethod
    def backward(ctx, gy):
        g = ctx.graph
        gy = gy.contiguous()
        gb = gy.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        gx = spmm_raw(g.bwd, g.w_t, None, gy, kind="gcn_bwd") if ctx.needs_input_grad[0] else None
        return gx, None, gb


class _PropagateMean(torch.autograd.Function):
    """mean_{j in N(i)} x_j with sum/max(count,1) (aggr='mean', graphsage.py:39,58)."""

    @staticmethod
    def forward(ctx, x, graph):
        ctx.graph = graph
        return spmm_raw(graph.fwd, None, graph.inv_deg, x, kind="mean_fwd")

    @staticmethod
    def backward(ctx, gy):
        g = ctx.graph
        return spmm_raw(g.bwd, g.w_mean_t, None, gy.contiguous(), kind="mean_bwd"), None


class _PropagateSum(torch.autograd.Function):
    """Unweighted sum over incoming edges (aggr='add', no norm)."""

    @staticmethod
    def forward(ctx, x, graph):
        ctx.graph = graph
        return spmm_raw(graph.fwd, None, None, x, kind="sum_fwd")

    @staticmethod
    def backward(ctx, gy):
        return spmm_raw(ctx.graph.bwd, None, None, gy.contiguous(), kind="sum_bwd"), None


def _is_dist(graph):
    return getattr(graph, "is_distributed", False)


def target_rows(x, graph):
    """The rows of `x` that are aggregation TARGETS of `graph`: all of them, except on a partitioned run's
    rectangular second stage (dist.ReplicaGraph: sources = all N replicated rows, targets = this rank's)."""
    fn = getattr(graph, "target_rows", None)
    return x if fn is None else fn(x)


def align_rows(x):
    """`x` ([N, F] float32 on the device) as a view whose ROWS start on 16-byte boundaries: F % 4 != 0 (Cora's 1433) ->
    a fresh [N, F4] buffer (F4 = F rounded up to 4, pad columns zero) viewed as [:, :F]. Same values, same shape; dense
    products over it read whole float4s (rgbx_gemm_tn_f32's aligned-row path, hipBLASLt with lda = F4) and _pad4 finds the
    padded matrix already there. Costs one copy, once per feature matrix (the reference moves / normalises the features
    once as well, itexperiments.py:258-299); returns `x` itself where nothing is to do."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.size(1) % 4 == 0:
        return x
    n, f = x.shape
    base = torch.zeros((n, (f + 3) // 4 * 4), dtype=torch.float32, device=x.device)
    view = base[:, :f]
    view.copy_(x)
    view._rgbx_base = base  # (this Python object only: views of it are ordinary strided tensors)
    return view


def _aligned_rows(t):
    """`t` itself when its rows sit on 16-byte boundaries (or nothing would be gained), else align_rows' padded copy."""
    if t.dim() != 2 or t.dtype != torch.float32 or t.size(1) % 4 == 0 or (t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0):
        return t
    return align_rows(t)


def _rows_padded_readable(t):
    """A [K, n] matrix whose 16-byte-aligned rows may be read up to the next multiple of 4 columns (rgbx_gemm_tn_f32's
    contract): contiguous rows, stride % 4 == 0, and the storage holds the last row's padding too."""
    if t.dim() != 2 or t.size(1) % 4 == 0 or t.stride(0) % 4 or t.data_ptr() % 16:
        return True  # nothing is read beyond the columns (or the rows are unaligned: the 4-byte path)
    last = t.storage_offset() + (t.size(0) - 1) * t.stride(0) + (t.size(1) + 3) // 4 * 4
    return last * 4 <= t.untyped_storage().nbytes()


def _rows_on_grid(t, vec=4):
    """`t` ([N, F] float32) as a matrix whose rows a kernel may read `vec` floats at a time: unit column stride, the first
    element on a 4 * vec byte boundary and, above one row, a leading dimension that is a multiple of vec. A view that
    meets this (a column block of a wider matrix, say) is handed on as it is; anything else is copied once into a fresh
    allocation. .contiguous() alone does not do: a contiguous view that starts in the middle of an allocation (a one-row
    block, a slice of a flat buffer) comes back unchanged, misaligned pointer included."""
    ok = (t.dim() == 2 and (t.size(1) <= 1 or t.stride(1) == 1) and t.data_ptr() % (4 * vec) == 0
          and (t.size(0) <= 1 or (t.stride(0) % vec == 0 and t.stride(0) >= t.size(1))))
    return t if ok else t.clone(memory_format=torch.contiguous_format)


def _head_vec(C):
    """The narrowest vector width at which the 64 lanes of a wave still cover one head of C channels (attn_common.h:
    pick_vec lowers the width to what the operands' pointers and leading dimensions allow, and make_layout refuses a
    head that would then need more than 64 lanes)."""
    return 1 if C <= 64 else (2 if C <= 128 else 4)


def _width_vec(C):
    """The widest vector (4, 2 or 1 floats) that divides a width of C channels."""
    return 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)


def _vec_on_grid(t, n):
    """A parameter (attention vector, bias) as n contiguous floats on a 16-byte boundary, detached; None stays None. The
    kernels read these `vec` floats at a time too, and pick_vec counts their pointers: a contiguous slice of a flat
    parameter buffer keeps its pointer through .contiguous()."""
    if t is None:
        return None
    t = t.detach().reshape(n).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _pad4(x):
    """Feature widths that are no multiple of 4 (C = 7 classes on Cora, 41 on Reddit, 47 on ogbn-products) run on
    zero-padded rows: 16-byte aligned rows take the float4 gather path and straddle fewer 128-byte lines. Measured at
    |V| = 2M, |E| = 60M: d = 7 1.22 ms vs 8 1.08 ms, 41 2.46 vs 44/48 2.21, 47 2.64 vs 48 2.21 (profiles/
    r02_narrow_width_ms.txt); the pad copy is N x d floats against E' x d gathered. Returns (x or its padded copy,
    original width); zero columns aggregate to zero columns, the caller slices them off (autograd pads the gradient)."""
    d = x.size(1)
    if d % 4 == 0 or not x.is_cuda:
        return x, d
    base = getattr(x, "_rgbx_base", None)
    if base is not None and not x.requires_grad:  # align_rows made the padded matrix already (pad columns zero)
        return base, d
    return torch.nn.functional.pad(x, (0, 4 - d % 4)), d


def _pad4_vec(v, d_padded):
    return v if v is None or v.numel() == d_padded else torch.nn.functional.pad(v, (0, d_padded - v.numel()))


def propagate_gcn(x, graph, bias=None):
    """A_hat x (+ bias, fused into the kernel's store)."""
    if _is_dist(graph):
        out = graph.propagate(x, "gcn")
        return out if bias is None else out + bias
    xp, d = _pad4(x)
    out = _PropagateGCN.apply(xp, graph, _pad4_vec(bias, xp.size(1)))
    return out if xp is x else out[:, :d]


def edge_dot_raw(csr, a, b, kind="edge_dot"):
    """g[p] = <a[i], b[col[p]]> for every slot p of row i of `csr` (rgbx_edge_dot_f32; no autograd): dL/dw of a weighted
    aggregation with a = dL/dout and b = the gathered matrix. Widths that are no multiple of 4 run zero-padded; widths
    above 256 in column blocks of 256 whose dots are added."""
    _lib.require_device(a, b)
    if a.size(1) % 4:
        pad = 4 - a.size(1) % 4
        a, b = torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(b, (0, pad))
    a, b = _rows_on_grid(a), _rows_on_grid(b)
    d = a.size(1)
    g = torch.empty(max(csr.nnz, 1), dtype=torch.float32, device=a.device)
    total = None
    for c0 in range(0, d, 256):
        c1 = min(c0 + 256, d)
        split, _scratch = (None, None) if csr.split is None else csr.split_arg(1, a.device)
        _launch(kind, "rgbx_edge_dot_f32", csr.rowptr, csr.col, _lib.mat(a[:, c0:c1], "a"), _lib.mat(b[:, c0:c1], "b"), g,
                csr.N, c1 - c0, split, variant=f"rows+d{c1 - c0}" if _EVENT_SINK is not None else None)
        if c1 < d or total is not None:
            total = g.clone() if total is None else total.add_(g)
    return g if total is None else total


def gcn_norm_bwd(graph, g_slot):
    """dL/d edge_weight [E] of a graph.WeightedGraph from dL/dw per forward slot (rgbx_gcn_norm_bwd_f32)."""
    f, b = graph.fwd, graph.bwd
    dev = f.rowptr.device
    dew = torch.empty(max(graph.E, 1), dtype=torch.float32, device=dev)
    ddeg = torch.empty(max(graph.N, 1), dtype=torch.float32, device=dev)
    _launch("gcn_norm_bwd", "rgbx_gcn_norm_bwd_f32", f.rowptr, f.col, f.perm, b.rowptr, b.col, graph.t2f, graph.loops[1],
            g_slot, graph.ew_slot, graph.dis, graph.N, graph.E, ddeg, dew)
    return dew[:graph.E]


class _PropagateGCNEdgeWeight(torch.autograd.Function):
    """A_hat(ew) h with the gradient in the edge weights as well (gcn_norm with edge_weight, dagnn.py:12-31; message
    dagnn.py:57-59). Forward = the row gather, dh = the transposed gather, d ew = the per-slot dots <dY[i], h[col[p]]>
    (rgbx_edge_dot_f32) pushed through the normalisation's backward (rgbx_gcn_norm_bwd_f32)."""

    @staticmethod
    def forward(ctx, h, edge_weight, graph, bias):
        ctx.graph, ctx.has_bias = graph, bias is not None
        ctx.save_for_backward(h)
        b = None if bias is None else bias.detach().contiguous()
        return spmm_raw(graph.fwd, graph.w, None, h, kind="gcn_fwd", bias=b)

    @staticmethod
    def backward(ctx, gy):
        g = ctx.graph
        (h,) = ctx.saved_tensors
        gy = gy.contiguous()
        gh = spmm_raw(g.bwd, g.w_t, None, gy, kind="gcn_bwd") if ctx.needs_input_grad[0] else None
        gew = gcn_norm_bwd(g, edge_dot_raw(g.fwd, gy, h)) if ctx.needs_input_grad[1] else None
        gb = gy.sum(0) if ctx.has_bias and ctx.needs_input_grad[3] else None
        return gh, gew, None, gb


def propagate_gcn_edge_weight(h, edge_weight, graph, bias=None):
    """A_hat(edge_weight) h (+ bias) for an edge_weight that requires grad; `graph` = get_graph(..., edge_weight)."""
    hp, d = _pad4(h)
    out = _PropagateGCNEdgeWeight.apply(hp, edge_weight, graph, _pad4_vec(bias, hp.size(1)))
    return out if hp is h else out[:, :d]


def propagate_mean(x, graph):
    if _is_dist(graph):
        return graph.propagate(x, "mean")
    xp, d = _pad4(x)
    out = _PropagateMean.apply(xp, graph)
    return out if xp is x else out[:, :d]


def propagate_sum(x, graph):
    if _is_dist(graph):
        return graph.propagate(x, "sum")
    xp, d = _pad4(x)
    out = _PropagateSum.apply(xp, graph)
    return out if xp is x else out[:, :d]


# ---- max / min over the neighbourhood (aggr='max' | 'min') --------------------------------------------------------------

EXTREMUM_MODES = {"max": 0, "min": 1}  # RGBX_EXTREMUM_MAX / RGBX_EXTREMUM_MIN


def spmm_extremum_raw(csr, x, mode, want_arg, kind=None):
    """(out [N, d], arg int32 [N, d] or None): out[i, c] = max / min over the slots p of row i of x[col[p], c], arg the
    slot that supplied it (lowest slot on ties; rows without slots: 0 / -1). No autograd; rgbx_spmm_csr_extremum_f32.
    `x` has a width that is a multiple of 4 (callers pad, cf. _pad4); widths above 256 run in column blocks of 256 (an
    extremum is taken per column). `want_arg=False` is the inference form: no arg is allocated or written."""
    if mode not in EXTREMUM_MODES:
        raise ValueError(f"mode must be 'max' or 'min', got {mode!r}")
    _lib.require_device(x)
    x = _rows_on_grid(x)
    N, d = csr.N, x.size(1)
    if d % 4:
        raise RuntimeError(f"spmm_extremum_raw: width {d} is no multiple of 4 (pad the rows)")
    out = torch.empty((N, d), dtype=torch.float32, device=x.device)
    arg = torch.empty((N, d), dtype=torch.int32, device=x.device) if want_arg else None
    for c0 in range(0, d, 256):
        c1 = min(c0 + 256, d)
        w = c1 - c0
        # one column block's arg rows are [N, w] with leading dimension w: a block of a wider matrix gets its own buffer
        blk = arg if (arg is None or w == d) else torch.empty((N, w), dtype=torch.int32, device=x.device)
        split, _scratch = csr.split_arg(2 * w, x.device)  # chunk values + chunk slots
        _launch(kind or f"{mode}_fwd", "rgbx_spmm_csr_extremum_f32", csr.rowptr, csr.col, _lib.mat(x[:, c0:c1], "x"),
                _lib.mat(out[:, c0:c1], "out"), blk, N, w, EXTREMUM_MODES[mode], split,
                variant=f"rows+d{w}" + ("+arg" if want_arg else "") if _EVENT_SINK is not None else None)
        if blk is not arg:
            arg[:, c0:c1] = blk
    return out, arg


def extremum_bwd_raw(graph, gout, arg, kind="extremum_bwd"):
    """gx[j, c] = sum over the out-edges q of j (target i) of gout[i, c] * [arg[i, c] == forward slot of q], over the
    transposed CSR (rgbx_extremum_bwd_f32; fixed summation order, no atomics). No autograd."""
    _lib.require_device(gout, arg)
    csr, t2f = graph.bwd, graph.t2f
    gout = _rows_on_grid(gout)
    d = gout.size(1)
    gx = torch.empty((csr.N, d), dtype=torch.float32, device=gout.device)
    for c0 in range(0, d, 256):
        c1 = min(c0 + 256, d)
        w = c1 - c0
        blk = arg if w == d else arg[:, c0:c1].contiguous()
        split, _scratch = csr.split_arg(w, gout.device)
        _launch(kind, "rgbx_extremum_bwd_f32", csr.rowptr, csr.col, t2f, _lib.mat(gout[:, c0:c1], "gout"), blk,
                _lib.mat(gx[:, c0:c1], "gx"), csr.N, w, split, variant=f"rows+d{w}" if _EVENT_SINK is not None else None)
    return gx


class _PropagateExtremum(torch.autograd.Function):
    """max / min over incoming edges (aggr='max' | 'min'; graphsage.py:38-40 leaves the aggregator to the caller). The
    forward keeps the winning slot of every (row, column) only when a gradient will be asked for; the backward routes
    gout through those slots over the transposed CSR."""

    @staticmethod
    def forward(ctx, x, graph, mode, want):
        ctx.graph = graph
        out, arg = spmm_extremum_raw(graph.fwd, x, mode, want)
        if want:
            graph.t2f  # built here, outside the backward (its construction reads sizes back to the host)
            ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, gy):
        (arg,) = ctx.saved_tensors
        return extremum_bwd_raw(ctx.graph, gy, arg), None, None, None


def _propagate_extremum(x, graph, mode):
    if _is_dist(graph):
        raise NotImplementedError(f"aggr='{mode}' is not implemented on the partitioned (distributed) route")
    _lib.require_device(x)
    xp, d = _pad4(x)
    # decided here: inside a Function's forward the grad mode is always off and cannot tell no_grad from training
    want = torch.is_grad_enabled() and xp.requires_grad
    out = _PropagateExtremum.apply(xp, graph, mode, want)
    return out if xp is x else out[:, :d]


def propagate_max(x, graph):
    """out[i] = max_{j in N(i)} x[j] per column over `graph` (0 where i has no in-edge)."""
    return _propagate_extremum(x, graph, "max")


def propagate_min(x, graph):
    """out[i] = min_{j in N(i)} x[j] per column over `graph` (0 where i has no in-edge)."""
    return _propagate_extremum(x, graph, "min")


# ---- several statistics of the neighbourhood from one gather (aggr='std' | 'var' | a list of aggregators) ------------

MULTI_BITS = {"sum": 1, "mean": 2, "var": 4, "std": 8, "max": 16, "min": 32}  # RGBX_MULTI_*


def multi_names(aggrs):
    """A string or a non-empty list / tuple of distinct aggregator names as the tuple of the kernel's names ('add' is
    'sum'); anything else: ValueError."""
    seq = (aggrs,) if isinstance(aggrs, str) else aggrs
    if not isinstance(seq, (list, tuple)) or not seq or not all(isinstance(a, str) for a in seq):
        raise ValueError(f"aggr must be a name or a non-empty list of names out of {sorted(MULTI_BITS) + ['add']}, got {aggrs!r}")
    names = tuple("sum" if a == "add" else a for a in seq)
    if any(a not in MULTI_BITS for a in names) or len(set(names)) != len(names):
        raise ValueError(f"aggr must name distinct aggregators out of {sorted(MULTI_BITS) + ['add']}, got {aggrs!r}")
    return names


def _block_ptr(t, c0, c1):
    """(pointer, leading dimension) of the column block [c0, c1) of a row-major matrix."""
    return t[:, c0:c1].data_ptr(), (t.stride(0) if t.size(0) > 1 else max(t.size(1), 1))


def spmm_multi_raw(csr, x, which, want_arg, keep=(), kind="multi_fwd"):
    """(out [N, k*d], argmax, argmin, kept): the k statistics `which` of every row's neighbourhood, concatenated in that
    order, from ONE gather pass over `csr` (rgbx_spmm_csr_multi_f32: every statistic is written straight into its column
    block). argmax / argmin: int32 [N, d] winning slots when `want_arg` and that extremum is asked for, else None
    (`want_arg=False` is the inference form). `keep`: further statistics, computed in the same pass into [N, d] matrices
    of their own (kept[name]) — what a backward needs and the output does not hold. No autograd. Widths that are no
    multiple of 4 run zero-padded; widths above 256 in column blocks of 256 (every statistic is taken per column)."""
    names = multi_names(which)
    _lib.require_device(x)
    d = x.size(1)
    if d % 4:
        x = torch.nn.functional.pad(x, (0, 4 - d % 4))
    x = _rows_on_grid(x)
    N, dp, k, dev = csr.N, x.size(1), len(names), x.device
    buf = torch.empty((N, k * dp), dtype=torch.float32, device=dev)
    dest = {a: buf[:, s * dp:(s + 1) * dp] for s, a in enumerate(names)}
    kept = {a: torch.empty((N, dp), dtype=torch.float32, device=dev) for a in multi_names(keep) if a not in dest} if keep else {}
    dest.update(kept)
    args = {a: torch.empty((N, dp), dtype=torch.int32, device=dev) for a in ("max", "min") if want_arg and a in names}
    bits = sum(MULTI_BITS[a] for a in dest)
    for c0 in range(0, dp, 256):
        c1 = min(c0 + 256, dp)
        w = c1 - c0
        o = _lib.MultiOut()
        for a, t in dest.items():
            p, ld = _block_ptr(t, c0, c1)
            setattr(o, a, p)
            setattr(o, "ld_" + a, ld)
        for a, t in args.items():
            p, ld = _block_ptr(t, c0, c1)
            setattr(o, "arg" + a, p)
            setattr(o, "ld_arg" + a, ld)
        split = None
        if csr.split is not None:
            words = ctypes.c_int64(0)
            _lib.call("rgbx_spmm_csr_multi_partial_words", csr.split["n_chunks"], w, bits, ctypes.byref(words))
            split, _scratch = csr.split_arg(words.value // csr.split["n_chunks"], dev)
        _launch(kind, "rgbx_spmm_csr_multi_f32", csr.rowptr, csr.col, _block_ptr(x, c0, c1), o, N, w, split,
                variant=f"rows+d{w}+{'+'.join(dest)}" + ("+arg" if args else "") if _EVENT_SINK is not None else None)
    out = buf if dp == d else buf.view(N, k, dp)[:, :, :d].reshape(N, k * d)
    cut = (lambda t: t) if dp == d else (lambda t: t[:, :d])
    return (out, cut(args["max"]) if "max" in args else None, cut(args["min"]) if "min" in args else None,
            {a: cut(t) for a, t in kept.items()})


def multi_bwd_raw(graph, a=None, b=None, x=None, gmax=None, argmax=None, gmin=None, argmin=None, kind="multi_bwd"):
    """gx[j] = sum_q a[i] + x[j] * sum_q b[i] + sum_q gmax[i] [argmax[i] == slot of q] + sum_q gmin[i] [argmin[i] == slot of
    q] over the out-edges q of j (target i), in ONE pass over the transposed CSR (rgbx_multi_bwd_f32; fixed summation order,
    no atomics). a, b, gmax, gmin: float32 [N, d] per TARGET (column blocks of a wider matrix are read in place); terms that
    are None are neither read nor added. No autograd. Widths as spmm_multi_raw."""
    terms = {"a": a, "b": b, "x": x if b is not None else None, "gmax": gmax, "argmax": argmax, "gmin": gmin,
             "argmin": argmin}
    terms = {k: v for k, v in terms.items() if v is not None}
    if not terms:
        raise ValueError("multi_bwd_raw: no term given")
    _lib.require_device(*terms.values())
    d = next(iter(terms.values())).size(1)
    if d % 4:
        terms = {k: torch.nn.functional.pad(v, (0, 4 - d % 4), value=-1 if k.startswith("arg") else 0)
                 for k, v in terms.items()}
    terms = {k: _rows_on_grid(v) for k, v in terms.items()}
    csr = graph.bwd
    t2f = graph.t2f if ("gmax" in terms or "gmin" in terms) else None
    dp, dev = (d + 3) // 4 * 4, next(iter(terms.values())).device
    gx = torch.empty((csr.N, dp), dtype=torch.float32, device=dev)
    for c0 in range(0, dp, 256):
        c1 = min(c0 + 256, dp)
        w = c1 - c0
        t = _lib.MultiGrad()
        for k, v in terms.items():
            p, ld = _block_ptr(v, c0, c1)
            setattr(t, k, p)
            setattr(t, "ld_" + k, ld)
        split, _scratch = csr.split_arg(w, dev)
        _launch(kind, "rgbx_multi_bwd_f32", csr.rowptr, csr.col, t2f, t, _block_ptr(gx, c0, c1), csr.N, w, split,
                variant=f"rows+d{w}+{'+'.join(terms)}" if _EVENT_SINK is not None else None)
    return gx if dp == d else gx[:, :d]


class _PropagateMulti(torch.autograd.Function):
    """[stat_1(N(i)) | ... | stat_k(N(i))] over incoming edges (PyG MultiAggregation, mode='cat'; a single 'std' / 'var' is
    the k = 1 case). The forward keeps x, the mean, the output (for its std block) and the winning slots only when a
    gradient will be asked for; the backward folds every statistic's cotangent into two per-target rows (a, b) with
    elementwise arithmetic and routes them, with the extremum cotangents, through one transposed gather."""

    @staticmethod
    def forward(ctx, x, graph, names, want):
        second = want and ("std" in names or "var" in names)
        keep = ("mean",) if second and "mean" not in names else ()
        out, amax, amin, kept = spmm_multi_raw(graph.fwd, x, names, want, keep=keep)
        ctx.graph, ctx.names = graph, names
        if want:
            # built here, outside the backward (their construction reads sizes back to the host)
            graph.bwd, graph.inv_deg
            if amax is not None or amin is not None:
                graph.t2f
            ctx.save_for_backward(x if second else None, out if second else None, kept.get("mean"), amax, amin)
        return out

    @staticmethod
    def backward(ctx, gy):
        x, out, kept_mean, amax, amin = ctx.saved_tensors
        names, g = ctx.names, ctx.graph
        gy = _rows_on_grid(gy)
        dp = gy.size(1) // len(names)
        blk = lambda t, a: t[:, names.index(a) * dp:(names.index(a) + 1) * dp]
        inv_n = g.inv_deg[:g.N, None]  # 1 / max(n, 1)
        a = b = None
        if "std" in names:  # d std / d x_j = (x_j - mean) / (n std); 0 where the clamp or the mask is active (std == 0)
            std = blk(out, "std")
            b = torch.where(std > 0, blk(gy, "std") * inv_n / std, torch.zeros_like(std))
        if "var" in names:  # d var / d x_j = 2 (x_j - mean) / n
            t = blk(gy, "var") * (2.0 * inv_n)
            b = t if b is None else b + t
        if b is not None:
            # sum_q b_i (x_j - mean_i) as x_j sum_q b_i - sum_q b_i mean_i cancels on features with an offset (x = 50 +
            # 0.05 noise: both halves are 1000 times their difference). Both are taken relative to the column mean s of
            # x — (x_j - s) sum_q b_i - sum_q b_i (mean_i - s), the same number — so the kernel's `x` is x - s
            s = x.mean(0, keepdim=True)
            a = -b * ((blk(out, "mean") if "mean" in names else kept_mean) - s)
            x = x - s
        if "sum" in names:
            a = blk(gy, "sum") if a is None else a + blk(gy, "sum")
        if "mean" in names:
            t = blk(gy, "mean") * inv_n
            a = t if a is None else a + t
        gx = multi_bwd_raw(g, a=a, b=b, x=x, gmax=blk(gy, "max") if "max" in names else None, argmax=amax,
                           gmin=blk(gy, "min") if "min" in names else None, argmin=amin)
        return gx, None, None, None


def propagate_multi(x, graph, aggrs):
    """[N, k*d]: the statistics `aggrs` (a list out of 'sum' / 'add', 'mean', 'var', 'std', 'max', 'min') of every node's
    in-neighbourhood, concatenated in that order, from one gather pass; 0 in every block where a node has no in-edge."""
    names = multi_names(aggrs)
    if _is_dist(graph):
        raise NotImplementedError(f"aggr={aggrs!r} is not implemented on the partitioned (distributed) route")
    _lib.require_device(x)
    xp, d = _pad4(x)
    # decided here: inside a Function's forward the grad mode is always off and cannot tell no_grad from training
    want = torch.is_grad_enabled() and xp.requires_grad
    out = _PropagateMulti.apply(xp, graph, names, want)
    if xp is x:
        return out
    return out.view(out.size(0), len(names), xp.size(1))[:, :, :d].reshape(out.size(0), len(names) * d)


def propagate_std(x, graph):
    """out[i] = the (biased) standard deviation of x over N(i) per column, 0 where the variance is at most 1e-5."""
    return propagate_multi(x, graph, ("std",))


def propagate_var(x, graph):
    """out[i] = mean(x^2) - mean(x)^2 over N(i) per column (biased, not clamped)."""
    return propagate_multi(x, graph, ("var",))


# ---- propagate of an already transformed matrix, with the passes that follow it taken in the same kernel --------------

def pad_rows4(weight, *vectors):
    """A Linear's weight [out, in] (and [out] vectors next to it) with zero rows up to the next multiple of 4: the product
    then comes out in 16-byte rows (C = 7 classes -> 8 columns) and no pad copy of the [N, C] matrix is needed in front of
    the aggregation (cf. _pad4). Differentiable (the pad's backward is a slice). Returns (weight', *vectors', padded out)."""
    n = weight.size(0)
    p = (-n) % 4
    if p == 0:
        return (weight,) + vectors + (n,)
    pad = torch.nn.functional.pad
    return (pad(weight, (0, 0, 0, p)),) + tuple(None if v is None else pad(v, (0, p)) for v in vectors) + (n + p,)


def rows_epilogue_ok(graph, width, x=None, y=None):
    """The row gather can take BatchNorm's column sums / the masked cross-entropy of its output into the kernel
    (rgbx_spmm_csr_epilogue_f32): single-GPU graph, device tensors, `width` (a multiple of 4) <= 256."""
    return (not _is_dist(graph) and width % 4 == 0 and 0 < width <= 256 and (x is None or x.is_cuda)
            and (y is None or (y.is_cuda and y.dtype == torch.int64)))


def spmm_epilogue_raw(csr, w, rs, x, y=None, a=1.0, b=0.0, bias=None, out=None, want_colsums=False, ce=None, n_classes=0,
                      kind="spmm"):
    """spmm_raw with an epilogue over the finished rows (no autograd; rgbx_spmm_csr_epilogue_f32). Exactly one of
    `want_colsums` -> (out, colsums [2, d] float64 of out and out^2), and `ce` = (labels, mask or (mask_a, mask_b),
    grad_scale or None) -> (loss gradient w.r.t. the logits, or None when grad_scale is None: nothing is written; stats [3]
    or [2, 3] float64 = nll sum, selected rows, correct). `n_classes`: columns beyond are padding (see pad_rows4)."""
    _lib.require_device(x, y, bias)
    xm = _lib.mat(x, "x")
    N, d = csr.N, x.size(1)
    ym = _lib.mat_opt(y, "y")
    keep = []
    E = _lib.SpmmEpilogue()
    stats = colsums = None
    want_out = True
    if ce is not None:
        labels, mask, grad_scale = ce
        groups = 1
        if isinstance(mask, (tuple, list)):
            if grad_scale is not None:
                raise RuntimeError("spmm_epilogue_raw: two masks are for statistics only (no loss gradient)")
            mask, groups = group_masks(*mask), 2
        _lib.require_device(labels, mask, grad_scale)
        if labels.dtype != torch.int64:
            raise RuntimeError(f"labels must be int64, got {labels.dtype}")
        if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError(f"mask must be bool, got {mask.dtype}")
        labels = labels.contiguous()
        mask = None if mask is None else mask.contiguous()
        stats = torch.empty(3 * groups, dtype=torch.float64, device=x.device)
        scratch = torch.empty(3 * groups * ((N + 31) // 32 + 64), dtype=torch.float64, device=x.device)
        ce_arg = _lib.CeEpilogue(_lib.ptr(labels), _lib.ptr(mask), _lib.ptr(grad_scale), _lib.ptr(stats), _lib.ptr(scratch),
                                 groups)
        keep += [labels, mask, scratch, ce_arg, grad_scale]
        E.ce, E.n_classes = ctypes.addressof(ce_arg), int(n_classes)
        want_out = grad_scale is not None
    elif want_colsums:
        nbytes = ctypes.c_size_t(0)
        _lib.call("rgbx_spmm_linear_stats_workspace_bytes", N, d, ctypes.byref(nbytes))
        ws = torch.empty(max(nbytes.value, 8), dtype=torch.uint8, device=x.device)
        colsums = torch.empty((2, d), dtype=torch.float64, device=x.device)
        keep.append(ws)
        E.out_colsums, E.stats_ws, E.stats_ws_bytes = colsums.data_ptr(), ws.data_ptr(), nbytes.value
    else:
        raise RuntimeError("spmm_epilogue_raw: no epilogue asked for (use spmm_raw)")
    if out is None and want_out:
        out = torch.empty((N, d), dtype=torch.float32, device=x.device)
    split, _scratch = csr.split_arg(d, x.device, hub_rows=1)
    variant = None
    if _EVENT_SINK is not None:
        variant = "rows+" + ("stats" if ce is None else ("ce_grad" if want_out else "ce_stats")) + f"+d{d}"
    _launch(kind, "rgbx_spmm_csr_epilogue_f32", csr.rowptr, csr.col, w, rs, xm, ym, bias,
            (0, d) if out is None else _lib.mat(out, "out"), N, d, float(a), float(b), split, E, variant=variant)
    del keep
    if ce is not None:
        return out, (stats.view(2, 3) if stats.numel() == 6 else stats)
    return out, colsums


def _kind_weights(graph, kind, transposed=False):
    """(per-slot weights, per-row scale) of the aggregation `kind` on the forward / the transposed CSR."""
    if kind == "gcn":
        return (graph.w_t, None) if transposed else (graph.w, None)
    if kind == "mean":
        return (graph.w_mean_t, None) if transposed else (None, graph.inv_deg)
    if kind == "sum":
        return None, None
    raise ValueError(kind)


class _PropagateRows(torch.autograd.Function):
    """out = P h[:, :n] (+ h[:, n:2n]) (+ bias), P = A_hat ('gcn'), the mean operator ('mean') or the plain edge sum
    ('sum'): the aggregation of a layer that has ALREADY been transformed (in > out: the reference's default shapes,
    initial_params.py:25-29), with the layer's root / self term as the right half of the same matrix — one GEMM
    x [W_l; W_r]^T reads the (wide) input once for both halves (models/graphsage.py:49-50 runs two Linears, SAGEConv [PyG]
    likewise) and the add is the kernel's `y` operand. `mode`:
      'plain'    returns out                      (rgbx_spmm_csr_f32)
      'colsums'  returns (out, colsums [2, n])    (a training-mode BatchNorm follows: models/gcn.py:28)
      'ce'       returns (loss, stats)            (the model's last layer: gcn.py:31 + itexperiments.py:429,624-626);
                 ce_args = (labels, mask, n_classes, want_grad); the logits are never written
    Backward: g_h[:, :n] = P^T g_out on the transposed CSR, g_h[:, n:] = g_out, g_bias = column sums of g_out; in 'ce'
    mode g_out is the loss gradient the forward stored, times the incoming scalar."""

    @staticmethod
    def forward(ctx, h, graph, kind, n, bias, mode, ce_args):
        split = h.size(1) == 2 * n
        if not split and h.size(1) != n:
            raise RuntimeError(f"propagate_rows: h is {tuple(h.shape)} for n = {n}")
        h = h if h.stride(-1) == 1 else h.contiguous()
        w, rs = _kind_weights(graph, kind)
        x = h[:, :n] if split else h
        y = h[:graph.fwd.N, n:] if split else None
        b = None if bias is None else bias.detach().contiguous()
        prefix = getattr(graph, "event_prefix", "")
        ctx.graph, ctx.kind, ctx.n, ctx.split, ctx.mode = graph, kind, n, split, mode
        ctx.has_bias, ctx.h_shape = bias is not None, tuple(h.shape)
        if mode == "plain":
            return spmm_raw(graph.fwd, w, rs, x, y=y, a=1.0, b=1.0, kind=f"{prefix}{kind}_fwd", bias=b)
        if mode == "colsums":
            out, cs = spmm_epilogue_raw(graph.fwd, w, rs, x, y=y, a=1.0, b=1.0, bias=b, want_colsums=True,
                                        kind=f"{prefix}{kind}_fwd")
            ctx.mark_non_differentiable(cs)
            return out, cs
        labels, mask, n_classes, want_grad = ce_args
        grad_scale = mask_scale(labels, mask, n_classes) if want_grad else None
        dlogits, stats = spmm_epilogue_raw(graph.fwd, w, rs, x, y=y, a=1.0, b=1.0, bias=b,
                                           ce=(labels, mask, grad_scale), n_classes=n_classes, kind=f"{prefix}{kind}_fwd")
        if want_grad:
            ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(stats)
        if stats.dim() == 2:  # two masks, statistics only
            return stats.new_zeros(()).float(), stats
        return (stats[0] / stats[1]).float(), stats

    @staticmethod
    def backward(ctx, g, _g_extra=None):
        graph, kind, n = ctx.graph, ctx.kind, ctx.n
        if ctx.mode == "ce":
            if not ctx.saved_tensors:
                raise RuntimeError("propagate_rows: backward asked of a loss forward that was run without want_grad")
            gy = ctx.saved_tensors[0] * g.reshape(()).float()
        else:
            gy = g.contiguous()
        gh = gb = None
        if ctx.needs_input_grad[0]:
            wt, _ = _kind_weights(graph, kind, transposed=True)
            prefix = getattr(graph, "event_prefix", "")
            gh = torch.empty(ctx.h_shape, dtype=torch.float32, device=gy.device)
            if ctx.split:
                gh[:graph.fwd.N, n:].copy_(gy)
                if gh.size(0) > graph.fwd.N:
                    gh[graph.fwd.N:, n:].zero_()
            spmm_raw(graph.bwd, wt, None, gy, out=gh[:, :n] if ctx.split else gh, kind=f"{prefix}{kind}_bwd")
        if ctx.has_bias and ctx.needs_input_grad[4]:
            gb = gy.sum(0)
        return gh, None, None, None, gb, None, None


def propagate_rows(h, graph, kind, n=None, bias=None, want_colsums=False):
    """P h[:, :n] (+ h[:, n:2n]) (+ bias) — see _PropagateRows; `n` defaults to h's width (no addend half). With
    `want_colsums` the output carries its column sums for the BatchNorm that follows (ops.COLSUMS) where the kernel can
    take them (rows_epilogue_ok), and is a plain output otherwise."""
    n = h.size(1) if n is None else n
    if want_colsums and rows_epilogue_ok(graph, n, h):
        return _tag_colsums(_PropagateRows.apply(h, graph, kind, n, bias, "colsums", None), True)
    return _PropagateRows.apply(h, graph, kind, n, bias, "plain", None)


def propagate_rows_ce(h, graph, kind, n, n_classes, y, mask, bias=None):
    """(loss, stats) of the masked cross-entropy of the logits P h[:, :n] (+ h[:, n:2n]) (+ bias), columns [n_classes, n)
    being padding — taken inside the gather kernel (the caller checked rows_epilogue_ok). `mask` = (mask_a, mask_b):
    (None, [2, 3] statistics) of one eval forward under both masks."""
    pair = isinstance(mask, (tuple, list))
    want_grad = (not pair) and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (h, bias))
    loss, stats = _PropagateRows.apply(h, graph, kind, n, bias, "ce", (y, mask, int(n_classes), want_grad))
    return (None if pair else loss), stats


# ---- the row gather with the gathered matrix stored as bfloat16 (rgbx_spmm_csr_bf16) ----------------------------------
# The gather is memory-bound and the gathered table is most of its bytes; stored as bfloat16 that term halves. Values are
# rounded ONCE (to nearest-even, rgbx_rows_f32_to_bf16) in front of the gather; every sum, the addend, the bias and the
# output are fp32. Opt-in (the layers' gather_dtype keyword): no fp32 route goes through here.

BF16_MAX_WIDTH = 256  # rgbx_spmm_csr_bf16_supported: wider matrices are gathered in column blocks of this many


def pad_rows8(weight, *vectors):
    """pad_rows4 for the bfloat16 gather: zero rows up to the next multiple of 8 (a lane of rgbx_spmm_csr_bf16 holds 8
    columns = 16 bytes). Returns (weight', *vectors', padded out)."""
    n = weight.size(0)
    p = (-n) % 8
    if p == 0:
        return (weight,) + vectors + (n,)
    pad = torch.nn.functional.pad
    return (pad(weight, (0, 0, 0, p)),) + tuple(None if v is None else pad(v, (0, p)) for v in vectors) + (n + p,)


def _no_dist_bf16(graph):
    if _is_dist(graph):
        raise NotImplementedError("the bfloat16 gather is not implemented on the partitioned (distributed) route")


def to_bf16_rows(t):
    """fp32 [n, d] (rows contiguous, possibly a column slice of a wider matrix) -> a fresh contiguous torch.bfloat16
    [n, d], rounded to nearest-even by rgbx_rows_f32_to_bf16 (the bits of t.to(torch.bfloat16)); no autograd."""
    _lib.require_device(t)
    t = t.detach()
    t = t if t.dim() != 2 or t.stride(-1) == 1 or t.size(1) <= 1 else t.contiguous()
    tm = _lib.mat(t, "t")
    n, d = t.shape
    out = torch.empty((n, d), dtype=torch.bfloat16, device=t.device)
    _launch("rows_to_bf16", "rgbx_rows_f32_to_bf16", tm, out, max(d, 1), n, d,
            variant=f"d{d}" if _EVENT_SINK is not None else None)
    return out


def spmm_bf16_raw(csr, w, rs, xb, y=None, a=1.0, b=0.0, bias=None, out=None, out_dtype=torch.float32, kind="spmm_bf16"):
    """out[i] = a*rs[i]*sum_p w[p]*xb[col[p]] + b*y[i] + bias over `csr` with xb stored as bfloat16 and every sum in
    fp32 (no autograd; rgbx_spmm_csr_bf16). `out_dtype`: torch.float32, or torch.bfloat16 for the result rounded to
    nearest-even in the kernel's store; `out` (of that dtype) may be given. The width must be a multiple of 8 (pad_rows8);
    beyond BF16_MAX_WIDTH the columns are gathered in blocks of that many (one launch each, the same sums)."""
    if not isinstance(xb, torch.Tensor) or xb.dtype != torch.bfloat16:
        raise RuntimeError(f"spmm_bf16_raw: xb must be a torch.bfloat16 matrix, got {getattr(xb, 'dtype', type(xb))}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"spmm_bf16_raw: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    _lib.require_device(xb, y, bias, out)
    xb = xb if xb.stride(-1) == 1 else xb.contiguous()
    px, ldx = _lib.mat_bf16(xb, "xb")
    N, d = csr.N, xb.size(1)
    if d % 8:
        raise RuntimeError(f"spmm_bf16_raw: width {d} is no multiple of 8 (zero-pad the rows: ops.pad_rows8)")
    if out is None:
        out = torch.empty((N, d), dtype=out_dtype, device=xb.device)
    elif out.dtype != out_dtype or tuple(out.shape) != (N, d):
        raise RuntimeError(f"spmm_bf16_raw: out is {out.dtype} {tuple(out.shape)}, expected {out_dtype} {(N, d)}")
    po, ldo = _lib.mat(out, "out") if out_dtype == torch.float32 else _lib.mat_bf16(out, "out")
    # the kernel reads y and bias four floats at a time: an addend half behind an offset view, a bias sliced out of a flat
    # parameter buffer are copied onto that grid (the sums are read from the copy, `out` may still alias the original)
    y = None if y is None else _rows_on_grid(y)
    py, ldy = _lib.mat_opt(y, "y")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != d):
        raise RuntimeError(f"spmm_bf16_raw: bias must be float32 [{d}]")
    bias = _vec_on_grid(bias, d)
    pb = _lib.ptr(bias)
    for c0 in range(0, max(d, 1), BF16_MAX_WIDTH):  # the column blocks are pointer offsets into the same matrices
        dc = min(BF16_MAX_WIDTH, d - c0)
        split, _scratch = csr.split_arg(dc, xb.device)
        f32 = (po + 4 * c0, ldo, 0, 0) if out_dtype == torch.float32 else (0, 0, po + 2 * c0, ldo)
        _launch(kind, "rgbx_spmm_csr_bf16", csr.rowptr, csr.col, w, rs, px + 2 * c0, ldx, py + 4 * c0 if py else 0, ldy,
                pb + 4 * c0 if pb else 0, f32, N, dc, float(a), float(b), split,
                variant=f"rows+d{dc}" if _EVENT_SINK is not None else None)
    return out


class _PropagateRowsBF16(torch.autograd.Function):
    """_PropagateRows in mode 'plain' with the gathered half stored as bfloat16: out = P bf16(h[:, :n]) (+ h[:, n:2n])
    (+ bias), fp32 sums and output. Backward: g_h[:, :n] = P^T bf16(g_out) on the transposed CSR, g_h[:, n:] = g_out,
    g_bias = column sums of g_out; the rounding counts as the identity in the gradient. Only the passes whose gradients
    are asked for run."""

    @staticmethod
    def forward(ctx, h, graph, kind, n, bias):
        split = h.size(1) == 2 * n
        if not split and h.size(1) != n:
            raise RuntimeError(f"propagate_rows_bf16: h is {tuple(h.shape)} for n = {n}")
        h = h if h.stride(-1) == 1 else h.contiguous()
        w, rs = _kind_weights(graph, kind)
        xb = to_bf16_rows(h[:, :n] if split else h)
        y = h[:, n:] if split else None
        b = None if bias is None else bias.detach().contiguous()
        ctx.graph, ctx.kind, ctx.n, ctx.split = graph, kind, n, split
        ctx.has_bias, ctx.h_shape = bias is not None, tuple(h.shape)
        return spmm_bf16_raw(graph.fwd, w, rs, xb, y=y, a=1.0, b=1.0, bias=b, kind=f"{kind}_fwd_bf16")

    @staticmethod
    def backward(ctx, g):
        graph, kind, n = ctx.graph, ctx.kind, ctx.n
        gy = g.contiguous()
        gh = gb = None
        if ctx.needs_input_grad[0]:
            wt, _ = _kind_weights(graph, kind, transposed=True)
            gh = torch.empty(ctx.h_shape, dtype=torch.float32, device=gy.device)
            if ctx.split:
                gh[:, n:].copy_(gy)
            spmm_bf16_raw(graph.bwd, wt, None, to_bf16_rows(gy), out=gh[:, :n] if ctx.split else gh,
                          kind=f"{kind}_bwd_bf16")
        if ctx.has_bias and ctx.needs_input_grad[4]:
            gb = gy.sum(0)
        return gh, None, None, None, gb


def propagate_rows_bf16(h, graph, kind, n=None, bias=None):
    """P h[:, :n] (+ h[:, n:2n]) (+ bias) with the gathered left half rounded to bfloat16 — see _PropagateRowsBF16. `kind`
    in 'gcn' / 'mean' / 'sum'; `n` defaults to h's width (no addend half) and must be a multiple of 8: the caller
    zero-pads (pad_rows8)."""
    if kind not in ("gcn", "mean", "sum"):
        raise ValueError(f"propagate_rows_bf16: kind must be 'gcn', 'mean' or 'sum', got {kind!r}")
    _no_dist_bf16(graph)
    _lib.require_device(h, bias)
    n = h.size(1) if n is None else n
    if n % 8:
        raise RuntimeError(f"propagate_rows_bf16: n = {n} is no multiple of 8 (zero-pad the rows: ops.pad_rows8)")
    return _PropagateRowsBF16.apply(h, graph, kind, n, bias)


def propagate_bf16(x, graph, kind):
    """P x with x rounded to bfloat16 for the gather (fp32 sums and output); any width: columns are zero-padded to a
    multiple of 8 here and sliced off again (autograd pads the gradient)."""
    _no_dist_bf16(graph)
    d = x.size(1)
    if d % 8 == 0:
        return propagate_rows_bf16(x, graph, kind)
    return propagate_rows_bf16(torch.nn.functional.pad(x, (0, (-d) % 8)), graph, kind)[:, :d]


def fused_linear_ok(graph, in_channels, out_channels, root=False, x=None):
    """The fused aggregate-then-transform kernel applies: supported widths, aggregating at the input width is
    not the more expensive order, and the graph is a single-GPU one — or a partitioned one asked to propagate its
    resident input features `x` (dist.DistGraph.pin_resident), which needs no exchange. `root`: with the
    SAGE-style root term x_i Wr^T accumulated in the same kernel."""
    if in_channels > out_channels:
        return False
    if _is_dist(graph):
        return x is not None and graph.fused_resident_ok(x, in_channels, out_channels, root)
    return bool(_lib.load().rgbx_spmm_linear_supported(in_channels, out_channels, int(root)))


_WEIGHTS_EPOCH = [0]


def note_weights_changed(*_args, **_kwargs):
    """Parameters may have been written without their Python-side version counters moving: a fused / foreach /
    capturable optimizer step (torch.optim.Adam(fused=True) writes through raw pointers), the replay of a captured
    hipGraph. Everything this package caches per parameter state (weight_t, ConvStack._eval_operands,
    dist.stack's folded operands) carries this counter in its key, so nothing made before the write is served after
    it. Registered below as a GLOBAL optimizer step post-hook: every torch.optim step of the process bumps it,
    whoever built the optimizer — a module of this package inside a foreign training loop needs no cooperation."""
    _WEIGHTS_EPOCH[0] += 1


def weights_epoch():
    return _WEIGHTS_EPOCH[0]


from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_post_hook  # noqa: E402

_register_step_post_hook(note_weights_changed)


class _MadeOn:
    """A device tensor kept for reuse, with the stream it was made on. Whoever takes it on ANOTHER stream first makes that
    stream wait for the making — the interleaved eval forwards of a multi-rank run (dist/runner.py, one HIP stream per
    forward, two host threads) share W^T copies, mask bitmaps and loss divisors: the forward that finds one cached must not
    launch on it before the other stream's transpose kernel has run. (Found by the first RCCL run with the ranks sharing a
    GPU, round 4: the replicate scheme's test loss, second forward, came out of the PREVIOUS step's W^T in the recycled block.)"""
    __slots__ = ("value", "stream", "event")

    def __init__(self, value):
        self.value, self.stream, self.event = value, None, None
        if value.is_cuda and not torch.cuda.is_current_stream_capturing():
            self.stream = torch.cuda.current_stream(value.device)
            self.event = torch.cuda.Event()
            self.event.record(self.stream)

    def get(self):
        if self.event is not None:
            cur = torch.cuda.current_stream(self.value.device)
            if cur != self.stream and not torch.cuda.is_current_stream_capturing():
                cur.wait_event(self.event)
                self.value.record_stream(cur)  # when the copy is replaced, its block is not handed out under this stream
        return self.value


def weight_t(weight):
    """W^T as the contiguous [K, Nout] operand rgbx_spmm_linear_f32 reads (its B fragments run along Nout). For an
    nn.Parameter the transposed copy is kept on the parameter and reused until the parameter may have changed: the
    in-place version counter, the storage address AND weights_epoch() (every optimizer step of the process, every
    hipGraph replay of epoch_graph) are its tag, instead of one `.t().contiguous()` per launch; temporaries (weights
    with a folded BatchNorm) and launches being captured into a hipGraph always transpose. Not seen: writes through
    `param.data` outside an optimizer (a fresh version counter by PyTorch's rules) — call note_weights_changed()."""
    w = weight.detach()
    if not isinstance(weight, torch.nn.Parameter) or (w.is_cuda and torch.cuda.is_current_stream_capturing()):
        return w.t().contiguous()
    tag = (weight._version, _WEIGHTS_EPOCH[0], w.data_ptr(), tuple(w.shape))
    cached = getattr(weight, "_rgbx_wt", None)
    if cached is None or cached[0] != tag:
        cached = (tag, _MadeOn(w.t().contiguous()))
        weight._rgbx_wt = cached
    return cached[1].get()


def _blocked(t, what):
    """(pointer, block columns, block stride) of a blocked matrix: a [B, n, cols] tensor whose blocks are contiguous
    [n, cols] matrices (views over the row range of a bigger one keep the block stride of their base)."""
    if (t.dtype != torch.float32 or t.dim() != 3 or (t.size(2) > 1 and t.stride(2) != 1)
            or (t.size(1) > 1 and t.stride(1) != t.size(2))):  # strides of size-1 dimensions mean nothing
        raise RuntimeError(f"{what}: expected a float32 [blocks, rows, cols] tensor with contiguous blocks, got "
                           f"{t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr(), t.size(2), t.stride(0)


def fused_layer(x, wt, csr=None, w=None, rs=None, bias=None, x_root=None, wt_root=None, pre=None, want_out=True,
                out_blocked=None, want_z=False, want_colsums=False, ce=None, kind="linear", out=None, z=None, w_pos=None,
                select_rows=False, col_sel=None, ce_fill=True):
    """One conv layer's arithmetic on rgbx_fused_layer_f32 (no autograd):
        z   = rs * sum_p w_p x[col_p]   over `csr`            (csr given: aggregate)
            = x                                                 (csr None: DENSE mode, the rows are loaded)
        z   = z * scale + shift * rowsum                        (`pre` = (scale [K], shift [K], rowsum [N]))
        out = z wt + bias (+ x_root' wt_root),  x_root' = x_root * scale + shift
    `x` is [n_src, K] row-major or, in DENSE mode, possibly BLOCKED ([B, N, K / B] — column slices as the exchange of
    a partitioned run delivers them); `x_root` likewise. `out_blocked` ([B', N, Nout / B'], optional): the output is
    (also) written there, in the layout the exchange sends from. `want_out=False`: no row-major output.
    `want_z`: the (mapped) aggregate is stored. `want_colsums`: [2, Nout] float64 column sums of out and out^2.
    `ce` = (y, mask, grad_scale): loss epilogue (see spmm_linear_raw). `out` / `z`: caller's row-major [N, Nout] /
    [N, K] tensors to write into (row ranges of bigger ones when a layer is launched piece by piece).
    `w_pos` (second weight vector over the same slots; implies want_z): z_pos = sum_p w_pos_p x[col_p] is stored as well
    and the return value is (out, (z, z_pos), colsums or stats).
    `select_rows` (one-GPU callers, with `ce`): only the rows the loss selects are gathered — a statistics-only launch
    runs over the cached list of those rows (selected_rows), and so does a loss-gradient launch (CE_GRAD_ROW_LIST; it
    skips the others in place where there is no list): the z and gradient rows of the others are 0 either way; see
    rgbx_ce_epilogue_t.rows / skip_unselected.
    `ce_fill=False` (with `select_rows` and a loss gradient): where the launch tiles the row list, the unlisted rows of
    out and z are left UNWRITTEN (rgbx_ce_epilogue_t.no_fill) — garbage, possibly NaN — instead of 0; for a caller whose
    every reader of the two walks that list or honours that selection. The other forms write what they always write.
    `col_sel` (uint8 [n_src] or None): slots whose column has a 0 there are not gathered (rgbx_fused_layer_t.col_sel).
    A vector that came from selected_cols is also carried in the column stream (col_tags, rgbx_fused_layer_t.col_tag).
    Returns (out, z, colsums or stats)."""
    _lib.require_device(x, wt, bias, x_root, wt_root, out_blocked, col_sel)
    L = _lib.FusedLayer()
    dense = csr is None
    if x.dim() == 3:
        if not dense:
            raise RuntimeError("fused_layer: a blocked x needs DENSE mode (no csr)")
        L.x, L.x_blk_cols, L.x_blk_stride = _blocked(x, "x")
        n_rows, K = x.size(1), x.size(0) * x.size(2)
    else:
        x = x if x.stride(-1) == 1 else x.contiguous()
        L.x, L.ldx = x.data_ptr(), x.stride(0) if x.size(0) > 1 else x.size(1)
        n_rows, K = x.size(0), x.size(1)
    N = n_rows if dense else csr.N
    wt = wt.contiguous()
    n_out = wt.size(1)
    if wt.size(0) != K:
        raise RuntimeError(f"fused_layer: wt is {tuple(wt.shape)}, the input width is {K}")
    keep = [x, wt]
    L.wt = wt.data_ptr()
    if not dense:
        L.rowptr, L.col, L.w, L.rs = _lib.ptr(csr.rowptr), _lib.ptr(csr.col), _lib.ptr(w), _lib.ptr(rs)
        if col_sel is not None:
            if col_sel.dtype != torch.uint8 or col_sel.numel() < x.size(0):
                raise RuntimeError(f"fused_layer: col_sel must be uint8 with an entry per input row, got {col_sel.dtype} "
                                   f"{tuple(col_sel.shape)} for {x.size(0)} rows")
            tag = col_tags(csr, col_sel)  # a selection of selected_cols: carried in the column stream (None: looked up)
            col_sel = col_sel.contiguous()
            keep.append(col_sel)
            L.col_sel = col_sel.data_ptr()
            if tag is not None:
                keep.append(tag)
                L.col_tag = tag.data_ptr()
        split, _scratch = csr.split_arg(K, x.device, hub_rows=2 if w_pos is not None else 1)
        keep.append(_scratch)
        if split is not None:
            keep.append(split)
            L.split = ctypes.addressof(split)
    if wt_root is not None:
        wtr = wt_root.contiguous()
        keep.append(wtr)
        L.wt_root = wtr.data_ptr()
        if x_root.dim() == 3:
            L.x_root, L.xr_blk_cols, L.xr_blk_stride = _blocked(x_root, "x_root")
        else:
            xr = x_root if x_root.stride(-1) == 1 else x_root.contiguous()
            keep.append(xr)
            L.x_root, L.ldr = xr.data_ptr(), xr.stride(0) if xr.size(0) > 1 else xr.size(1)
    if bias is not None:
        b = bias.contiguous()
        keep.append(b)
        L.bias = b.data_ptr()
    if pre is not None:
        ps, pt, pr = (t.contiguous() for t in pre)
        keep += [ps, pt, pr]
        L.pre_scale, L.pre_shift, L.pre_rowsum = ps.data_ptr(), pt.data_ptr(), pr.data_ptr()
    ce_stats = None
    groups = 1
    if ce is not None:
        y, mask, grad_scale = ce
        if isinstance(mask, (tuple, list)):  # two masks, one forward: statistics set 0 / 1 = bit 0 / 1 of the grouped mask
            if grad_scale is not None:
                raise RuntimeError("fused_layer: two masks are for statistics only (no loss gradient)")
            mask, groups = group_masks(*mask), 2
        _lib.require_device(y, mask, grad_scale)
        if y.dtype != torch.int64:
            raise RuntimeError(f"labels must be int64, got {y.dtype}")
        if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
            raise RuntimeError(f"mask must be bool, got {mask.dtype}")
        y = y.contiguous()
        mask = None if mask is None else mask.contiguous()
        ce_stats = torch.empty(3 * groups, dtype=torch.float64, device=x.device)
        scratch_doubles = 3 * groups * ((N + 31) // 32 + 64)
        rows = None
        if select_rows and not dense and w_pos is None and mask is not None:
            if grad_scale is not None:
                # the gradient form tiles the list too (CE_GRAD_ROW_LIST), where the 16-byte zero fill of the unlisted
                # rows applies; without a list (inside a capture before it exists) or with an empty one: the in-place skip
                if CE_GRAD_ROW_LIST and (out is None or (out.data_ptr() % 16 == 0 and (N == 1 or out.stride(0) % 4 == 0))):
                    rows = selected_rows(y, mask, n_out)
                    if rows is not None and rows.numel() == 0:
                        rows = None
            elif not want_z and z is None:
                rows = selected_rows(y, mask, n_out)  # None: inside a graph capture before the list exists (all tiles)
        if rows is not None and grad_scale is not None:
            count = ctypes.c_int64(0)
            _lib.call("rgbx_ce_rows_grad_scratch_doubles", N, ctypes.byref(count))
            scratch_doubles = count.value
        ce_scratch = torch.empty(scratch_doubles, dtype=torch.float64, device=x.device)
        ce_arg = _lib.CeEpilogue(_lib.ptr(y), _lib.ptr(mask), _lib.ptr(grad_scale), _lib.ptr(ce_stats),
                                 _lib.ptr(ce_scratch), groups)
        if rows is not None:
            ce_arg.rows, ce_arg.n_rows = rows.data_ptr(), rows.numel()
            ce_arg.no_fill = int(not ce_fill and grad_scale is not None)
            keep.append(rows)
        elif select_rows and not dense and w_pos is None and grad_scale is not None:
            ce_arg.skip_unselected = 1
        keep += [y, mask, ce_scratch, ce_arg]
        L.ce = ctypes.addressof(ce_arg)
        want_out = grad_scale is not None  # statistics only: the logits are never written
    if out is not None:
        if tuple(out.shape) != (N, n_out) or out.stride(1) != 1 or out.dtype != torch.float32:
            raise RuntimeError(f"fused_layer: out is {tuple(out.shape)}, expected a float32 [{N}, {n_out}] with contiguous rows")
    elif want_out:
        out = torch.empty((N, n_out), dtype=torch.float32, device=x.device)
    if out is not None:
        L.out, L.ldo = out.data_ptr(), out.stride(0) if N > 1 else n_out
    else:
        L.ldo = n_out
    if out_blocked is not None:
        L.out_blk, L.ob_cols, L.ob_stride = _blocked(out_blocked, "out_blocked")
        if out_blocked.size(1) != N or out_blocked.size(0) * out_blocked.size(2) != n_out:
            raise RuntimeError(f"fused_layer: out_blocked is {tuple(out_blocked.shape)} for a [{N}, {n_out}] output")
    if z is not None:
        if tuple(z.shape) != (N, K) or z.stride(1) != 1 or z.dtype != torch.float32:
            raise RuntimeError(f"fused_layer: z is {tuple(z.shape)}, expected a float32 [{N}, {K}] with contiguous rows")
    elif want_z or w_pos is not None:
        z = torch.empty((N, K), dtype=torch.float32, device=x.device)
    L.ldz = K
    if z is not None:
        L.z_out, L.ldz = z.data_ptr(), z.stride(0) if N > 1 else K
    z_pos = None
    if w_pos is not None:
        _lib.require_device(w_pos)
        z_pos = torch.empty_strided((N, K), (L.ldz, 1), dtype=torch.float32, device=x.device)
        keep.append(w_pos)
        L.w_pos, L.z_pos_out = w_pos.data_ptr(), z_pos.data_ptr()
    colsums = None
    if want_colsums:
        nbytes = ctypes.c_size_t(0)
        _lib.call("rgbx_spmm_linear_stats_workspace_bytes", N, n_out, ctypes.byref(nbytes))
        ws = torch.empty(max(nbytes.value, 8), dtype=torch.uint8, device=x.device)
        colsums = torch.empty((2, n_out), dtype=torch.float64, device=x.device)
        keep.append(ws)
        L.out_colsums, L.stats_ws, L.stats_ws_bytes = colsums.data_ptr(), ws.data_ptr(), nbytes.value
    L.N, L.K, L.Nout = N, K, n_out
    variant = None
    if _EVENT_SINK is not None:  # which form this launch is (bench.py's per-variant table)
        variant = "+".join([name for name, on in (
            ("dense", dense), ("pre", pre is not None), ("root", wt_root is not None), ("z", z is not None),
            ("zpos", w_pos is not None), ("stats", want_colsums), ("ce_stats", ce is not None and ce[2] is None),
            ("ce_grad", ce is not None and ce[2] is not None), ("noout", out is None and out_blocked is None and ce is None),
            ("blk", out_blocked is not None)) if on]) or "plain"
    _launch(kind, "rgbx_fused_layer_f32", L, variant=variant)
    del keep
    if groups == 2:
        ce_stats = ce_stats.view(2, 3)  # row k = [nll sum, selected rows, correct] under mask k
    return out, (z if w_pos is None else (z, z_pos)), (ce_stats if ce is not None else colsums)


def blocked_to_rows(src, out=None, bias=None):
    """[B, n, cols] blocked -> [n, B * cols] row-major (+ bias per column) (rgbx_blocked_to_rows_f32)."""
    _lib.require_device(src, bias)
    ptr, bc, bs = _blocked(src, "src")
    n, d = src.size(1), src.size(0) * src.size(2)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=src.device)
    b = None if bias is None else bias.detach().contiguous()
    _lib.launch("rgbx_blocked_to_rows_f32", ptr, bc, bs, out, out.stride(0), n, d, b)
    return out


def spmm_linear_raw(csr, w, rs, x, wt, bias=None, want_z=False, x_root=None, wt_root=None, kind="linear", pre=None,
                    want_colsums=False, ce=None, select_rows=False, ce_fill=True):
    """out = (rs * sum_p w_p x[col_p]) wt + bias (+ x_root wt_root) on the fused aggregate+transform kernel; `wt` /
    `wt_root` are [K, Nout] row-major. Returns (out, z) with z the stored aggregate [N, K] if `want_z`. `pre` = (scale
    [K], shift [K], rowsum [N]): the gathered matrix (and the root rows) stand for x * scale + shift. `want_colsums`:
    returns (out, z, colsums) with colsums [2, Nout] float64 = column sums of out and out^2 from the MFMA tiles.
    `ce` = (y, mask, grad_scale): the layer is the model's last and its logits go straight into the masked
    cross-entropy (rgbx_ce_epilogue_t): returns (out, z, stats) with stats [3] float64 = (nll sum, selected rows,
    correct); out = the loss gradient grad_scale * (softmax - onehot) when grad_scale is a device scalar, None (nothing
    written) when it is None. `select_rows`, `ce_fill`: see fused_layer."""
    out, z, extra = fused_layer(x, wt, csr=csr, w=w, rs=rs, bias=bias, x_root=x_root if wt_root is not None else None,
                                wt_root=wt_root, pre=pre, want_z=want_z, want_colsums=want_colsums, ce=ce, kind=kind,
                                select_rows=select_rows, ce_fill=ce_fill)
    if ce is not None or want_colsums:
        return out, z, extra
    return out, z


class _AggregateLinear(torch.autograd.Function):
    """y = z W^T + b (+ x_root Wr^T) for an aggregate z = P x that was formed earlier and is kept (the opt-in
    cache of the static input features' aggregate, models/_stack.ConvStack.cache_input_aggregate): the DENSE form of
    rgbx_fused_layer_f32. z and x_root take no gradient (they are functions of the input features only);
    dW = dy^T z, db = column sums of dy, dWr = dy^T x_root."""

    @staticmethod
    def forward(ctx, z, weight, bias, root_weight, x_root, want_colsums):
        out, _, cs = fused_layer(z, weight_t(weight), bias=None if bias is None else bias.detach(),
                                 x_root=x_root if root_weight is not None else None,
                                 wt_root=None if root_weight is None else weight_t(root_weight),
                                 want_colsums=want_colsums, kind="cached_aggregate_linear_fwd")
        ctx.save_for_backward(z, x_root if root_weight is not None else None)
        ctx.has_bias = bias is not None
        if want_colsums:
            ctx.mark_non_differentiable(cs)
            return out, cs
        return out

    @staticmethod
    def backward(ctx, gy, _g_cs=None):
        z, x_root = ctx.saved_tensors
        gy = gy.contiguous()
        gw = gb = gwr = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            if want_b:
                gw, gb = gemm_tn(gy, z, colsum=True)
            else:
                gw = gemm_tn(gy, z)
        elif want_b:
            gb = gy.sum(0)
        if x_root is not None and ctx.needs_input_grad[3]:
            gwr = gemm_tn(gy, x_root)
        return None, gw, gb, gwr, None, None


def aggregate_linear_ok(in_channels, out_channels, root=False):
    return bool(_lib.load().rgbx_spmm_linear_supported(in_channels, out_channels, int(root)))


def aggregate_linear(z, weight, bias=None, root_weight=None, x_root=None, want_colsums=False):
    """Transform of a kept aggregate (see _AggregateLinear); the caller checked aggregate_linear_ok."""
    return _tag_colsums(_AggregateLinear.apply(z, weight, bias, root_weight, x_root, want_colsums), want_colsums)


def fold_bn_linear(weight, bias=None, bias2=None, root_weight=None, bn=None):
    """(W'^T [K, Nout], b' [Nout] or None, Wr'^T or None): the operands rgbx_fused_layer_f32 reads for a linear layer
    with the eval-mode BatchNorm1d `bn` behind it folded in (bn None: the plain transposes), in ONE launch
    (rgbx_fold_bn_linear_f32). No autograd: eval forwards only."""
    _lib.require_device(weight, bias, bias2, root_weight)
    W = weight.detach()
    W = W if W.stride(-1) == 1 else W.contiguous()
    n_out, K = W.shape
    Wr = None
    if root_weight is not None:
        Wr = root_weight.detach()
        Wr = Wr if Wr.stride(-1) == 1 else Wr.contiguous()
    wt = torch.empty((K, n_out), dtype=torch.float32, device=W.device)
    wrt = torch.empty_like(wt) if Wr is not None else None
    has_b = bias is not None or bias2 is not None or bn is not None
    b_out = torch.empty(n_out, dtype=torch.float32, device=W.device) if has_b else None
    c = lambda t: None if t is None else t.detach().contiguous()
    b1, b2 = c(bias), c(bias2)
    g = be = rm = rv = None
    eps = 0.0
    if bn is not None:
        g, be, rm, rv, eps = c(bn.weight), c(bn.bias), c(bn.running_mean), c(bn.running_var), bn.eps
    _lib.launch("rgbx_fold_bn_linear_f32", W, W.stride(0), Wr, 0 if Wr is None else Wr.stride(0), b1, b2, g, be, rm, rv,
                float(eps), wt, wrt, b_out, n_out, K)
    return wt, b_out, wrt


# The dense tail of the backward, one switch for both forms (tests, A/B runs; False = the launches as they were):
#  - the conv that feeds a training-mode BatchNorm owns that BatchNorm's backward (BNHandover) and forms the input
#    gradient inside its weight-gradient GEMM (gemm_tn_bn_bwd) instead of reading back a written one;
#  - the last conv's weight gradient runs over the rows the loss selects (gemm_tn_rows).
# Either way every result is the same, bit for bit.
FUSE_DENSE_BACKWARD = True
# The training form of the last layer (loss gradient, select_rows) tiles the list of the selected rows instead of keeping
# every tile and skipping the deselected rows in place (rgbx_ce_epilogue_t.rows with grad_scale): the same gradient,
# aggregate and statistics, bit for bit. False = the in-place skip (skip_unselected), for tests and A/B runs.
CE_GRAD_ROW_LIST = True

BN_HANDOVER = "_rgbx_bn_handover"  # attribute of a conv output whose node owns the backward of the BatchNorm behind it


class BNHandover:
    """Plain record between the node of a conv (`_PropagateLinear`, the producer) and the node of the conv that takes the
    producer's output through a training-mode BatchNorm `bn` without writing BN(.) (`_BNPropagateLinear` /
    `_PropagateLinearCE`, the consumer). The producer's output tensor then STANDS FOR the BatchNorm's output in the
    autograd graph: the consumer returns g_h, the true gradient of BN's output, for it, and nothing for bn.weight /
    bn.bias; the producer, which has them as inputs, runs BatchNorm's backward on g_h and its own output. The consumer's
    forward fills in what that needs of the statistics — constants only (mean, rstd, row count, the reduction over
    ranks). A record nobody filled (the consumer took another route) leaves the producer's backward as it was."""
    __slots__ = ("bn", "mean", "rstd", "n", "reduce")

    def __init__(self, bn):
        self.bn, self.mean, self.rstd, self.n, self.reduce = bn, None, None, None, None

    def fill(self, mean, rstd, n, reduce):
        self.mean, self.rstd, self.n, self.reduce = mean, rstd, n, reduce


def _take_handover(x, bn):
    """The unfilled BNHandover riding on `x` for this `bn`, if x's node will run (it returns bn's gradients)."""
    rec = getattr(x, BN_HANDOVER, None)
    if rec is None or rec.bn is not bn or rec.mean is not None or not x.requires_grad or not FUSE_DENSE_BACKWARD:
        return None
    return rec


class _PropagateLinear(torch.autograd.Function):
    """y = (P x) W^T + b (+ x Wr^T) with P = A_hat ('gcn'), the mean operator ('mean') or the plain edge sum ('sum'), in one launch
    (rgbx_spmm_linear_f32). Backward: dW = dy^T (P x) on the split-K MFMA kernel (P x was stored by the
    forward when a gradient is needed), db = column sums from the same pass, dWr = dy^T x, and — only if x
    needs a gradient — dx = P^T (dy W) + dy Wr = (P^T dy) W + dy Wr: the SAME fused kernel on the transposed CSR
    (W as stored is already the [K, Nout] operand) when in == out, else GEMMs and the transposed SpMM with the
    root part as its additive term."""

    @staticmethod
    def forward(ctx, x, graph, kind, weight, bias, need_z=True, root_weight=None, x_root=None, want_colsums=False,
                bn_weight=None, bn_bias=None, handover=None):
        """`x_root`: the targets' own rows when they are not simply the first rows of `x` viewed as a separate
        tensor (partitioned graph: x = [local; halo], x_root = local). `want_colsums`: returns (out, colsums).
        `handover` (BNHandover, with the parameters of its BatchNorm as `bn_weight` / `bn_bias`): this node owns the
        backward of the training-mode BatchNorm behind it, once the consumer has filled the record."""
        x = x.contiguous()
        xr = x if x_root is None else x_root.contiguous()
        w = graph.w if kind == "gcn" else None          # properties: each builds its vector on first use only
        rs = graph.inv_deg if kind == "mean" else None  # ('sum': neither)
        if kind not in ("gcn", "mean", "sum"):
            raise ValueError(kind)
        res = spmm_linear_raw(graph.fwd, w, rs, x, weight_t(weight), None if bias is None else bias.detach(),
                              need_z, xr if root_weight is not None else None,
                              None if root_weight is None else weight_t(root_weight),
                              kind=f"{getattr(graph, 'event_prefix', '')}{kind}_linear_fwd", want_colsums=want_colsums)
        out, z = res[0], res[1]
        ctx.save_for_backward(z, weight, root_weight, xr if root_weight is not None else None,
                              bn_weight if handover is not None else None, out if handover is not None else None)
        ctx.graph, ctx.kind, ctx.has_bias, ctx.handover = graph, kind, bias is not None, handover
        if want_colsums:
            ctx.mark_non_differentiable(res[2])
            return out, res[2]
        return out

    @staticmethod
    def backward(ctx, gy, _g_colsums=None):
        z, weight, root_weight, x, bn_weight, y = ctx.saved_tensors
        g, kind = ctx.graph, ctx.kind
        gy = gy.contiguous()
        gx = gw = gb = gwr = g_bnw = g_bnb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[4]
        rec, bn_a = ctx.handover, None
        if rec is not None and rec.mean is not None:
            # gy is g_h, the gradient of BN(y): BatchNorm's backward runs here — its column sums and coefficients as ever,
            # its apply pass inside the dW GEMM unless something else reads gx too (dx, dWr, a bias gradient on its own)
            from .nn import batchnorm as B
            ca, cb, ck, g_bnw, g_bnb = B.train_backward_coefficients(gy, y, bn_weight, rec.mean, rec.rstd, rec.n,
                                                                     rec.reduce)
            if (ctx.needs_input_grad[0] or (root_weight is not None and ctx.needs_input_grad[6])
                    or not ctx.needs_input_grad[3]):
                gy = B.bwd_apply(gy, y, rec.mean, rec.rstd, ca, cb, ck)
            else:
                bn_a = (y, rec.mean, rec.rstd, ca, cb, ck)
        if bn_a is not None:
            gw, gb = gemm_tn_bn_bwd(gy, *bn_a, z, colsum=want_b)
        elif ctx.needs_input_grad[3]:
            if want_b:
                gw, gb = gemm_tn(gy, z, colsum=True)  # dy is read once for dW and db
            else:
                gw = gemm_tn(gy, z)
        elif want_b:
            gb = gy.sum(0)
        if root_weight is not None and ctx.needs_input_grad[6]:
            gwr = gemm_tn(gy, x)
        if ctx.needs_input_grad[0]:
            gx = _propagate_linear_input_grad(g, kind, gy, weight, root_weight)
        return gx, None, None, gw, gb, None, gwr, None, None, g_bnw, g_bnb, None


def _input_grad_is_fused(weight, root_weight):
    """The transposed launch of a conv with this weight runs on the fused kernel (_propagate_linear_input_grad)."""
    n_out, n_in = weight.shape
    return n_out <= n_in and bool(_lib.load().rgbx_spmm_linear_supported(n_out, n_in, int(root_weight is not None)))


def _input_grad_skips_deselected(g, weight, root_weight):
    """Every slot the transposed launch gathers of dy is a selected one when it is given a col_sel: the fused kernel takes
    the launch and honours col_sel there (rgbx_fused_layer_t.col_sel: K = the weight's rows in {64, 128, 256}, Nout = its
    columns <= 128), and the transposed CSR has no hub rows, which gather every slot."""
    n_out, n_in = weight.shape
    return (_input_grad_is_fused(weight, root_weight) and n_out in (64, 128, 256) and n_in <= 128
            and g.bwd.split is None)


def _propagate_linear_input_grad(g, kind, gy, weight, root_weight, ce_sel=None, sparse_gy=False):
    """dx = P^T (dy W) + dy Wr = (P^T dy) W + dy Wr: the fused kernel on the transposed CSR (W as stored is already
    the [K, Nout] operand) when in == out, else GEMMs and the transposed SpMM with the root part as its additive
    term. `ce_sel` = (y, mask, C): dy is the loss gradient of the masked cross-entropy, zero outside the rows that loss
    selects; the fused kernel then does not gather those rows (selected_cols; every slot keeps its place in the sum, so
    the result is the full gather's, bit for bit). `sparse_gy`: those rows of dy were never written (the forward ran with
    ce_fill=False) and MUST not be read: any route that would read them raises."""
    csr = g.bwd
    wt = {"gcn": lambda: g.w_t, "mean": lambda: g.w_mean_t, "sum": lambda: None}[kind]()
    prefix = getattr(g, "event_prefix", "")
    col_sel = None if ce_sel is None else selected_cols(*ce_sel)
    if sparse_gy and (col_sel is None or not _input_grad_skips_deselected(g, weight, root_weight)):
        raise RuntimeError("propagate_linear_ce: the loss gradient was stored without its zero rows, and the transposed "
                           "launch can no longer skip them (the column selection or the fused route is gone)")
    if _input_grad_is_fused(weight, root_weight):
        gx, _, _ = fused_layer(gy, weight.detach().contiguous(), csr=csr, w=wt,
                               x_root=gy if root_weight is not None else None,
                               wt_root=None if root_weight is None else root_weight.detach().contiguous(),
                               col_sel=col_sel, kind=f"{prefix}{kind}_linear_bwd")
        return gx
    gz = gy @ weight
    gr = gy @ root_weight if root_weight is not None else None
    if gr is None:
        return spmm_raw(csr, wt, None, gz, kind=f"{prefix}{kind}_bwd")
    return spmm_raw(csr, wt, None, gz, y=gr, a=1.0, b=1.0, out=gr, kind=f"{prefix}{kind}_bwd")


class _BNPropagateLinear(torch.autograd.Function):
    """y = (P BN(x)) W^T + b (+ BN(x) Wr^T) for a TRAINING-mode BatchNorm1d in front of a conv layer
    (models/gcn.py:28-29: x = bns[i](x); x = convs[i+1](x, edge_index)) without writing BN(x): the statistics pass
    gives BN(x) = x * s + t per column, and rgbx_spmm_linear_f32 gathers the RAW rows and maps the aggregate,
    s * (P x) + t * rowsum(P) (linearity of the aggregation), before the MFMA transform.
    Backward = the two layers' own backward passes one after the other, unchanged: dW = dy^T z (z = the mapped
    aggregate the forward stored), the gradient g_h of the BatchNorm output from the fused kernel on the transposed
    CSR, then BatchNorm's backward (column sums of g_h and g_h * xhat, apply)."""

    @staticmethod
    def forward(ctx, x, bn_weight, bn_bias, graph, kind, weight, bias, root_weight, eps, reduce, running, need_z,
                colsums=None, want_colsums=False, handover=None):
        """`handover` (BNHandover): x's node owns BatchNorm's backward; x then stands for BN(x) in the graph and this
        node's backward returns g_h for it."""
        from .nn import batchnorm as B
        x = x.contiguous()
        mean, rstd, scale, shift, n = B.train_statistics(x, bn_weight, bn_bias, eps, reduce, running, colsums)
        if handover is not None:
            handover.fill(mean, rstd, n, reduce)
        ctx.handed_over = handover is not None
        w, rs = (graph.w, None) if kind == "gcn" else (None, graph.inv_deg)
        res = spmm_linear_raw(graph.fwd, w, rs, x, weight_t(weight), None if bias is None else bias.detach(), need_z,
                              x if root_weight is not None else None,
                              None if root_weight is None else weight_t(root_weight), kind=f"{kind}_linear_fwd",
                              pre=(scale, shift, graph.rowsum(kind)), want_colsums=want_colsums)
        out, z = res[0], res[1]
        ctx.save_for_backward(x, bn_weight, mean, rstd, n, z, weight, root_weight, scale, shift)
        ctx.graph, ctx.kind, ctx.has_bias, ctx.reduce = graph, kind, bias is not None, reduce
        if want_colsums:
            ctx.mark_non_differentiable(res[2])
            return out, res[2]
        return out

    @staticmethod
    def backward(ctx, gy, _g_colsums=None):
        from .nn import batchnorm as B
        x, bn_weight, mean, rstd, n, z, weight, root_weight, scale, shift = ctx.saved_tensors
        g, kind = ctx.graph, ctx.kind
        gy = gy.contiguous()
        gw = gb = gwr = None
        if ctx.needs_input_grad[5]:
            gw, gcol = gemm_tn(gy, z, colsum=True)  # dy is read once for dW and the column sums
            gb = gcol if ctx.has_bias and ctx.needs_input_grad[6] else None
        else:
            gcol = gy.sum(0)
            gb = gcol if ctx.has_bias and ctx.needs_input_grad[6] else None
        if root_weight is not None and ctx.needs_input_grad[7]:
            # dWr = dy^T BN(x) = (dy^T x) diag(s) + colsum(dy) t^T
            gwr = gemm_tn(gy, x) * scale + gcol[:, None] * shift
        g_h = _propagate_linear_input_grad(g, kind, gy, weight, root_weight)
        if ctx.handed_over:
            return g_h, None, None, None, None, gw, gb, gwr, None, None, None, None, None, None, None
        gx, g_bnw, g_bnb = B.train_backward(g_h, x, bn_weight, mean, rstd, n, ctx.reduce)
        return gx, g_bnw, g_bnb, None, None, gw, gb, gwr, None, None, None, None, None, None, None


_SCALE_CACHE = {}


def mask_scale(y, mask, C):
    """Device scalar 1 / (number of rows the masked cross-entropy selects): rows with mask set (all if None) and a
    label in [0, C). A mask is fixed for a run, so the count is taken once per (labels, mask) pair — the fused loss
    epilogue needs the mean's divisor BEFORE the launch that produces the logits."""
    key = (y.data_ptr(), y._version, y.numel(), None if mask is None else (mask.data_ptr(), mask._version), int(C))
    hit = _SCALE_CACHE.get(key)
    if hit is None:
        sel = (y >= 0) & (y < C)
        if mask is not None:
            sel = sel & mask.bool()
        hit = (_MadeOn((1.0 / sel.sum().double()).float().reshape(1)), y, mask)  # the tensors stay alive with their addresses
        _SCALE_CACHE[key] = hit
        while len(_SCALE_CACHE) > 32:
            _SCALE_CACHE.pop(next(iter(_SCALE_CACHE)))
    return hit[0].get()


_GROUP_MASKS = {}


def group_masks(mask_a, mask_b):
    """uint8 [N] with bit 0 = mask_a, bit 1 = mask_b (rgbx_ce_epilogue_t.mask_groups == 2): made once per pair of mask
    tensors (address + version), masks are fixed for a run."""
    _lib.require_device(mask_a, mask_b)
    key = (mask_a.data_ptr(), mask_a._version, mask_b.data_ptr(), mask_b._version, mask_a.numel())
    hit = _GROUP_MASKS.get(key)
    if hit is None:
        g = (mask_a.bool().to(torch.uint8) | (mask_b.bool().to(torch.uint8) << 1)).contiguous()
        hit = (_MadeOn(g), mask_a, mask_b)  # the mask tensors stay alive with their addresses
        _GROUP_MASKS[key] = hit
        while len(_GROUP_MASKS) > 16:
            _GROUP_MASKS.pop(next(iter(_GROUP_MASKS)))
    return hit[0].get()


def ce_selection(y, mask, C):
    """bool [N]: the rows the masked cross-entropy selects — mask bit(s) set (either of the two of a grouped mask) AND a
    label in [0, C). The loss epilogue's own predicate (spmm_linear.hip, ce_select), restated for the row list of the
    statistics-only form (selected_rows) and the column selection of the backward's transposed gather (selected_cols)."""
    sel = (y >= 0) & (y < C)
    if mask is not None:
        sel = sel & mask.bool()
    return sel


def _sel_key(y, mask, C):
    return (y.data_ptr(), y._version, y.numel(),
            None if mask is None else (mask.data_ptr(), mask._version, mask.numel()), int(C))


_SEL_ROWS = {}


def selected_rows(y, mask, C):
    """int32 device list (ascending) of the rows ce_selection picks: the tiles of a statistics-only loss launch
    (rgbx_ce_epilogue_t.rows). Built once per (labels, mask, C) — keyed on address, in-place version and size, so an
    edited mask gets a new list — with the one host read of `nonzero`; None inside a graph capture where the list does
    not exist yet (the caller then runs every tile)."""
    key = _sel_key(y, mask, C)
    hit = _SEL_ROWS.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        rows = ce_selection(y, mask, C).nonzero().reshape(-1).to(torch.int32).contiguous()
        hit = (_MadeOn(rows), y, mask)  # the tensors stay alive with their addresses
        _SEL_ROWS[key] = hit
        while len(_SEL_ROWS) > 16:
            _SEL_ROWS.pop(next(iter(_SEL_ROWS)))
    return hit[0].get()


_SEL_COLS = {}


def selected_cols(y, mask, C):
    """uint8 device vector of ce_selection: the column selection (rgbx_fused_layer_t.col_sel) of the transposed gather of
    a loss gradient that is zero on every row the loss does not select. Built once per (labels, mask, C), keyed as
    selected_rows; None inside a graph capture where it does not exist yet (every slot gathered, same result)."""
    key = _sel_key(y, mask, C)
    hit = _SEL_COLS.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        hit = (_MadeOn(ce_selection(y, mask, C).to(torch.uint8).contiguous()), y, mask)
        _SEL_COLS[key] = hit
        while len(_SEL_COLS) > 16:
            _SEL_COLS.pop(next(iter(_SEL_COLS)))
    return hit[0].get()


_COL_TAGS = {}


def col_tags(csr, col_sel):
    """int32 [nnz] device vector col_sel[col[p]] ? col[p] : ~col[p] (rgbx_col_tag_i32) for a `col_sel` that selected_cols
    handed out: the selection carried in the column stream of the transposed gather (rgbx_fused_layer_t.col_tag), so that
    the launch has no per-slot look-up in col_sel. Built once per (the CSR's `col`, selection key) and kept with the
    tensors it was keyed on, like _SEL_COLS; two entries at most, each 4 * nnz bytes (248 MB at workload L: a run has one
    training graph and one mask). None — the launch then looks col_sel up per slot, the same result — for any other
    vector, for an empty CSR, and inside a graph capture where the array does not exist yet."""
    key = next((k for k, hit in _SEL_COLS.items() if hit[0].value is col_sel), None)
    if key is None or csr.nnz <= 0:
        return None
    key = (csr.col.data_ptr(), csr.nnz, key)
    hit = _COL_TAGS.get(key)
    if hit is None or hit[2] is not col_sel:  # (a selection evicted from _SEL_COLS and made again is a new vector)
        if torch.cuda.is_current_stream_capturing():
            return None
        tag = torch.empty(csr.nnz, dtype=torch.int32, device=csr.col.device)
        _lib.launch("rgbx_col_tag_i32", csr.col, col_sel, csr.nnz, col_sel.numel(), tag)
        hit = (_MadeOn(tag), csr.col, col_sel)  # the tensors stay alive with their addresses
        _COL_TAGS[key] = hit
        while len(_COL_TAGS) > 2:
            _COL_TAGS.pop(next(iter(_COL_TAGS)))
    return hit[0].get()


def ce_from_logits(logits, y, mask):
    """(loss, stats) of the masked cross-entropy taken from materialised logits: the unfused route of the *_ce
    entry points. loss = NLLLoss(log_softmax(logits)[mask], y[mask]); stats = [nll sum, selected rows, correct].
    `mask` = (mask_a, mask_b): (None, [2, 3] stats) of both masks from the one set of logits."""
    if isinstance(mask, (tuple, list)):
        return None, torch.stack([masked_ce_accuracy(logits, y, m) for m in mask])
    if torch.is_grad_enabled() and logits.requires_grad:
        return masked_ce_loss(logits, y, mask, with_stats=True)
    stats = masked_ce_accuracy(logits, y, mask)
    return (stats[0] / stats[1]).float(), stats


def fused_ce_ok(graph, in_channels, out_channels, root, x, y):
    """The model's last conv can take the loss into its kernel: fused aggregate+transform applies, at most 128
    classes, single-GPU graph, device labels."""
    return (not _is_dist(graph) and out_channels <= 128 and y is not None and y.is_cuda and y.dtype == torch.int64
            and fused_linear_ok(graph, in_channels, out_channels, root=root, x=x))


class _PropagateLinearCE(torch.autograd.Function):
    """loss = masked cross-entropy of ((P x') W^T + b (+ x' Wr^T)) with x' = BN(x) (training BatchNorm handed over as
    in _BNPropagateLinear) or x itself — the model's last conv with the loss taken inside the kernel
    (rgbx_ce_epilogue_t): the logits are never written. A forward that prepares a backward stores the loss gradient
    w.r.t. the logits instead (scaled by 1 / selected rows); the backward is then _PropagateLinear's / _BNPropagateLinear's
    with that matrix as dy and the incoming scalar folded into the small operands (W, Wr, dW, db)."""

    @staticmethod
    def forward(ctx, x, graph, kind, weight, bias, root_weight, y, mask, want_grad, bn_weight, bn_bias, bn_args):
        from .nn import batchnorm as B
        x = x.contiguous()
        pre = None
        if bn_weight is not None:
            eps, reduce, running, colsums, handover = bn_args
            mean, rstd, scale, shift, n = B.train_statistics(x, bn_weight, bn_bias, eps, reduce, running, colsums)
            pre = (scale, shift, graph.rowsum(kind))
            if handover is not None:  # x's node owns BatchNorm's backward (BNHandover): the backward returns g_h for x
                handover.fill(mean, rstd, n, reduce)
        ctx.handed_over = bn_weight is not None and bn_args[4] is not None
        w, rs = (graph.w, None) if kind == "gcn" else (None, graph.inv_deg)
        grad_scale = mask_scale(y, mask, weight.size(0)) if want_grad else None
        # The zero rows of dlogits and z (0.8 GB per step at workload L) are written only where somebody reads them. Nobody
        # does when every reader in this node's backward is driven by the row list or the selection: dW / db walk the list
        # (gemm_tn_rows: the weight wants a gradient, FUSE_DENSE_BACKWARD), there is no root weight (its dWr = dy^T x and
        # root term read every row of dy), and the transposed launch, if one will run, skips the deselected slots
        # (_input_grad_skips_deselected) with a selection that exists now. Neither tensor leaves this Function.
        need_h = ctx.needs_input_grad[0] or (bn_weight is not None and (ctx.needs_input_grad[9] or ctx.needs_input_grad[10]))
        ce_sel = (y, mask, weight.size(0))
        no_fill = bool(want_grad and CE_GRAD_ROW_LIST and FUSE_DENSE_BACKWARD and root_weight is None and mask is not None
                       and ctx.needs_input_grad[3] and selected_rows(*ce_sel) is not None
                       and selected_rows(*ce_sel).numel() > 0
                       and (not need_h or (selected_cols(*ce_sel) is not None
                                           and _input_grad_skips_deselected(graph, weight, None))))
        ctx.ce_no_fill = no_fill  # the backward holds itself to it
        dlogits, z, stats = spmm_linear_raw(
            graph.fwd, w, rs, x, weight_t(weight), None if bias is None else bias.detach(),
            want_grad and weight.requires_grad, x if root_weight is not None else None,
            None if root_weight is None else weight_t(root_weight), kind=f"{kind}_linear_fwd", pre=pre,
            ce=(y, mask, grad_scale), select_rows=True, ce_fill=not no_fill)
        ctx.graph, ctx.kind, ctx.has_bias, ctx.has_bn = graph, kind, bias is not None, bn_weight is not None
        # the saved dy is the loss gradient: zero outside the selected rows, so the backward's transposed gather may skip
        # the rows of those slots (selected_cols)
        ctx.ce_sel = (y, mask, weight.size(0)) if want_grad else None
        if want_grad:
            if ctx.has_bn:
                ctx.save_for_backward(dlogits, z, weight, root_weight, x, bn_weight, mean, rstd, n, scale, shift)
                ctx.reduce = bn_args[1]
            else:
                ctx.save_for_backward(dlogits, z, weight, root_weight, x if root_weight is not None else None)
        ctx.mark_non_differentiable(stats)
        if stats.dim() == 2:  # two masks (statistics only): the caller reads the [2, 3] table
            return stats.new_zeros(()).float(), stats
        return (stats[0] / stats[1]).float(), stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        from .nn import batchnorm as B
        saved = ctx.saved_tensors
        if ctx.has_bn:
            gy, z, weight, root_weight, x, bn_weight, mean, rstd, n, scale, shift = saved
        else:
            gy, z, weight, root_weight, x = saved
        graph, kind = ctx.graph, ctx.kind
        g = g.reshape(()).float()
        gw = gb = gwr = gx = g_bnw = g_bnb = None
        gcol = None
        sparse = ctx.ce_no_fill  # the unlisted rows of gy and z were never written: every reader below must skip them
        if ctx.needs_input_grad[3]:  # z was stored by the forward exactly when the weight wants a gradient
            # gy is zero outside the rows the loss selects: the product runs over the list of those rows where it exists
            rows = selected_rows(*ctx.ce_sel) if FUSE_DENSE_BACKWARD else None
            if sparse and rows is None:
                raise RuntimeError("propagate_linear_ce: the loss gradient was stored without its zero rows, and the row "
                                   "list its weight gradient walks is gone (FUSE_DENSE_BACKWARD switched off since?)")
            gw, gcol = gemm_tn_rows(gy, z, rows, colsum=True, rows_only=sparse)
        if sparse and (gcol is None or root_weight is not None):
            raise RuntimeError("propagate_linear_ce: the loss gradient was stored without its zero rows, but a full pass "
                               "over it is wanted")
        if ctx.has_bias and ctx.needs_input_grad[4]:
            gb = gcol if gcol is not None else gy.sum(0)
        if root_weight is not None and ctx.needs_input_grad[5]:
            if ctx.has_bn:  # dWr = dy^T BN(x) = (dy^T x) diag(s) + colsum(dy) t^T
                gcol = gcol if gcol is not None else gy.sum(0)
                gwr = gemm_tn(gy, x) * scale + gcol[:, None] * shift
            else:
                gwr = gemm_tn(gy, x)
        need_h = ctx.needs_input_grad[0] or (ctx.has_bn and (ctx.needs_input_grad[9] or ctx.needs_input_grad[10]))
        # the incoming scalar multiplies everything linear in dy: the small operands take it, in ONE multi-tensor launch
        items = [(k, t) for k, t in (("gw", gw), ("gb", gb), ("gwr", gwr)) if t is not None]
        if need_h:
            items.append(("w", weight.detach()))
            if root_weight is not None:
                items.append(("wr", root_weight.detach()))
        sc = dict(zip((k for k, _ in items), torch._foreach_mul([t for _, t in items], g))) if items else {}
        gw, gb, gwr = sc.get("gw"), sc.get("gb"), sc.get("gwr")
        if need_h:
            g_h = _propagate_linear_input_grad(graph, kind, gy, sc["w"], sc.get("wr"), ce_sel=ctx.ce_sel, sparse_gy=sparse)
            if ctx.has_bn and not ctx.handed_over:
                gx, g_bnw, g_bnb = B.train_backward(g_h, x, bn_weight, mean, rstd, n, ctx.reduce)
            else:
                gx = g_h
        return gx, None, None, gw, gb, gwr, None, None, None, g_bnw, g_bnb, None


def propagate_linear_ce(x, graph, kind, weight, bias, root_weight, y, mask, bn=None, colsums=None):
    """(loss, stats) = masked cross-entropy of the last conv's logits, taken inside rgbx_spmm_linear_f32 (the
    caller checked fused_ce_ok, and bn.folds_into_next_layer when a training BatchNorm `bn` is handed over)."""
    # any operand a gradient can reach (frozen-weight fine-tuning: only a bias or the root weight may want one)
    want_grad = not isinstance(mask, (tuple, list)) and torch.is_grad_enabled() and any(
        t is not None and t.requires_grad
        for t in (weight, x, bias, root_weight) + ((bn.weight, bn.bias) if bn is not None else ()))
    if bn is not None:
        bn_args = (bn.eps, bn._reduce, bn.begin_training_step(), colsums, _take_handover(x, bn) if want_grad else None)
        return _PropagateLinearCE.apply(x, graph, kind, weight, bias, root_weight, y, mask, want_grad, bn.weight, bn.bias,
                                        bn_args)
    return _PropagateLinearCE.apply(x, graph, kind, weight, bias, root_weight, y, mask, want_grad, None, None, None)


def bn_propagate_linear(x, bn, graph, kind, weight, bias=None, root_weight=None, colsums=None, want_colsums=False):
    """conv(bn(x)) for a training-mode BatchNorm1d `bn` and a conv layer whose propagate runs on the fused
    aggregate+transform kernel (single-GPU graphs; the caller checked fused_linear_ok and bn.folds_into_next_layer).
    `colsums`: the [2, d] column sums of x and x^2 if the launch that produced x already took them."""
    need_z = weight.requires_grad
    return _tag_colsums(_BNPropagateLinear.apply(x, bn.weight, bn.bias, graph, kind, weight, bias, root_weight, bn.eps,
                                                 bn._reduce, bn.begin_training_step(), need_z, colsums, want_colsums,
                                                 _take_handover(x, bn)),
                        want_colsums)


COLSUMS = "_rgbx_colsums"  # attribute a conv output carries when the launch also produced its column sums


def _tag_colsums(res, want_colsums):
    """(out, colsums) of a Function -> out, with the [2, Nout] float64 column sums of out and out^2 riding on it as
    an attribute for the BatchNorm that follows (models/_stack.ConvStack reads it right after the conv returns)."""
    if not want_colsums:
        return res
    out, colsums = res
    setattr(out, COLSUMS, colsums)
    return out


def propagate_linear(x, graph, kind, weight, bias=None, root_weight=None, want_colsums=False, next_bn=None):
    """`next_bn`: the training-mode BatchNorm1d the caller will hand, with this output, to the next conv
    (forward_after_bn) and to nothing else: this node then owns that BatchNorm's backward (BNHandover)."""
    if _is_dist(graph):  # resident input features of a partitioned graph (fused_linear_ok checked it)
        return graph.propagate_linear(x, kind, weight, bias, root_weight)
    # the aggregate is kept only when the weight gradient (dy^T (P x)) will be asked for; Function.forward
    # cannot see the caller's grad mode, so the decision is taken here
    need_z = torch.is_grad_enabled() and weight.requires_grad
    if next_bn is None or not FUSE_DENSE_BACKWARD or not torch.is_grad_enabled():
        return _tag_colsums(_PropagateLinear.apply(x, graph, kind, weight, bias, need_z, root_weight, None, want_colsums),
                            want_colsums)
    rec = BNHandover(next_bn)
    out = _tag_colsums(_PropagateLinear.apply(x, graph, kind, weight, bias, need_z, root_weight, None, want_colsums,
                                              next_bn.weight, next_bn.bias, rec), want_colsums)
    setattr(out, BN_HANDOVER, rec)
    return out


def appnp_raw(csr, w, h, K, alpha, kind="appnp"):
    _lib.require_device(h)
    h = h.contiguous()
    hm = _lib.mat(h, "h")
    out = torch.empty_like(h)
    tmp = torch.empty_like(h) if K > 1 else None
    po, ldo = _lib.mat(out, "out")  # out and tmp share the leading dimension
    split, _scratch = csr.split_arg(h.size(1), h.device)
    _launch(kind, "rgbx_appnp_f32", csr.rowptr, csr.col, w, hm, po, tmp, ldo, csr.N, h.size(1), int(K), float(alpha), split)
    return out


class _APPNP(torch.autograd.Function):
    """z <- (1-alpha) A_hat z + alpha h, K times (appnp_stack.py:29; twin pta.py:79-84).

    Backward is the same recurrence on the transposed graph applied to the incoming gradient:
    dL/dh = M^K g + alpha * sum_{j<K} M^j g with M = (1-alpha) A_hat^T (Horner form)."""

    @staticmethod
    def forward(ctx, h, graph, K, alpha):
        ctx.graph, ctx.K, ctx.alpha = graph, K, alpha
        return appnp_raw(graph.fwd, graph.w, h, K, alpha, kind="appnp_fwd")

    @staticmethod
    def backward(ctx, gy):
        g = ctx.graph
        return appnp_raw(g.bwd, g.w_t, gy, ctx.K, ctx.alpha, kind="appnp_bwd"), None, None, None


class _APPNPCE(torch.autograd.Function):
    """(loss, stats) of the masked cross-entropy of APPNP's output (models/appnp_stack.py:29-31 followed by the loss of
    itexperiments.py:429 / the metrics of :624-626): steps 1..K-1 as rgbx_appnp_f32, the last step on the row kernel with
    the loss epilogue — the [N, C] logits are never written. `h` is [N, n] with columns [n_classes, n) zero padding.
    Backward: the recurrence on the transposed graph applied to the stored loss gradient (see _APPNP)."""

    @staticmethod
    def forward(ctx, h, graph, K, alpha, labels, mask, n_classes, want_grad):
        h = h.contiguous()
        z = appnp_raw(graph.fwd, graph.w, h, K - 1, alpha, kind="appnp_fwd") if K > 1 else h
        grad_scale = mask_scale(labels, mask, n_classes) if want_grad else None
        dlogits, stats = spmm_epilogue_raw(graph.fwd, graph.w, None, z, y=h, a=1.0 - alpha, b=alpha,
                                           ce=(labels, mask, grad_scale), n_classes=n_classes, kind="appnp_fwd")
        ctx.graph, ctx.K, ctx.alpha = graph, K, alpha
        if want_grad:
            ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(stats)
        if stats.dim() == 2:
            return stats.new_zeros(()).float(), stats
        return (stats[0] / stats[1]).float(), stats

    @staticmethod
    def backward(ctx, g, _g_stats=None):
        if not ctx.saved_tensors:
            raise RuntimeError("appnp_propagate_ce: backward asked of a forward that was run without want_grad")
        gy = ctx.saved_tensors[0] * g.reshape(()).float()
        gr = ctx.graph
        return appnp_raw(gr.bwd, gr.w_t, gy, ctx.K, ctx.alpha, kind="appnp_bwd"), None, None, None, None, None, None, None


def appnp_propagate_ce(h, graph, K, alpha, n_classes, y, mask):
    """(loss, stats) of APPNP(K, alpha)(h)'s masked cross-entropy with the loss inside the last step's kernel; h [N, n],
    n % 4 == 0, columns beyond n_classes zero (pad_rows4). The caller checked rows_epilogue_ok and K >= 1."""
    pair = isinstance(mask, (tuple, list))
    want_grad = (not pair) and torch.is_grad_enabled() and h.requires_grad
    loss, stats = _APPNPCE.apply(h, graph, int(K), float(alpha), y, mask, int(n_classes), want_grad)
    return (None if pair else loss), stats


def appnp_propagate(h, graph, K, alpha):
    if _is_dist(graph):
        out = graph.appnp(h, K, alpha)  # reshard scheme: all K steps inside one pair of transposes
        if out is not None:
            return out
        z = h  # halo scheme: one exchange per iteration; autograd chains the K distributed propagates
        for _ in range(K):
            z = (1.0 - alpha) * graph.propagate(z, "gcn") + alpha * h
        return z
    hp, d = _pad4(h)  # C = 7 classes: all K propagates on 8-float rows
    out = _APPNP.apply(hp, graph, K, alpha)
    return out if hp is h else out[:, :d]


class _DAGNNProp(torch.autograd.Function):
    """Prop.forward of DAGNN (reference models/dagnn.py:41-55): K gcn-normalised propagates, then
    out = sum_k sigmoid(<hop_k, s> + b) * hop_k over the K+1 hops. The hops are written by the SpMM into one
    [K, N, d] buffer and read once by rgbx_dagnn_gate_fwd_f32 — no stack, no [N, K+1, d] projection input.
    Backward: one pass (rgbx_dagnn_gate_bwd_f32) writes every hop's direct gradient and reduces g_s / g_b; the
    chain through the propagates is the Horner form G_k = A_hat^T G_{k+1} + direct_k, K transposed SpMMs that add
    their `y` operand in the store."""

    @staticmethod
    def forward(ctx, x, graph, K, s, b):
        N, d = x.shape
        x = x.contiguous()
        hops = torch.empty((K, N, d), dtype=torch.float32, device=x.device)
        src = x
        for k in range(K):
            spmm_raw(graph.fwd, graph.w, None, src, out=hops[k], kind="gcn_fwd")
            src = hops[k]
        out = torch.empty_like(x)
        sv = s.detach().reshape(-1).contiguous()
        bv = None if b is None else b.detach().reshape(-1).contiguous()
        _launch("dagnn_gate_fwd", "rgbx_dagnn_gate_fwd_f32", x, x.stride(0), hops, N * d, d, sv, bv, out, out.stride(0),
                N, d, K)
        ctx.graph, ctx.K, ctx.has_b = graph, K, b is not None
        ctx.save_for_backward(x, hops, sv, bv)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, hops, sv, bv = ctx.saved_tensors
        g, K = ctx.graph, ctx.K
        N, d = x.shape
        gout = gout.contiguous()
        d0 = torch.empty_like(x)
        dk = torch.empty((K, N, d), dtype=torch.float32, device=x.device)
        g_s = torch.empty(d, dtype=torch.float32, device=x.device)
        g_b = torch.empty(1, dtype=torch.float32, device=x.device) if ctx.has_b else None
        need = ctypes.c_size_t(0)
        _lib.call("rgbx_dagnn_gate_bwd_workspace_bytes", d, ctypes.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
        _launch("dagnn_gate_bwd", "rgbx_dagnn_gate_bwd_f32", x, x.stride(0), hops, N * d, d, sv, bv, gout, gout.stride(0),
                d0, d0.stride(0), dk, N * d, d, g_s, g_b, ws, need.value, N, d, K)
        gx = None
        if ctx.needs_input_grad[0]:
            # G_K = direct_K; G_k = A_hat^T G_{k+1} + direct_k, each written over direct_k
            cur = dk[K - 1] if K else d0
            for k in range(K - 1, -1, -1):
                dst = dk[k - 1] if k else d0
                spmm_raw(g.bwd, g.w_t, None, cur, y=dst, a=1.0, b=1.0, out=dst, kind="gcn_bwd")
                cur = dst
            gx = d0
        return gx, None, None, g_s, g_b


def dagnn_prop(x, graph, K, proj_weight, proj_bias=None):
    """DAGNN's propagate-and-mix (reference models/dagnn.py:41-55) on the HIP path; proj_weight [1, C], proj_bias [1].
    Returns None when this shape is left to the caller's torch formulation (a partitioned graph, C > 256)."""
    if _is_dist(graph) or x.size(1) > 256:
        return None
    _lib.require_device(x, proj_weight, proj_bias)
    xp, d = _pad4(x)
    s = proj_weight.reshape(-1)
    if xp is not x:
        s = torch.nn.functional.pad(s, (0, xp.size(1) - d))  # zero columns: no part in the scores or the mix
    out = _DAGNNProp.apply(xp, graph, int(K), s, proj_bias)
    return out if xp is x else out[:, :d]


# ---- GGNN: one GatedGraphConv step (csrc/gru.hip) -----------------------------------------------------------------

GRU_FORMS = ("fused", "composed", "general")
# None = the default choice (gru_step_form): the fused step wherever it applies, else the general form. The A/B tool
# (tools/ggnn_bench.py) sets a form explicitly.
GRU_FORM = None


def gru_step_supported(C):
    """The fused step (rgbx_gru_step_f32) takes state width C (a multiple of 4): 4 C a multiple of 32 and <= 256."""
    return bool(_lib.load().rgbx_gru_step_supported(int(C)))


def gru_step_form(C, form=None):
    form = form or GRU_FORM
    if form is None:
        return "fused" if gru_step_supported(C) else "general"
    if form not in GRU_FORMS:
        raise ValueError(f"unknown GRU step form {form!r} (one of {GRU_FORMS})")
    if form != "general" and not gru_step_supported(C):
        raise RuntimeError(f"the {form} GRU step needs 4 C a multiple of 32 and at most 256 (C = {C}); use 'general'")
    return form


def gru_operands(weight_i, w_ih, w_hh, b_ih, b_hh, Cp):
    """(Weff [4Cp, Cp], Wroot [4Cp, Cp], bias [4Cp]) of one step at padded width Cp >= C, from the step's weight [C, C]
    and the GRUCell's parameters (gates r, z, n): pre = (A x) Weffᵀ + x Wrootᵀ + bias has the columns
    [r, z pre-activations | gi_n | gh_n], each block Cp wide (pad rows and columns zero: a zero pad column of the state
    stays zero). Differentiable torch ops on the parameters: autograd carries dWeff back to W_ih and weight_i."""
    C = weight_i.size(0)
    p = Cp - C
    pad = torch.nn.functional.pad
    wi = (w_ih @ weight_i.t()).view(3, C, C)  # (A x) weight_i W_ihᵀ = (A x) (W_ih weight_iᵀ)ᵀ
    wh = w_hh.view(3, C, C)
    if p:
        wi, wh = pad(wi, (0, p, 0, p)), pad(wh, (0, p, 0, p))
    zero = wi.new_zeros(Cp, Cp)
    weff = torch.cat([wi[0], wi[1], wi[2], zero], 0)
    wroot = torch.cat([wh[0], wh[1], zero, wh[2]], 0)
    if b_ih is None:
        bias = wi.new_zeros(4 * Cp)
    else:
        bi, bh = b_ih.view(3, C), b_hh.view(3, C)
        if p:
            bi, bh = pad(bi, (0, p)), pad(bh, (0, p))
        bias = torch.cat([bi[0] + bh[0], bi[1] + bh[1], bi[2], bh[2]], 0)
    return weff, wroot, bias


def gru_gate_fwd(pre, x, out=None):
    """The GRU cell over a finished pre [N, 4C] (rgbx_gru_gate_fwd_f32): the new state [N, C]."""
    _lib.require_device(pre, x)
    N, C = x.shape
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _launch("gru_gate_fwd", "rgbx_gru_gate_fwd_f32", _lib.mat(pre, "pre"), _lib.mat(x, "x"), _lib.mat(out, "out"), N, C,
            variant=f"d{C}" if _EVENT_SINK is not None else None)
    return out


def gru_gate_bwd(pre, x, gout):
    """(dpre [N, 4C], dx_direct [N, C] = gout ⊙ z) of the GRU cell (rgbx_gru_gate_bwd_f32)."""
    _lib.require_device(pre, x, gout)
    N, C = x.shape
    dpre = torch.empty((N, 4 * C), dtype=torch.float32, device=x.device)
    dx = torch.empty((N, C), dtype=torch.float32, device=x.device)
    _launch("gru_gate_bwd", "rgbx_gru_gate_bwd_f32", _lib.mat(pre, "pre"), _lib.mat(x, "x"), _lib.mat(gout, "gout"),
            dpre, 4 * C, dx, C, N, C, variant=f"d{C}" if _EVENT_SINK is not None else None)
    return dpre, dx


def gru_step_raw(x, graph, weff, wroot, bias, form, want_saved=False):
    """One step without autograd: returns (x', z = A x or None, pre or None); z and pre only when `want_saved`.
    fused: rgbx_gru_step_f32 (gather, both products and the cell in one kernel). composed: the fused aggregate +
    transform kernel writes pre (rgbx_spmm_linear_f32 with the root term), the gate kernel follows. general: the sum
    aggregation at width C (rgbx_spmm_csr_f32), pre by two dense products, the gate kernel."""
    _lib.require_device(x, weff, wroot, bias)
    N, C = x.shape
    dev = x.device
    b = bias.detach().contiguous()
    if form == "fused":
        out = torch.empty((N, C), dtype=torch.float32, device=dev)
        z = torch.empty((N, C), dtype=torch.float32, device=dev) if want_saved else None
        pre = torch.empty((N, 4 * C), dtype=torch.float32, device=dev) if want_saved else None
        wt, wtr = weff.detach().t().contiguous(), wroot.detach().t().contiguous()
        xm = _lib.mat(x, "x")
        split, _scratch = graph.fwd.split_arg(C, dev, hub_rows=True)
        _launch("gru_step_fwd", "rgbx_gru_step_f32", graph.fwd.rowptr, graph.fwd.col, xm, wt, wtr, b, out, C, z, C, pre,
                4 * C, N, C, split, variant=f"d{C}{'+z+pre' if want_saved else ''}" if _EVENT_SINK is not None else None)
        return out, z, pre
    if form == "composed":
        pre, z = spmm_linear_raw(graph.fwd, None, None, x, weff.detach().t().contiguous(), b, want_saved, x,
                                 wroot.detach().t().contiguous(), kind="gru_linear_fwd")
    elif form == "general":
        z = spmm_raw(graph.fwd, None, None, x, kind="sum_fwd")
        pre = torch.addmm(b, z, weff.detach().t())
        pre.addmm_(x, wroot.detach().t())
    else:
        raise ValueError(form)
    return gru_gate_fwd(pre, x), z, pre


class _GRUStep(torch.autograd.Function):
    """x' = GRU cell of pre = (A x) Weffᵀ + x Wrootᵀ + bias (see gru_operands). Backward: dpre and the direct part
    dx' ⊙ z from the gate backward kernel; dWeff = dpreᵀ (A x) and dbias = column sums of dpre in one pass of the split-K
    MFMA kernel, dWroot = dpreᵀ x; dx = Aᵀ(dpre Weff) + dpre Wroot + dx' ⊙ z with the transposed gather at width C."""

    @staticmethod
    def forward(ctx, x, graph, weff, wroot, bias, form):
        x = _rows_on_grid(x)
        want = any(ctx.needs_input_grad)
        out, z, pre = gru_step_raw(x, graph, weff, wroot, bias, form, want_saved=want)
        if want:
            ctx.save_for_backward(x, z, pre, weff, wroot)
            ctx.graph = graph
        return out

    @staticmethod
    def backward(ctx, gout):
        x, z, pre, weff, wroot = ctx.saved_tensors
        dpre, dxd = gru_gate_bwd(pre, x, _rows_on_grid(gout))
        gw = gb = gwr = gx = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[4]:
            gw, gb = gemm_tn(dpre, z, colsum=True)  # dpre is read once for dWeff and dbias
        if ctx.needs_input_grad[3]:
            gwr = gemm_tn(dpre, x)
        if ctx.needs_input_grad[0]:
            g1 = dpre @ weff.detach()
            g2 = torch.addmm(dxd, dpre, wroot.detach())
            gx = spmm_raw(ctx.graph.bwd, None, None, g1, y=g2, a=1.0, b=1.0, out=g2, kind="sum_bwd")
        return gx, None, gw, gwr, gb, None


def gru_step(x, graph, weff, wroot, bias, form=None):
    """One GatedGraphConv step on the state x [N, Cp] (Cp % 4 == 0, single-GPU graph); operands from gru_operands.
    `form`: one of GRU_FORMS, None = gru_step_form's default."""
    if _is_dist(graph):
        raise RuntimeError("GatedGraphConv has no node-partitioned form: run it on one GPU")
    C = x.size(1)
    if C % 4:
        raise RuntimeError(f"gru_step: the state width must be a multiple of 4 (got {C}); pad it (GatedGraphConv does)")
    return _GRUStep.apply(x, graph, weff, wroot, bias, gru_step_form(C, form))


class _GATScores(torch.autograd.Function):
    """a_src[n,h] = <hfeat[n,h,:], att_src[h,:]> and a_dst likewise (GATConv.forward [PyG])."""

    @staticmethod
    def forward(ctx, hfeat, att_src, att_dst, H, C):
        _lib.require_device(hfeat, att_src, att_dst)
        hfeat = hfeat.contiguous()
        n = hfeat.size(0)
        a_src = torch.empty((n, H), dtype=torch.float32, device=hfeat.device)
        a_dst = torch.empty_like(a_src)
        hm = _lib.mat(hfeat, "hfeat")
        att_s = att_src.reshape(H, C).contiguous()
        att_d = att_dst.reshape(H, C).contiguous()
        _lib.launch("rgbx_gat_scores_f32", hm, att_s, att_d, a_src, a_dst, n, H, C)
        ctx.save_for_backward(hfeat, att_s, att_d)
        ctx.H, ctx.C, ctx.att_shape = H, C, att_src.shape
        return a_src, a_dst

    @staticmethod
    def backward(ctx, g_as, g_ad):
        hfeat, att_s, att_d = ctx.saved_tensors
        H, C = ctx.H, ctx.C
        h3 = hfeat.view(-1, H, C)
        g_h = (g_as.unsqueeze(-1) * att_s + g_ad.unsqueeze(-1) * att_d).reshape(hfeat.shape)
        g_att_s = torch.einsum("nh,nhc->hc", g_as, h3).reshape(ctx.att_shape)
        g_att_d = torch.einsum("nh,nhc->hc", g_ad, h3).reshape(ctx.att_shape)
        return g_h, g_att_s, g_att_d, None, None


class _GATAggregate(torch.autograd.Function):
    """out[i,h,:] = sum_j softmax_j(leaky_relu(a_src[j,h] + a_dst[i,h])) * hfeat[j,h,:]."""

    @staticmethod
    def forward(ctx, hfeat, a_src, a_dst, graph, H, C, slope, att_src=None, want_grad=True):
        """`att_src` ([H, C], no gradient through this argument: the score path's gradient flows through
        `a_src`) lets the kernel form the source scores from the rows it gathers anyway. `want_grad`: a backward
        will follow (the forward then also stores the positive-score parts the backward's prep pass needs)."""
        _lib.require_device(hfeat, a_src, a_dst, att_src)
        hfeat, a_src, a_dst = hfeat.contiguous(), a_src.contiguous(), a_dst.contiguous()
        att = None if att_src is None else att_src.detach().reshape(H, C).contiguous()
        N = graph.fwd.N  # targets; hfeat / a_src may have more rows (sources incl. a halo) than targets
        dev = hfeat.device
        out = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        m = torch.empty((N, H), dtype=torch.float32, device=dev)
        rden = torch.empty_like(m)
        csr = graph.fwd
        opos, apos = _gat_train_extras(want_grad, N, H, C, dev)
        split, _scratch = csr.split_arg((2 * H * C + 3 * H) if want_grad else (H * C + 2 * H), dev)
        _launch("gat_fwd", "rgbx_gat_aggregate_fwd_f32", csr.rowptr, csr.col, _lib.mat(hfeat, "hfeat"), a_src, att, a_dst,
                None, None, None, _lib.mat(out, "out"), m, rden, opos, apos, N, H, C, float(slope), split)
        ctx.save_for_backward(hfeat, a_src, a_dst, m, rden, out, opos, apos)
        ctx.graph, ctx.H, ctx.C, ctx.slope = graph, H, C, slope
        return out

    @staticmethod
    def backward(ctx, gout):
        """Two launches, one full gather pass: (1) per-target records nodeq = (a_dst, max - log(1/sum),
        <gout, out>) and the target-side score gradient g_a_dst in a streaming pass; (2) the source-side pass
        over the transposed CSR gathers gout rows + records and produces g_hfeat and g_a_src."""
        hfeat, a_src, a_dst, m, rden, out, opos, apos = ctx.saved_tensors
        g_h, g_as, g_ad = _gat_backward_core(ctx.graph, hfeat, a_src, a_dst, m, rden, out, gout.contiguous(), ctx.H,
                                             ctx.C, ctx.slope, opos=opos, apos=apos)
        return g_h, g_as, g_ad, None, None, None, None, None, None


def _gat_train_extras(want_grad, N, H, C, dev):
    """(out_pos [N, H*C], a_pos [N, H]) buffers of a forward whose backward will be asked for, else (None, None)."""
    if not want_grad:
        return None, None
    return (torch.empty((N, H * C), dtype=torch.float32, device=dev),
            torch.empty((N, H), dtype=torch.float32, device=dev))


def _gat_backward_core(g, hfeat, a_src, a_dst, m, rden, out, gout, H, C, slope, bias=None, opos=None, apos=None,
                       att=None):
    """(g_hfeat through the aggregation, g_a_src [n_src, H], g_a_dst [n_tgt, H]). `bias`: the vector the
    forward added to `out` in its store, if any. `opos` / `apos`: the positive-score parts the forward stored
    (rgbx_gat_aggregate_fwd_f32 out_pos / a_pos): with them g_a_dst comes out of the streaming prep pass; without
    them (a forward run without want_grad) the source-side pass also writes the per-edge score gradient ds [E', H]
    and g_a_dst is its width-H segment sum over each target's in-edges. `att` = (att_src, att_dst) [H, C] (needs
    opos / apos): the scores are products of hfeat with these vectors, so the source pass folds their backward into
    its g_hfeat store (and forms the source's own score from its row when `a_src` is None)."""
    N, n_src, dev = g.fwd.N, g.bwd.N, gout.device
    nodeq = torch.empty((N, H, 4), dtype=torch.float32, device=dev)  # (a_dst, max - log(1/sum), dsum, -) records
    g_as = torch.empty((n_src, H), dtype=torch.float32, device=dev)
    g_h = torch.empty_like(hfeat)
    hm, gm = _lib.mat(hfeat, "hfeat"), _lib.mat(gout, "gout")
    per_node = opos is not None
    fold = per_node and att is not None
    if a_src is None and not fold:
        raise RuntimeError("gat backward: a_src may only be left to the kernel together with the folded score backward")
    g_ad = None
    if per_node:  # the fold reads g_a_dst by SOURCE row: rows that are no target (halo rows of a partitioned run) are 0
        g_ad_full = (torch.zeros if fold and n_src > N else torch.empty)((max(n_src, N) if fold else N, H),
                                                                         dtype=torch.float32, device=dev)
        g_ad = g_ad_full[:N]
    att2 = torch.cat([att[0].reshape(1, H, C), att[1].reshape(1, H, C)]).contiguous() if fold else None
    ds = None if per_node else torch.empty((max(g.bwd.nnz, 1), H), dtype=torch.float32, device=dev)
    _launch("gat_bwd_prep", "rgbx_gat_bwd_prep_f32", a_dst, m, rden, _lib.mat(out, "out"), bias, gm, nodeq, opos, apos,
            float(slope), g_ad, N, H, C)
    split, _scratch = g.bwd.split_arg(H * C + 2 * H, dev)
    _launch("gat_bwd_src", "rgbx_gat_bwd_src_f32", g.bwd.rowptr, g.bwd.col, hm, a_src, nodeq, gm, _lib.mat(g_h, "g_hfeat"),
            g_as, ds, att2, g_ad_full if fold else None, n_src, H, C, float(slope), split)
    if not per_node:
        g_ad = spmm_raw(gat_segment_csr(g), None, None, ds, kind="gat_bwd_segsum")
    return g_h, g_as, g_ad


def gat_segment_csr(graph):
    """CSR over the targets whose `col` is, per forward slot, the TRANSPOSED slot of the same edge: summing
    rows of the per-edge tensor `ds` (stored in transposed-slot order) through it gives per-target totals.
    Built once per graph from the two slot -> edge-id permutations."""
    seg = getattr(graph, "_gat_seg", None)
    if seg is None:
        from .graph import CSR
        f, b = graph.fwd, graph.bwd
        if f.nnz:
            inv = torch.empty(int(max(f.perm[:f.nnz].max(), b.perm[:b.nnz].max()).item()) + 1, dtype=torch.int32,
                              device=f.perm.device)
            inv[b.perm[:b.nnz].long()] = torch.arange(b.nnz, dtype=torch.int32, device=inv.device)
            col = inv[f.perm[:f.nnz].long()].contiguous()
        else:
            col = f.col
        seg = CSR(f.rowptr, col, f.perm, f.N, f.nnz, f.split)
        graph._gat_seg = seg
    return seg


def gat_scores(hfeat, att_src, att_dst, H, C):
    return _GATScores.apply(hfeat, att_src, att_dst, H, C)


def gat_aggregate(hfeat, a_src, a_dst, graph, H, C, slope=0.2, att_src=None):
    want_grad = torch.is_grad_enabled() and (hfeat.requires_grad or a_src.requires_grad or a_dst.requires_grad)
    return _GATAggregate.apply(hfeat, a_src, a_dst, graph, H, C, slope, att_src, want_grad)


class _GATAttend(torch.autograd.Function):
    """One GATConv attention block as a single autograd node: scores (rgbx_gat_scores_f32) + fused
    edge-softmax/aggregate forward; backward = prep + source pass + segment sum (as _GATAggregate) followed
    by rgbx_gat_scores_bwd_f32, which folds the score gradients into g_hfeat in place and reduces the
    attention-vector gradients without materialising [N, H, C] products. `bias` ([H*C], optional) is added
    in the aggregation kernel's store (GATConv's `+ bias` for concatenated heads). `out_scale` ([H*C], inference
    only — the stored rows are then not the aggregate the backward needs): stored row = aggregate * out_scale + bias,
    an eval-mode BatchNorm after the layer folded into the store."""

    @staticmethod
    def forward(ctx, hfeat, att_src, att_dst, graph, H, C, slope, bias=None, out_scale=None, want_grad=True):
        _lib.require_device(hfeat, att_src, att_dst, bias, out_scale)
        hfeat = hfeat.contiguous()
        b = None if bias is None else bias.detach().reshape(H * C).contiguous()
        sc = None if out_scale is None else out_scale.detach().reshape(H * C).contiguous()
        ctx.inference_only = sc is not None
        att_s = att_src.detach().reshape(H, C).contiguous()
        att_d = att_dst.detach().reshape(H, C).contiguous()
        n_src, N, dev = hfeat.size(0), graph.fwd.N, hfeat.device
        hm = _lib.mat(hfeat, "hfeat")
        want_grad = want_grad and sc is None
        in_kernel = _scores_in_kernel(C)
        if in_kernel:
            # heads spanning <= 8 lanes: both score products are formed inside the aggregation kernel from rows it
            # holds anyway (the gathered row for a_src, the target's own row for a_dst): no scores pass over hfeat.
            # a_dst is stored only for a backward (the per-target records need it)
            a_src = None
            a_dst = torch.empty((N, H), dtype=torch.float32, device=dev) if want_grad else None
        else:
            a_src = torch.empty((n_src, H), dtype=torch.float32, device=dev)
            a_dst = torch.empty_like(a_src)
            _lib.launch("rgbx_gat_scores_f32", hm, att_s, att_d, a_src, a_dst, n_src, H, C)
        out = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        m = torch.empty((N, H), dtype=torch.float32, device=dev)
        rden = torch.empty_like(m)
        opos, apos = _gat_train_extras(want_grad, N, H, C, dev)
        split, _scratch = graph.fwd.split_arg((2 * H * C + 3 * H) if want_grad else (H * C + 2 * H), dev)
        _launch("gat_fwd", "rgbx_gat_aggregate_fwd_f32", graph.fwd.rowptr, graph.fwd.col, hm, a_src,
                att_s if in_kernel else None, a_dst, att_d if in_kernel else None, sc, b, _lib.mat(out, "out"), m, rden,
                opos, apos, N, H, C, float(slope), split)
        ctx.save_for_backward(hfeat, a_src, a_dst, m, rden, out, att_s, att_d, b, opos, apos)
        ctx.graph, ctx.H, ctx.C, ctx.slope = graph, H, C, slope
        ctx.att_shapes = (att_src.shape, att_dst.shape)
        ctx.bias_shape = None if bias is None else bias.shape
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.inference_only:
            raise RuntimeError("gat_attend(out_scale=...) is an inference-only form (eval-mode BatchNorm fold)")
        hfeat, a_src, a_dst, m, rden, out, att_s, att_d, b, opos, apos = ctx.saved_tensors
        H, C = ctx.H, ctx.C
        gout = gout.contiguous()
        if opos is None:
            raise RuntimeError("gat_attend: backward asked of a forward that was run without want_grad")
        g_h, g_as, g_ad = _gat_backward_core(ctx.graph, hfeat, a_src, a_dst, m, rden, out, gout, H, C, ctx.slope, b,
                                             opos=opos, apos=apos, att=(att_s, att_d))
        g_b = gout.sum(0).reshape(ctx.bias_shape) if b is not None and ctx.needs_input_grad[7] else None
        n = hfeat.size(0)
        n_scr = ctypes.c_int64(0)
        _lib.call("rgbx_gat_scores_bwd_scratch_floats", n, H, C, ctypes.byref(n_scr))
        scratch = torch.empty(n_scr.value, dtype=torch.float32, device=hfeat.device)
        g_att_s = torch.empty((H, C), dtype=torch.float32, device=hfeat.device)
        g_att_d = torch.empty_like(g_att_s)
        # the source pass folded the score terms into g_h: attention-vector sums only
        _launch("gat_scores_bwd", "rgbx_gat_scores_bwd_f32", _lib.mat(hfeat, "hfeat"), g_as, g_ad, g_ad.size(0), att_s,
                att_d, None, 0, g_att_s, g_att_d, scratch, n_scr.value, n, H, C)
        return (g_h, g_att_s.reshape(ctx.att_shapes[0]), g_att_d.reshape(ctx.att_shapes[1]), None, None, None, None, g_b,
                None, None)


def gat_attend(h, att_src, att_dst, graph, H, C, slope=0.2, bias=None, out_scale=None):
    """Scores + edge-softmax + aggregation (* out_scale + bias) of one GATConv; dispatches to the partitioned
    graph. `out_scale` is for inference (no_grad) only."""
    if _is_dist(graph):
        out = graph.gat(h, att_src, att_dst, H, C, slope)
        if out_scale is not None:
            out = out * out_scale
        return out if bias is None else out + bias
    if out_scale is not None and torch.is_grad_enabled():
        raise RuntimeError("gat_attend(out_scale=...) is an inference-only form")
    want_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (h, att_src, att_dst, bias))
    return _GATAttend.apply(h, att_src, att_dst, graph, H, C, slope, bias, out_scale, want_grad)


def gat_linear_ok(graph, in_channels, out_channels, x=None, y=None):
    """A single-head GATConv can run aggregate-first (gat_attend_linear): widths the fused kernel's second-aggregate
    form takes, aggregating at the input width not the more expensive order, single-GPU graph."""
    return (not _is_dist(graph) and in_channels in (64, 128, 256) and in_channels <= out_channels <= 128
            and out_channels % 32 == 0 and (x is None or x.is_cuda)
            and (y is None or (y.is_cuda and y.dtype == torch.int64)))


def gat_edge_softmax(csr, a_src, a_dst, slope, train, N):
    """(alpha [E'], alpha_pos or None, m [N], rden [N], a_pos or None) of a single head (rgbx_gat_edge_softmax_f32)."""
    dev = a_src.device
    alpha = torch.empty(max(csr.nnz, 1), dtype=torch.float32, device=dev)
    alpha_pos = torch.empty_like(alpha) if train else None
    m = torch.empty(N, dtype=torch.float32, device=dev)
    rden = torch.empty_like(m)
    a_pos = torch.empty_like(m) if train else None
    split, _scratch = csr.split_arg(1, dev)  # hub rows: a workgroup each (no scratch used)
    _launch("gat_edge_softmax", "rgbx_gat_edge_softmax_f32", csr.rowptr, csr.col, a_src, a_dst, float(slope), alpha,
            alpha_pos, m, rden, a_pos, N, split)
    return alpha, alpha_pos, m, rden, a_pos


class _GATAttendLinear(torch.autograd.Function):
    """A single-head GATConv with its transform BEHIND the aggregation:
        out_i = (sum_j alpha_ij x_j) W^T + b,   alpha = edge softmax of leaky_relu(a_src[j] + a_dst[i]),
        a_src = x (W^T att_src),  a_dst = x (W^T att_dst)
    — the same function as lin -> scores -> edge softmax -> aggregate -> + bias of GATConv.forward with heads = 1 [PyG]
    (the last layer of reference models/gat.py:21,30), re-associated: sum_j alpha_ij (W x_j) = W sum_j alpha_ij x_j.
    Launches: scores over x (no h = x W^T product), the coefficients as a per-edge vector (rgbx_gat_edge_softmax_f32;
    one head: 4 bytes per edge), then rgbx_fused_layer_f32 with w = alpha — the transform on the MFMA units under the
    gather and, with labels given, the loss inside the kernel (no logits). A forward that prepares a backward also
    stores the aggregate z (dW = dy^T z) and its positive-score part (w_pos): exactly the (out, out_pos) pair the
    per-node GAT backward needs with hfeat := x and gout := dy W, so the backward is that of _GATAttend on those
    operands plus the chain through v = att W. `y` / `mask`: returns (loss, stats) as _PropagateLinearCE does."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, graph, slope, y, mask, want_grad):
        _lib.require_device(x, weight, att_src, att_dst, bias)
        x = x.contiguous()
        W = weight.detach()
        C, K = W.shape
        att = torch.stack([att_src.detach().reshape(C), att_dst.detach().reshape(C)])  # [2, C]
        v = (att @ W).contiguous()  # [2, K]: the scores are products of x with these vectors
        n_src, N, dev = x.size(0), graph.fwd.N, x.device
        a_src = torch.empty(n_src, dtype=torch.float32, device=dev)
        a_dst = torch.empty_like(a_src)
        _lib.launch("rgbx_gat_scores_f32", _lib.mat(x, "x"), v[0], v[1], a_src, a_dst, n_src, 1, K)
        alpha, alpha_pos, m, rden, a_pos = gat_edge_softmax(graph.fwd, a_src, a_dst, slope, want_grad, N)
        ce = None
        if y is not None:
            ce = (y, mask, mask_scale(y, mask, C) if want_grad else None)
        out, zz, stats = fused_layer(x, weight_t(weight), csr=graph.fwd, w=alpha,
                                     bias=None if bias is None else bias.detach(), ce=ce, kind="gat_linear_fwd",
                                     w_pos=alpha_pos)
        ctx.graph, ctx.slope, ctx.has_bias, ctx.ce = graph, slope, bias is not None, y is not None
        ctx.shapes = (att_src.shape, att_dst.shape)
        if want_grad:
            z, z_pos = zz
            ctx.save_for_backward(x, a_src, a_dst, m, rden, z, z_pos, a_pos, v, weight, att, out if ctx.ce else None)
        if y is None:
            return out
        ctx.mark_non_differentiable(stats)
        return (stats[0] / stats[1]).float(), stats

    @staticmethod
    def backward(ctx, g, _g_stats=None):
        if not ctx.saved_tensors:
            raise RuntimeError("gat_attend_linear: backward asked of a forward that was run without want_grad")
        x, a_src, a_dst, m, rden, z, z_pos, a_pos, v, weight, att, dlogits = ctx.saved_tensors
        W = weight.detach()
        C, K = W.shape
        if ctx.ce:  # the kernel stored the loss gradient w.r.t. the logits; the incoming scalar rides on W and dW
            dy, scalar = dlogits, g.reshape(()).float()
            Wg = W * scalar
        else:
            dy, scalar, Wg = g.contiguous(), None, W
        g_z = dy @ Wg  # [N, K]: gradient w.r.t. the aggregate
        gw, gcol = gemm_tn(dy, z, colsum=True)
        g_x, g_as, g_ad = _gat_backward_core(ctx.graph, x, a_src, a_dst, m, rden, z, g_z, 1, K, ctx.slope, opos=z_pos,
                                             apos=a_pos, att=(v[0:1], v[1:2]))
        n = x.size(0)
        n_scr = ctypes.c_int64(0)
        _lib.call("rgbx_gat_scores_bwd_scratch_floats", n, 1, K, ctypes.byref(n_scr))
        scratch = torch.empty(n_scr.value, dtype=torch.float32, device=x.device)
        g_v = torch.empty((2, K), dtype=torch.float32, device=x.device)
        # the source pass folded the score terms into g_x: the vectors' sums only
        _launch("gat_scores_bwd", "rgbx_gat_scores_bwd_f32", _lib.mat(x, "x"), g_as, g_ad, g_ad.size(0), v[0], v[1], None, 0,
                g_v[0], g_v[1], scratch, n_scr.value, n, 1, K)
        # v = att W: g_att = g_v W^T, and W collects att^T g_v next to dy^T z
        g_att = g_v @ W.t()
        if scalar is not None:
            gw, gcol = gw * scalar, gcol * scalar
        gw = torch.addmm(gw, att.t(), g_v)
        need = ctx.needs_input_grad
        return (g_x if need[0] else None, gw if need[1] else None,
                g_att[0].reshape(ctx.shapes[0]) if need[2] else None, g_att[1].reshape(ctx.shapes[1]) if need[3] else None,
                gcol if ctx.has_bias and need[4] else None, None, None, None, None, None)


def gat_attend_linear(x, weight, att_src, att_dst, graph, slope=0.2, bias=None, ce=None):
    """Single-head GATConv, aggregate-first (the caller checked gat_linear_ok). `ce` = (y, mask): returns
    (loss, stats) with the loss taken inside the kernel; else the logits."""
    want_grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (x, weight, att_src, att_dst, bias))
    y, mask = ce if ce is not None else (None, None)
    return _GATAttendLinear.apply(x, weight, att_src, att_dst, bias, graph, slope, y, mask, want_grad)


SUPERGAT_REDRAWS = 8  # candidate pairs a negative slot may draw before it is dropped from the loss


def supergat_sample_negatives(graph, seed, n_neg):
    """(neg int64 [2, n_neg], valid uint8 [n_neg]): ordered non-edges drawn on the device (no host read)."""
    dev = seed.device
    neg = torch.empty((2, max(n_neg, 1)), dtype=torch.int64, device=dev)[:, :n_neg].contiguous()
    valid = torch.empty(n_neg, dtype=torch.uint8, device=dev)
    keys, n_keys = graph.undirected_keys
    _lib.launch("rgbx_supergat_sample_negatives", keys, n_keys, graph.N, seed, n_neg, SUPERGAT_REDRAWS, neg, valid)
    return neg, valid


def supergat_random_choices(record, graph, H):
    """The exact random choices of the training forward that filled `record` (SuperGATConv keeps the record of its last
    forward): {'pos': bool [E'] in forward CSR slot order, 'drop': bool [E', H] (True = kept), 'neg': int64 [2, n_neg],
    'valid': bool [n_neg], 'src' / 'dst': int64 [E'] endpoints of every forward CSR slot}."""
    csr = graph.fwd
    dev = csr.rowptr.device
    nnz = csr.nnz
    pos = torch.empty(nnz, dtype=torch.uint8, device=dev)
    drop = torch.empty((nnz, H), dtype=torch.uint8, device=dev)
    _lib.launch("rgbx_supergat_draws_u8", record["seed"], nnz, H, float(record["p_drop"]), float(record["pos_ratio"]), pos,
                drop)
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(csr.N, device=dev), deg)
    valid = record["valid"]
    return {"pos": pos.bool(), "drop": drop.bool(), "neg": record["neg"],
            "valid": torch.ones(record["neg"].size(1), dtype=torch.bool, device=dev) if valid is None else valid.bool(),
            "src": csr.col[:nnz].long(), "dst": dst}


class _SuperGATAttend(torch.autograd.Function):
    """One SuperGATConv ('MX') attention block as a single autograd node: fused score + edge-softmax + aggregation
    (+ attention dropout + the positive half of the link-prediction loss in training mode), the negative sampler and
    the negative half of the loss; backward = target-side pass, source-side pass, negative scatter, attention-vector
    sums. Returns (out [N, H*C], att_loss scalar)."""

    @staticmethod
    def forward(ctx, hfeat, att_l, att_r, graph, H, C, slope, bias, train, p_drop, pos_ratio, neg_ratio, neg_edge_index,
                record):
        _lib.require_device(hfeat, att_l, att_r, bias, neg_edge_index)
        hfeat = _rows_on_grid(hfeat.contiguous(), _head_vec(C))
        b = _vec_on_grid(bias, H * C)
        al = _vec_on_grid(att_l, H * C).view(H, C)
        ar = _vec_on_grid(att_r, H * C).view(H, C)
        csr, N, dev = graph.fwd, graph.fwd.N, hfeat.device
        if hfeat.size(0) != N:
            raise RuntimeError(f"supergat_attend: {hfeat.size(0)} feature rows for a graph of {N} nodes")
        out = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        m = torch.empty((N, H), dtype=torch.float32, device=dev)
        rden = torch.empty_like(m)
        hm = _lib.mat(hfeat, "hfeat")
        split, _scratch = csr.split_arg(H * C + 2 * H, dev)
        seed = records = pos_stats = None
        n_rec = 0
        if train:
            # two 32-bit words from torch's device generator (torch.manual_seed makes the run repeatable); they stay
            # on the device: every kernel reads them there
            seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
            cnt = ctypes.c_int64(0)
            _lib.call("rgbx_supergat_loss_records", N, split, ctypes.byref(cnt))
            n_rec = max(cnt.value, 8192)
            records = torch.empty((n_rec, 2), dtype=torch.float32, device=dev)
            pos_stats = torch.empty(2, dtype=torch.float64, device=dev)
        _launch("supergat_fwd", "rgbx_supergat_aggregate_fwd_f32", csr.rowptr, csr.col, hm, al, ar, b, _lib.mat(out, "out"),
                m, rden, N, H, C, float(slope), seed, float(p_drop), float(pos_ratio), records, n_rec, pos_stats, split)
        ctx.train = train
        ctx.graph, ctx.H, ctx.C, ctx.slope = graph, H, C, slope
        ctx.att_shapes = (att_l.shape, att_r.shape)
        ctx.bias_shape = None if bias is None else bias.shape
        ctx.rng = (float(p_drop), float(pos_ratio))
        if not train:
            ctx.save_for_backward(hfeat, al, ar, b, m, rden, out)
            loss = torch.zeros((), dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(loss)
            return out, loss
        if neg_edge_index is None:
            n_neg = int(neg_ratio * pos_ratio * csr.nnz)
            neg, valid = supergat_sample_negatives(graph, seed, n_neg)
        else:
            neg, valid = neg_edge_index.contiguous(), None
            n_neg = neg.size(1)
        neg_stats = torch.empty(2, dtype=torch.float64, device=dev)
        _launch("supergat_neg_fwd", "rgbx_supergat_neg_loss_fwd_f32", hm, neg, valid, n_neg, H, C, records, n_rec, neg_stats)
        terms = (pos_stats[1] + neg_stats[1]).clamp(min=1.0)
        loss = ((pos_stats[0] + neg_stats[0]) / terms).to(torch.float32)
        if record is not None:
            record.update(seed=seed, neg=neg, valid=valid, p_drop=float(p_drop), pos_ratio=float(pos_ratio),
                          pos_stats=pos_stats, neg_stats=neg_stats)
        ctx.save_for_backward(hfeat, al, ar, b, m, rden, out, seed, neg, valid, terms)
        return out, loss

    @staticmethod
    def backward(ctx, gout, g_loss):
        train = ctx.train
        if train:
            hfeat, al, ar, b, m, rden, out, seed, neg, valid, terms = ctx.saved_tensors
        else:
            hfeat, al, ar, b, m, rden, out = ctx.saved_tensors
            seed = neg = valid = None
        g, H, C, slope = ctx.graph, ctx.H, ctx.C, ctx.slope
        p_drop, pos_ratio = ctx.rng
        N, dev = g.fwd.N, hfeat.device
        gout = torch.zeros_like(out) if gout is None else _rows_on_grid(gout.contiguous(), _head_vec(C))
        gl = None
        if train:
            gl = (torch.zeros((), device=dev) if g_loss is None else g_loss.to(torch.float64) / terms).to(
                torch.float32).reshape(1).contiguous()
        nodeq = torch.empty((N, H, 4), dtype=torch.float32, device=dev)
        g_h = torch.empty_like(hfeat)
        g_ar = torch.empty((N, H), dtype=torch.float32, device=dev)
        g_al = torch.empty_like(g_ar)
        hm, gm, ghm = _lib.mat(hfeat, "hfeat"), _lib.mat(gout, "gout"), _lib.mat(g_h, "g_hfeat")
        split, _scratch = g.fwd.split_arg(H * C + H, dev)
        _launch("supergat_bwd_dst", "rgbx_supergat_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, hm, al, ar, m, rden,
                _lib.mat(out, "out"), b, gm, nodeq, ghm, g_ar, N, H, C, float(slope), seed, p_drop, pos_ratio, gl, split)
        split, _scratch2 = g.bwd.split_arg(H * C + H, dev)
        _launch("supergat_bwd_src", "rgbx_supergat_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.t2f if train else None, hm, al,
                nodeq, gm, ghm, g_al, N, H, C, float(slope), seed, p_drop, pos_ratio, gl, split)
        if train and neg.size(1):
            _launch("supergat_neg_bwd", "rgbx_supergat_neg_loss_bwd_f32", hm, neg, valid, neg.size(1), H, C, gl, ghm)
        n_scr = ctypes.c_int64(0)
        _lib.call("rgbx_gat_scores_bwd_scratch_floats", N, H, C, ctypes.byref(n_scr))
        scratch = torch.empty(n_scr.value, dtype=torch.float32, device=dev)
        g_att_l = torch.empty((H, C), dtype=torch.float32, device=dev)
        g_att_r = torch.empty_like(g_att_l)
        # g_att_l = sum_j g_al[j] h_j, g_att_r = sum_i g_ar[i] h_i, in workgroup order
        _launch("supergat_att_bwd", "rgbx_gat_scores_bwd_f32", hm, g_al, g_ar, N, al, ar, None, 0, g_att_l, g_att_r, scratch,
                n_scr.value, N, H, C)
        g_b = gout.sum(0).reshape(ctx.bias_shape) if b is not None and ctx.needs_input_grad[7] else None
        return (g_h, g_att_l.reshape(ctx.att_shapes[0]), g_att_r.reshape(ctx.att_shapes[1]), None, None, None, None, g_b,
                None, None, None, None, None, None)


def supergat_supported(H, C):
    return bool(_lib.load().rgbx_supergat_supported(H, C))


def supergat_attend(h, att_l, att_r, graph, H, C, slope=0.2, bias=None, training=False, p_drop=0.0, pos_ratio=1.0,
                    neg_ratio=0.5, neg_edge_index=None, record=None):
    """(out, att_loss) of one SuperGATConv with 'MX' attention on h = x W^T [N, H*C]. In training mode the layer draws
    its attention dropout, its positive sample and (unless `neg_edge_index` int64 [2, n] is given) its negative pairs
    from a seed taken from torch's device generator; `record` (a dict) receives that seed and the pairs, for
    supergat_random_choices. att_loss is 0 outside training mode."""
    if _is_dist(graph):
        raise RuntimeError("SuperGATConv has no node-partitioned form: run it on one GPU")
    if not supergat_supported(H, C):
        raise RuntimeError(f"supergat_attend: {H} heads of {C} channels; pad the head width (SuperGATConv does)")
    if neg_edge_index is not None and training:
        if neg_edge_index.dtype != torch.int64 or neg_edge_index.dim() != 2 or neg_edge_index.size(0) != 2:
            raise RuntimeError("neg_edge_index must be int64 [2, n]")
        if neg_edge_index.numel() and (int(neg_edge_index.min()) < 0 or int(neg_edge_index.max()) >= graph.N):
            raise RuntimeError(f"neg_edge_index values outside [0, {graph.N})")
    return _SuperGATAttend.apply(h, att_l, att_r, graph, H, C, slope, bias, bool(training), p_drop, pos_ratio, neg_ratio,
                                 neg_edge_index, record)


def gatv2_random_choices(record, graph, H):
    """The attention-dropout decisions of the training forward that filled `record` (GATv2Conv keeps the record of its
    last forward): {'keep': bool [E', H] in forward CSR slot order (True = kept), 'src' / 'dst': int64 [E'] endpoints of
    every forward CSR slot}."""
    csr = graph.fwd
    dev, nnz = csr.rowptr.device, csr.nnz
    if record.get("seed") is None:
        keep = torch.ones((nnz, H), dtype=torch.uint8, device=dev)
    else:
        keep = torch.empty((nnz, H), dtype=torch.uint8, device=dev)
        _lib.launch("rgbx_gatv2_draws_u8", record["seed"], nnz, H, float(record["p_drop"]), keep)
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    return {"keep": keep.bool(), "src": csr.col[:nnz].long(),
            "dst": torch.repeat_interleave(torch.arange(csr.N, device=dev), deg)}


class _GATv2Attend(torch.autograd.Function):
    """One GATv2Conv attention block as a single autograd node: fused score + edge-softmax + aggregation (+ attention
    dropout in training mode); backward = target-side pass (g_xr, g_att), source-side pass (g_xl). Saves xl, xr, att,
    out, m / rden [N, H] and the dropout seed; nothing per edge (the backward recomputes scores and keep bits)."""

    @staticmethod
    def forward(ctx, xl, xr, att, graph, H, C, slope, bias, train, p_drop, record, want_grad):
        _lib.require_device(xl, xr, att, bias)
        # column blocks of one product stay views, where the widest head still fits a wave at the vector width they allow
        xl, xr = _rows_on_grid(xl, _head_vec(C)), _rows_on_grid(xr, _head_vec(C))
        b = _vec_on_grid(bias, H * C)
        a = _vec_on_grid(att, H * C)
        csr, N, dev = graph.fwd, graph.fwd.N, xl.device
        if xl.size(0) != N or xr.size(0) != N or xl.size(1) != H * C or xr.size(1) != H * C:
            raise RuntimeError(f"gatv2_attend: xl {tuple(xl.shape)} / xr {tuple(xr.shape)} for a graph of {N} nodes and "
                               f"{H} x {C} channels")
        seed = None
        if train and p_drop > 0.0:
            # two 32-bit words from torch's device generator (torch.manual_seed makes the run repeatable; under a
            # hipGraph capture the generator's offset advances with every replay); they stay on the device
            seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
        if record is not None:
            record.update(seed=seed, p_drop=float(p_drop))
        out = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        # m / rden are the backward's; without one the kernel runs its inference form
        m = torch.empty((N, H), dtype=torch.float32, device=dev) if want_grad or seed is not None else None
        rden = None if m is None else torch.empty_like(m)
        split, _scratch = csr.split_arg(H * C + 2 * H, dev)
        _launch("gatv2_fwd", "rgbx_gatv2_fwd_f32", csr.rowptr, csr.col, _lib.mat(xl, "xl"), _lib.mat(xr, "xr"), a, b,
                _lib.mat(out, "out"), m, rden, N, H, C, float(slope), seed, float(p_drop), split)
        ctx.graph, ctx.H, ctx.C, ctx.slope, ctx.p_drop = graph, H, C, float(slope), float(p_drop)
        ctx.att_shape = att.shape
        ctx.bias_shape = None if bias is None else bias.shape
        ctx.save_for_backward(xl, xr, a, b, m, rden, out, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        xl, xr, a, b, m, rden, out, seed = ctx.saved_tensors
        g, H, C, slope, p_drop = ctx.graph, ctx.H, ctx.C, ctx.slope, ctx.p_drop
        N, dev = g.fwd.N, xl.device
        F = H * C
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        nodeq = torch.empty((N, H, 2), dtype=torch.float32, device=dev)
        g_xl = torch.empty((N, F), dtype=torch.float32, device=dev)
        g_xr = torch.empty_like(g_xl)
        g_att = torch.empty(F, dtype=torch.float32, device=dev)
        lm, rm, gm = _lib.mat(xl, "xl"), _lib.mat(xr, "xr"), _lib.mat(gout, "gout")
        split, _scratch = g.fwd.split_arg(F, dev)
        n_part = ctypes.c_int64(0)
        _lib.call("rgbx_gatv2_att_partial_floats", N, H, C, split, ctypes.byref(n_part))
        part = torch.empty(max(n_part.value, 1), dtype=torch.float32, device=dev)
        _launch("gatv2_bwd_dst", "rgbx_gatv2_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, lm, rm, a, m, rden, _lib.mat(out, "out"),
                b, gm, nodeq, _lib.mat(g_xr, "g_xr"), g_att, part, n_part.value, N, H, C, slope, seed, p_drop, split)
        split, _scratch2 = g.bwd.split_arg(F, dev)
        _launch("gatv2_bwd_src", "rgbx_gatv2_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.t2f if seed is not None else None, lm,
                rm, a, nodeq, gm, _lib.mat(g_xl, "g_xl"), N, H, C, slope, seed, p_drop, split)
        need = ctx.needs_input_grad
        g_b = gout.sum(0).reshape(ctx.bias_shape) if b is not None and need[7] else None
        return (g_xl if need[0] else None, g_xr if need[1] else None, g_att.reshape(ctx.att_shape) if need[2] else None,
                None, None, None, None, g_b, None, None, None, None)


def gatv2_supported(H, C):
    return bool(_lib.load().rgbx_gatv2_supported(H, C))


def gatv2_attend(xl, xr, att, graph, H, C, slope=0.2, bias=None, training=False, p_drop=0.0, record=None):
    """One GATv2Conv attention block on xl = lin_l(x), xr = lin_r(x) [N, H*C] (rows contiguous; column blocks of one
    wider matrix are taken as they are) and att [H*C]: out_i = sum_j softmax_i(sum_c att_c lrelu(xl_j + xr_i)_c) xl_j
    (+ bias [H*C]) over the graph in mode LOOPS_REMOVE_ADD. In training mode with p_drop > 0 the coefficients are
    dropped after the softmax with a seed from torch's device generator; `record` (a dict) receives it, for
    gatv2_random_choices."""
    if _is_dist(graph):
        raise RuntimeError("GATv2Conv has no node-partitioned form: run it on one GPU")
    _lib.require_device(xl, xr, att, bias)
    if not (0.0 <= p_drop < 1.0):
        raise ValueError("gatv2_attend: dropout must be in [0, 1)")
    if not gatv2_supported(H, C):
        raise RuntimeError(f"gatv2_attend: {H} heads of {C} channels; pad the head width (GATv2Conv does)")
    want_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xl, xr, att, bias))
    return _GATv2Attend.apply(xl, xr, att, graph, H, C, float(slope), bias, bool(training), float(p_drop), record,
                              want_grad)


def transformer_random_choices(record, graph, H):
    """The attention-dropout decisions of the training forward that filled `record` (TransformerConv keeps the record
    of its last forward): {'keep': bool [E, H] in forward CSR slot order (True = kept), 'src' / 'dst': int64 [E]
    endpoints of every forward CSR slot}. The keep hash is GATv2's, so its inspection entry point serves."""
    return gatv2_random_choices(record, graph, H)


class _TransformerAttend(torch.autograd.Function):
    """One TransformerConv attention block as a single autograd node: fused scaled dot-product score + edge-softmax +
    aggregation of the value rows (+ attention dropout in training mode); backward = target-side pass (g_q and the
    per-node record), source-side pass (g_k, g_v). Saves q, k, v, out, m / rden [N, H] and the dropout seed; nothing
    per edge (the backward recomputes scores and keep bits)."""

    @staticmethod
    def forward(ctx, q, k, v, graph, H, C, scale, train, p_drop, record, want_grad):
        _lib.require_device(q, k, v)
        # column blocks of one product stay views, where the widest head still fits a wave at the vector width they allow
        q, k, v = (_rows_on_grid(t, _head_vec(C)) for t in (q, k, v))
        csr, N, dev = graph.fwd, graph.fwd.N, q.device
        if any(t.size(0) != N or t.size(1) != H * C for t in (q, k, v)):
            raise RuntimeError(f"transformer_attend: q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} for a "
                               f"graph of {N} nodes and {H} x {C} channels")
        seed = None
        if train and p_drop > 0.0:
            # two 32-bit words from torch's device generator, as _GATv2Attend draws them; they stay on the device
            seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
        if record is not None:
            record.update(seed=seed, p_drop=float(p_drop))
        out = torch.empty((N, H * C), dtype=torch.float32, device=dev)
        # m / rden are the backward's; without one the kernel runs its inference form
        m = torch.empty((N, H), dtype=torch.float32, device=dev) if want_grad or seed is not None else None
        rden = None if m is None else torch.empty_like(m)
        split, _scratch = csr.split_arg(H * C + 2 * H, dev)
        _launch("transformer_fwd", "rgbx_transformer_fwd_f32", csr.rowptr, csr.col, _lib.mat(q, "q"), _lib.mat(k, "k"),
                _lib.mat(v, "v"), _lib.mat(out, "out"), m, rden, N, H, C, float(scale), seed, float(p_drop), split)
        ctx.graph, ctx.H, ctx.C, ctx.scale, ctx.p_drop = graph, H, C, float(scale), float(p_drop)
        ctx.save_for_backward(q, k, v, m, rden, out, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, m, rden, out, seed = ctx.saved_tensors
        g, H, C, scale, p_drop = ctx.graph, ctx.H, ctx.C, ctx.scale, ctx.p_drop
        N, dev = g.fwd.N, q.device
        F = H * C
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        # every row of the four buffers is written by the kernels (rows without slots as zeros)
        nodeq = torch.empty((N, H, 2), dtype=torch.float32, device=dev)
        g_q = torch.empty((N, F), dtype=torch.float32, device=dev)
        g_k = torch.empty_like(g_q)
        g_v = torch.empty_like(g_q)
        qm, km, vm, gm = _lib.mat(q, "q"), _lib.mat(k, "k"), _lib.mat(v, "v"), _lib.mat(gout, "gout")
        split, _scratch = g.fwd.split_arg(F, dev)
        _launch("transformer_bwd_dst", "rgbx_transformer_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, qm, km, vm, m, rden,
                _lib.mat(out, "out"), gm, nodeq, _lib.mat(g_q, "g_q"), N, H, C, scale, seed, p_drop, split)
        split, _scratch2 = g.bwd.split_arg(2 * F, dev)
        _launch("transformer_bwd_src", "rgbx_transformer_bwd_src_f32", g.bwd.rowptr, g.bwd.col,
                g.t2f if seed is not None else None, qm, km, vm, nodeq, gm, _lib.mat(g_k, "g_k"), _lib.mat(g_v, "g_v"),
                N, H, C, scale, seed, p_drop, split)
        need = ctx.needs_input_grad
        return (g_q if need[0] else None, g_k if need[1] else None, g_v if need[2] else None, None, None, None, None,
                None, None, None, None)


def transformer_supported(H, C):
    return bool(_lib.load().rgbx_transformer_supported(H, C))


def transformer_attend(q, k, v, graph, H, C, scale, training=False, p_drop=0.0, record=None):
    """One TransformerConv attention block on q, k, v [N, H*C] (rows contiguous; column blocks of one wider matrix are
    taken as they are): out_i = sum_j softmax_i(<q_i, k_j> * scale) v_j per head over the in-edges of i, the graph in
    mode LOOPS_KEEP (edges as given; a node without in-edges gets zeros). `scale` is 1 / sqrt(C) of the TRUE head
    width (the caller may have zero-padded the heads). In training mode with p_drop > 0 the coefficients are dropped
    after the softmax with a seed from torch's device generator; `record` (a dict) receives it, for
    transformer_random_choices."""
    if _is_dist(graph):
        raise RuntimeError("TransformerConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(q, k, v)
    if not (0.0 <= p_drop < 1.0):
        raise ValueError("transformer_attend: dropout must be in [0, 1)")
    if not transformer_supported(H, C):
        raise RuntimeError(f"transformer_attend: {H} heads of {C} channels; pad the head width (TransformerConv does)")
    want_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    return _TransformerAttend.apply(q, k, v, graph, H, C, float(scale), bool(training), float(p_drop), record,
                                    want_grad)


class _ResGatedAggregate(torch.autograd.Function):
    """One ResGatedGraphConv aggregation as a single autograd node: fused per-channel gate sigmoid(k_i + q_j) and sum
    of the gated value rows; backward = target-side pass (g_k) and source-side pass (g_q, g_v), independent of each
    other and run only where a gradient is asked for. Saves k, q, v and nothing else: no output, no per-node state,
    nothing per edge (both passes recompute the gate)."""

    @staticmethod
    def forward(ctx, k, q, v, graph):
        _lib.require_device(k, q, v)
        C = k.size(1)
        # column blocks of one product stay views, where the row still fits a wave at the vector width they allow
        k, q, v = (_rows_on_grid(t, _head_vec(C)) for t in (k, q, v))
        csr, N, dev = graph.fwd, graph.fwd.N, k.device
        if any(t.dim() != 2 or t.size(0) != N or t.size(1) != C for t in (k, q, v)):
            raise RuntimeError(f"resgated_aggregate: k {tuple(k.shape)} / q {tuple(q.shape)} / v {tuple(v.shape)} for a "
                               f"graph of {N} nodes")
        out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (rows without slots: zeros)
        split, _scratch = csr.split_arg(C, dev)
        _launch("resgated_fwd", "rgbx_resgated_fwd_f32", csr.rowptr, csr.col, _lib.mat(k, "k"), _lib.mat(q, "q"),
                _lib.mat(v, "v"), _lib.mat(out, "out"), N, C, split)
        ctx.graph = graph
        ctx.save_for_backward(k, q, v)
        return out

    @staticmethod
    def backward(ctx, gout):
        k, q, v = ctx.saved_tensors
        g = ctx.graph
        N, C, dev = g.fwd.N, k.size(1), k.device
        need = ctx.needs_input_grad
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        km, qm, vm, gm = _lib.mat(k, "k"), _lib.mat(q, "q"), _lib.mat(v, "v"), _lib.mat(gout, "gout")
        g_k = g_q = g_v = None
        if need[0]:
            g_k = torch.empty((N, C), dtype=torch.float32, device=dev)
            split, _scratch = g.fwd.split_arg(C, dev)
            _launch("resgated_bwd_dst", "rgbx_resgated_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, km, qm, vm, gm,
                    _lib.mat(g_k, "g_k"), N, C, split)
        if need[1] or need[2]:  # one pass forms both sums from the same two gathered rows
            g_q = torch.empty((N, C), dtype=torch.float32, device=dev)
            g_v = torch.empty_like(g_q)
            split, _scratch2 = g.bwd.split_arg(2 * C, dev)
            _launch("resgated_bwd_src", "rgbx_resgated_bwd_src_f32", g.bwd.rowptr, g.bwd.col, km, qm, vm, gm,
                    _lib.mat(g_q, "g_q"), _lib.mat(g_v, "g_v"), N, C, split)
        return g_k, g_q if need[1] else None, g_v if need[2] else None, None


def resgated_supported(C):
    return bool(_lib.load().rgbx_resgated_supported(C))


def resgated_aggregate(k, q, v, graph):
    """One ResGatedGraphConv aggregation on k, q, v [N, C] (rows contiguous; column blocks of one wider matrix are taken
    as they are): out_i = sum_j sigmoid(k_i + q_j) * v_j, elementwise over the C channels, over the in-edges of i, the
    graph in mode LOOPS_KEEP (edges as given: self-loops stay, duplicates count twice, a node without in-edges gets
    zeros). No normalisation, no dropout, no random state."""
    if _is_dist(graph):
        raise RuntimeError("ResGatedGraphConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(k, q, v)
    if k.dim() != 2 or not resgated_supported(k.size(1)):
        raise RuntimeError(f"resgated_aggregate: k {tuple(k.shape)}: the kernels take [N, C] with any C <= 64, even "
                           "C <= 128 or C % 4 == 0 up to 256; pad the width (ResGatedGraphConv does)")
    return _ResGatedAggregate.apply(k, q, v, graph)


_EDGE_SLOTS_MAX = 4  # cached slot-ordered copies per graph (each is an [E, D] matrix)


def _slot_to_edge(graph):
    """(perm, inv) of a LOOPS_KEEP graph: perm [E] the input edge of every forward CSR slot, inv [E] the slot of every
    input edge (perm is a permutation there: nothing is added, nothing coalesced). Built once per graph."""
    cached = graph.__dict__.get("_slot_to_edge")
    if cached is None:
        perm = graph.fwd.perm[:graph.fwd.nnz]
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
        cached = graph._slot_to_edge = (perm.contiguous(), inv)
    return cached


class _EdgeRowsToSlots(torch.autograd.Function):
    """edge_attr[perm] through rgbx_gather_rows_f32; the backward is the gather through the inverse permutation (every
    input edge owns exactly one slot, so nothing is added: no atomics)."""

    @staticmethod
    def forward(ctx, edge_attr, graph):
        ctx.graph = graph
        return gather_rows(edge_attr.contiguous(), _slot_to_edge(graph)[0])

    @staticmethod
    def backward(ctx, gout):
        return gather_rows(gout.contiguous(), _slot_to_edge(ctx.graph)[1]), None


def edge_rows_to_slots(edge_attr, graph):
    """edge_attr [E, D] (one row per INPUT edge, float32) as [E, D] in forward CSR slot order: row p is the attribute row
    of the edge in slot p, edge_attr[perm[p]]. Only for graphs in mode LOOPS_KEEP, where every input edge owns exactly one
    slot (nnz == E, perm a permutation); any other mode raises. An attribute matrix that does not require grad is
    permuted once per (storage, shape, in-place version) and the result kept on the graph; one that does is permuted by a
    differentiable gather on every call (backward: the gather through the inverse permutation, no atomics). The
    permutation happens at the raw width D: a layer's Linear over the result yields its per-slot rows directly."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("edge attributes have no node-partitioned form: run it on one GPU")
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("edge_rows_to_slots: only a graph in mode LOOPS_KEEP maps every input edge to exactly one CSR "
                           f"slot (got loops_mode={getattr(graph, 'loops_mode', None)!r})")
    if edge_attr.dim() != 2 or edge_attr.size(0) != graph.E or edge_attr.dtype != torch.float32:
        raise RuntimeError(f"edge_rows_to_slots: edge_attr {edge_attr.dtype} {tuple(edge_attr.shape)} for a graph of "
                           f"{graph.E} edges (float32 [E, D])")
    if graph.fwd.nnz != graph.E:
        raise RuntimeError(f"edge_rows_to_slots: {graph.fwd.nnz} CSR slots for {graph.E} input edges")
    if graph.E == 0:
        return edge_attr[:0]
    if edge_attr.requires_grad and torch.is_grad_enabled():
        return _EdgeRowsToSlots.apply(edge_attr, graph)
    cache = graph.__dict__.setdefault("_edge_slots", {})
    key = (edge_attr.data_ptr(), tuple(edge_attr.shape), edge_attr._version)
    hit = cache.get(key)
    if hit is None:
        # the key holds the attribute's data_ptr: keep its storage alive beside the permuted copy
        hit = cache[key] = (edge_attr, gather_rows(edge_attr.detach().contiguous(), _slot_to_edge(graph)[0]))
        while len(cache) > _EDGE_SLOTS_MAX:
            cache.pop(next(iter(cache)))
    return hit[1]


class _GINEAggregate(torch.autograd.Function):
    """One GINEConv aggregation as a single autograd node: fused message relu(x_j + e_p), sum over the in-edges and root
    term (1 + eps) x_i; backward = edge-side pass (g_e, one row per slot), source-side pass (g_x) and, for a trained
    eps, g_eps = sum_i <gout_i, x_i> (dense per-node work, on torch), each run only where a gradient is asked for. Saves
    x, e and eps and nothing else: every pass recomputes the mask from the forward's own add. The kernels read eps from
    device memory, so a captured launch follows an eps the optimizer moves."""

    @staticmethod
    def forward(ctx, x, e_slot, eps, graph):
        _lib.require_device(x, e_slot, eps)
        C = x.size(1)
        # column blocks of a wider matrix stay views, where the row still fits a wave at the vector width they allow
        x, e = (_rows_on_grid(t, _head_vec(C)) for t in (x, e_slot))
        csr, N, dev = graph.fwd, graph.fwd.N, x.device
        epsv = None if eps is None else eps.detach().reshape(-1).contiguous()
        if csr.nnz == 0:  # no slot row is ever read: a pointer the entry point accepts
            e = torch.empty((1, C), dtype=torch.float32, device=dev)
        out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (rows without slots: the root)
        split, _scratch = csr.split_arg(C, dev)
        _launch("gine_fwd", "rgbx_gine_fwd_f32", csr.rowptr, csr.col, _lib.mat(x, "x"), _lib.mat(e, "e_slot"), epsv,
                _lib.mat(out, "out"), N, C, split)
        ctx.graph, ctx.eps_shape = graph, None if eps is None else eps.shape
        ctx.save_for_backward(x, e, epsv)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, e, epsv = ctx.saved_tensors
        g = ctx.graph
        N, C, dev = g.fwd.N, x.size(1), x.device
        need = ctx.needs_input_grad
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        xm, em, gm = _lib.mat(x, "x"), _lib.mat(e, "e_slot"), _lib.mat(gout, "gout")
        g_x = g_e = g_eps = None
        if need[1]:
            nnz = g.fwd.nnz
            g_e = torch.empty((nnz, C), dtype=torch.float32, device=dev)  # every slot row is written
            if nnz:
                split, _scratch = g.fwd.split_arg(1, dev)  # the plan only: this pass leaves no chunk record
                _launch("gine_bwd_edge", "rgbx_gine_bwd_edge_f32", g.fwd.rowptr, g.fwd.col, xm, em, gm,
                        _lib.mat(g_e, "g_e"), N, C, split)
        if need[0]:
            g_x = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (no out-edge: the root)
            split, _scratch2 = g.bwd.split_arg(C, dev)
            _launch("gine_bwd_src", "rgbx_gine_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.t2f, xm, em, gm, epsv,
                    _lib.mat(g_x, "g_x"), N, C, split)
        if epsv is not None and need[2]:
            g_eps = (gout * x).sum().reshape(ctx.eps_shape)
        return g_x, g_e, g_eps, None


def gine_supported(C):
    return bool(_lib.load().rgbx_gine_supported(C))


GINE_BLOCK = 256  # wider inputs run as column blocks of this many channels


def gine_aggregate(x, e_slot, graph, eps=None):
    """One GINEConv aggregation on x [N, C] and e_slot [nnz, C], one row per forward CSR slot (edge_rows_to_slots gives
    the order; rows contiguous, column blocks of a wider matrix are taken as they are):
    out_i = (1 + eps) x_i + sum_p relu(x_j + e_p) over the in-edges of i, the graph in mode LOOPS_KEEP (edges as given:
    self-loops stay, duplicates count twice, a node without in-edges gets the root term alone). `eps`: a one-element
    float32 tensor on x's device (it may take a gradient), or None for no root term. relu'(0) = 0. Widths above 256 run
    as column blocks of 256: the message is per channel, so nothing couples columns. No dropout, no random state."""
    if _is_dist(graph):
        raise RuntimeError("GINEConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(x, e_slot, eps)
    N, nnz = graph.fwd.N, graph.fwd.nnz
    if x.dim() != 2 or e_slot.dim() != 2 or x.size(0) != N or tuple(e_slot.shape) != (nnz, x.size(1)):
        raise RuntimeError(f"gine_aggregate: x {tuple(x.shape)} / e_slot {tuple(e_slot.shape)} for a graph of {N} nodes "
                           f"and {nnz} slots (x [N, C], e_slot [nnz, C])")
    if eps is not None and (eps.numel() != 1 or eps.dtype != torch.float32):
        raise RuntimeError(f"gine_aggregate: eps {eps.dtype} {tuple(eps.shape)} (one float32)")
    C = x.size(1)
    if C > GINE_BLOCK and gine_supported(C % GINE_BLOCK or GINE_BLOCK):  # (else: refused below, before any launch)
        return torch.cat([_GINEAggregate.apply(x[:, a:a + GINE_BLOCK], e_slot[:, a:a + GINE_BLOCK], eps, graph)
                          for a in range(0, C, GINE_BLOCK)], dim=1)
    if not gine_supported(C):
        raise RuntimeError(f"gine_aggregate: x {tuple(x.shape)}: the kernels take [N, C] with any C <= 64, even "
                           "C <= 128 or C % 4 == 0 up to 256 (and blocks of 256 above); pad the width (GINEConv does)")
    return _GINEAggregate.apply(x, e_slot, eps, graph)


# ---- CGConv: sigmoid(lin_f(z)) * softplus(lin_s(z)) with z = [x_i, x_j, e_ij], as three linear terms -----------------

class _CGConvAggregate(torch.autograd.Function):
    """One CGConv aggregation as a single autograd node: fused message sigmoid(zf) * softplus(zs) with
    z = a_i + b_j + c_p, sum or mean over the in-edges and root term; backward = target-side pass (g_a and, from the same
    registers, g_c, one row per slot) and source-side pass (g_b), independent of each other and run only where a gradient
    is asked for; g_root = gout. Saves a, b, c and nothing else (of root only whether it was there): both passes recompute
    both branches. The mean's 1 / deg is read from rowptr inside the kernels, so a captured launch stays valid."""

    @staticmethod
    def forward(ctx, a, b, c_slot, root, graph, C, mean):
        _lib.require_device(a, b, c_slot, root)
        # column blocks of one product stay views, where the row still fits a wave at the vector width they allow
        vec = _head_vec(C)
        a, b = (_rows_on_grid(t, vec) for t in (a, b))
        csr, N, dev = graph.fwd, graph.fwd.N, a.device
        c = None
        if c_slot is not None and csr.nnz:  # (no slot: no c row is ever read, the call runs without the edge term)
            c = _rows_on_grid(c_slot, vec)
        rt = None if root is None else _rows_on_grid(root, vec)
        out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (rows without slots: the root)
        split, _scratch = csr.split_arg(C, dev)
        _launch("cgconv_fwd", "rgbx_cgconv_fwd_f32", csr.rowptr, csr.col, _lib.mat(a, "a"), _lib.mat(b, "b"),
                _lib.mat_opt(c, "c_slot"), _lib.mat_opt(rt, "root"), _lib.mat(out, "out"), N, C, int(mean), split)
        ctx.graph, ctx.C, ctx.mean = graph, C, mean
        ctx.c_shape = None if c_slot is None else tuple(c_slot.shape)
        ctx.save_for_backward(a, b, c)
        return out

    @staticmethod
    def backward(ctx, gout):
        a, b, c = ctx.saved_tensors
        g = ctx.graph
        N, C, dev, mean = g.fwd.N, ctx.C, a.device, int(ctx.mean)
        need = ctx.needs_input_grad
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        am, bm, cm, gm = _lib.mat(a, "a"), _lib.mat(b, "b"), _lib.mat_opt(c, "c_slot"), _lib.mat(gout, "gout")
        g_a = g_b = g_c = None
        want_c = need[2] and ctx.c_shape is not None
        if want_c:
            g_c = torch.empty(ctx.c_shape, dtype=torch.float32, device=dev)  # every slot row is written
        if need[0] or (want_c and g.fwd.nnz):  # one pass forms both from the same registers
            if need[0]:
                g_a = torch.empty((N, 2 * C), dtype=torch.float32, device=dev)  # every row is written
            split, _scratch = g.fwd.split_arg(2 * C, dev)
            _launch("cgconv_bwd_dst", "rgbx_cgconv_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, am, bm, cm, gm,
                    _lib.mat_opt(g_a, "g_a"), _lib.mat(g_c, "g_c") if want_c and g.fwd.nnz else (0, 0), N, C, mean, split)
        if need[1]:
            g_b = torch.empty((N, 2 * C), dtype=torch.float32, device=dev)  # every row is written
            split, _scratch2 = g.bwd.split_arg(2 * C, dev)
            _launch("cgconv_bwd_src", "rgbx_cgconv_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.t2f, g.fwd.rowptr, am, bm, cm, gm,
                    _lib.mat(g_b, "g_b"), N, C, mean, split)
        return g_a, g_b, g_c, gout if need[3] else None, None, None, None


def cgconv_supported(C):
    return bool(_lib.load().rgbx_cgconv_supported(C))


def cgconv_aggregate(a, b, c_slot, graph, C, aggr="add", root=None):
    """One CGConv aggregation on a, b [N, 2C] and c_slot [nnz, 2C] or None, every row (f half | s half); c_slot has one
    row per forward CSR slot (edge_rows_to_slots gives the order). Rows contiguous; column blocks of one wider matrix are
    taken as they are. With zf = a_f[i] + b_f[j] + c_f[p] and zs likewise:
    out_i = root_i + aggr_p sigmoid(zf) * softplus(zs), elementwise over the C channels, over the in-edges of i, the graph
    in mode LOOPS_KEEP (edges as given: self-loops stay, duplicates count twice, a node without in-edges gets the root
    term alone). aggr: "add" or "mean" (the division by the in-edge count). root [N, C] or None. No dropout, no random
    state."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("CGConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(a, b, c_slot, root)
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("cgconv_aggregate: the graph must be in mode LOOPS_KEEP (edges as given; got "
                           f"loops_mode={getattr(graph, 'loops_mode', None)!r})")
    if aggr not in ("add", "mean"):
        raise NotImplementedError(f"cgconv_aggregate: aggr={aggr!r} (the kernels form sums: 'add' or 'mean')")
    N, nnz = graph.fwd.N, graph.fwd.nnz
    C = int(C)
    if (a.dim() != 2 or b.dim() != 2 or tuple(a.shape) != (N, 2 * C) or tuple(b.shape) != (N, 2 * C)
            or (c_slot is not None and tuple(c_slot.shape) != (nnz, 2 * C))
            or (root is not None and tuple(root.shape) != (N, C))):
        raise RuntimeError(f"cgconv_aggregate: a {tuple(a.shape)} / b {tuple(b.shape)} / c_slot "
                           f"{None if c_slot is None else tuple(c_slot.shape)} / root "
                           f"{None if root is None else tuple(root.shape)} for a graph of {N} nodes and {nnz} slots at "
                           f"C = {C} (a, b [N, 2C], c_slot [nnz, 2C], root [N, C])")
    if not cgconv_supported(C):
        raise RuntimeError(f"cgconv_aggregate: C = {C}: the kernels take any C <= 64, even C <= 128 or C % 4 == 0 up to "
                           "256; pad the width (CGConv does)")
    return _CGConvAggregate.apply(a, b, c_slot, root, graph, C, aggr == "mean")


# ---- PNAConv: the statistics of a per-edge message, scaled by functions of the in-degree -------------------------------

PNA_SCALERS = {"identity": 0, "amplification": 1, "attenuation": 2, "linear": 3, "inverse_linear": 4}  # RGBX_PNA_*
PNA_BLOCK = 256  # wider inputs run as column blocks of at most this many channels, cut at tower boundaries


def pna_scaler_names(scalers):
    """A name or a non-empty list / tuple of distinct scaler names as a tuple; anything else: ValueError."""
    seq = (scalers,) if isinstance(scalers, str) else scalers
    if (not isinstance(seq, (list, tuple)) or not seq or any(s not in PNA_SCALERS for s in seq)
            or len(set(seq)) != len(seq)):
        raise ValueError(f"scalers must name distinct scalers out of {sorted(PNA_SCALERS)}, got {scalers!r}")
    return tuple(seq)


def degree_averages(graph):
    """float32 [2] on the graph's device: [mean of deg, mean of log(deg + 1)] over the in-degrees of all nodes — PyG's
    avg_deg['lin'] and avg_deg['log'] of PNAConv's degree histogram (sum_k k hist[k] / sum_k hist[k], and the same with
    log(k + 1)). Computed where the CSR lives, once per graph, with no read-back. A graph without nodes gives zeros."""
    cached = graph.__dict__.get("_avg_deg")
    if cached is None:
        rowptr = graph.fwd.rowptr
        deg = (rowptr[1:] - rowptr[:-1]).to(torch.float64)
        if deg.numel() == 0:
            cached = torch.zeros(2, dtype=torch.float32, device=rowptr.device)
        else:
            cached = torch.stack([deg.mean(), torch.log(deg + 1).mean()]).to(torch.float32)
        graph._avg_deg = cached
    return cached


def pna_scales(graph, scalers, avg_deg):
    """float32 [N, S]: scale_s of every node (D = max(in-degree, 1)), torch's restatement of the kernel's epilogue for
    the dense per-node work of the backward."""
    rowptr = graph.fwd.rowptr
    D = (rowptr[1:] - rowptr[:-1]).to(torch.float32).clamp(min=1)
    logD = torch.log(D + 1)
    lin, log = avg_deg[0], avg_deg[1]
    cols = {"identity": lambda: torch.ones_like(D), "amplification": lambda: logD / log,
            "attenuation": lambda: log / logD, "linear": lambda: D / lin, "inverse_linear": lambda: lin / D}
    return torch.stack([cols[s]() for s in scalers], dim=1)


def _pna_blocks(d, F):
    """[(t0, t1)]: the towers of every launch, as many as fit into PNA_BLOCK channels."""
    per = max(PNA_BLOCK // F, 1)
    return [(t0, min(t0 + per, d // F)) for t0 in range(0, d // F, per)]


def pna_fwd_raw(csr, a, b, c, avg_deg, aggregators, scalers, F, keep=()):
    """(out [N, T*S*A*F], kept): rgbx_pna_fwd_f32 over `csr` on operands that are already on the vector grid (a, c may be
    None); `keep`: out of 'mean', 'var', 'std', 'argmax', 'argmin', the raw statistics of u stored beside (kept[name],
    [N, d]). No autograd, no checks beyond the entry point's."""
    names, scalers = multi_names(aggregators), pna_scaler_names(scalers)
    N, dev = csr.N, b.device
    d, S, A = b.size(1), len(scalers), len(names)
    if csr.nnz == 0:
        c = None  # no slot row is ever read
    avg = avg_deg.detach().reshape(-1).contiguous()
    out = torch.empty((N, (d // F) * S * A * F), dtype=torch.float32, device=dev)  # every row is written
    kept = {k: torch.empty((N, d), dtype=torch.int32 if k.startswith("arg") else torch.float32, device=dev) for k in keep}
    bits = sum(MULTI_BITS[n] for n in names)
    order = (ctypes.c_int32 * A)(*[MULTI_BITS[n] for n in names])
    kinds = (ctypes.c_int32 * S)(*[PNA_SCALERS[s] for s in scalers])
    for t0, t1 in _pna_blocks(d, F):
        c0, c1 = t0 * F, t1 * F
        w = c1 - c0
        o = _lib.PnaOut()
        o.out, o.ld_out = _block_ptr(out, t0 * S * A * F, t1 * S * A * F)
        for k, t in kept.items():
            p, ld = _block_ptr(t, c0, c1)
            setattr(o, k, p)
            setattr(o, "ld_" + k, ld)
        split, words = None, 0
        if csr.split is not None:
            n_words = ctypes.c_int64(0)
            _lib.call("rgbx_pna_partial_words", csr.split["n_chunks"], w,
                      bits | (MULTI_BITS["mean"] if "mean" in kept else 0), ctypes.byref(n_words))
            words = n_words.value
            split, _scratch = csr.split_arg(words // csr.split["n_chunks"], dev)
        variant = (f"rows+d{w}+{'+'.join(names)}x{S}" + ("+c" if c is not None else "") + ("+kept" if kept else "")
                   if _EVENT_SINK is not None else None)
        _launch("pna_fwd", "rgbx_pna_fwd_f32", csr.rowptr, csr.col, (0, 0) if a is None else _block_ptr(a, c0, c1),
                _block_ptr(b, c0, c1), (0, 0) if c is None else _block_ptr(c, c0, c1), avg, bits, order, kinds, S, o, N, w, F,
                split, words, variant=variant)
    return out, kept


def pna_bwd_raw(graph, terms, b, c, F, want_b=True, want_c=False):
    """(g_b [N, d] or None, g_c [nnz, d] or None): rgbx_pna_bwd_src_f32 over the transposed CSR and rgbx_pna_bwd_edge_f32
    over the forward one, each only where wanted. `terms`: the per-target rows A, B, gmax, argmax, gmin, argmin that are
    present ([N, d], on the vector grid); b and c are read with B alone (c may be None for the source pass). No autograd."""
    first = next(iter(terms.values()))
    N, d, dev = graph.fwd.N, first.size(1), first.device
    nnz = graph.fwd.nnz
    with_b = "B" in terms
    g_b = torch.empty((N, d), dtype=torch.float32, device=dev) if want_b else None  # every row is written
    g_c = torch.empty((nnz, d), dtype=torch.float32, device=dev) if want_c else None  # every slot row is written
    want_c = want_c and nnz > 0  # (no slot: the [0, d] gradient is complete as it is)
    if nnz == 0:
        c = None
    for t0, t1 in _pna_blocks(d, F) if (want_b or want_c) else ():
        c0, c1 = t0 * F, t1 * F
        w = c1 - c0
        t = _lib.PnaGrad()
        for k, v in terms.items():
            p, ld = _block_ptr(v, c0, c1)
            setattr(t, k, p)
            setattr(t, "ld_" + k, ld)
        bm = _block_ptr(b, c0, c1) if with_b else (0, 0)
        cm = _block_ptr(c, c0, c1) if (with_b and c is not None) else (0, 0)
        variant = f"rows+d{w}+{'+'.join(terms)}" + ("+c" if cm[0] else "") if _EVENT_SINK is not None else None
        if want_c:
            split, _scratch = graph.fwd.split_arg(1, dev)  # the plan only: this pass leaves no chunk record
            _launch("pna_bwd_edge", "rgbx_pna_bwd_edge_f32", graph.fwd.rowptr, graph.fwd.col, bm, cm, t,
                    _block_ptr(g_c, c0, c1), N, w, split, variant=variant)
        if want_b:
            bwd = graph.bwd
            split, _scratch2 = bwd.split_arg(w, dev)
            _launch("pna_bwd_src", "rgbx_pna_bwd_src_f32", bwd.rowptr, bwd.col, graph.t2f, bm, cm, t,
                    _block_ptr(g_b, c0, c1), bwd.N, w, split, variant=variant)
    return g_b, g_c


class _PNAAggregate(torch.autograd.Function):
    """One PNA aggregation as a single autograd node: forward = rgbx_pna_fwd_f32 (statistics of u_p = b_j + c_p, the
    shift by a, S * A scaled blocks stored once each); backward = the cotangent folded over the scalers and into the
    per-target rows (A, B, G_max, G_min) with dense per-node work on torch, then the source pass (g_b) and the edge pass
    (g_c), each run only where a gradient is asked for; g_a needs no kernel. Saved: b, c, the raw mean and std of u and
    the winning slots (only when a gradient will be asked for)."""

    @staticmethod
    def forward(ctx, a, b, c_slot, avg_deg, graph, names, scalers, F, want):
        a, b, c = (None if t is None else _rows_on_grid(t) for t in (a, b, c_slot))
        second = want and ("std" in names or "var" in names)
        keep = []
        if second:
            keep.append("mean")
        if want:
            keep += [k for k, n in (("std", "std"), ("argmax", "max"), ("argmin", "min")) if n in names]
        out, kept = pna_fwd_raw(graph.fwd, a, b, c, avg_deg, names, scalers, F, keep)
        ctx.graph, ctx.names, ctx.scalers, ctx.F = graph, names, scalers, F
        ctx.has = (a is not None, c_slot is not None)
        if want:
            # built here, outside the backward (their construction reads sizes back to the host)
            graph.bwd, graph.t2f
            ctx.save_for_backward(b if second else None, c if second else None, avg_deg.detach().reshape(-1),
                                  kept.get("mean"), kept.get("std"), kept.get("argmax"), kept.get("argmin"))
        return out

    @staticmethod
    def backward(ctx, gout):
        b, c, avg, mean_u, std, amax, amin = ctx.saved_tensors
        g, names, scalers, F = ctx.graph, ctx.names, ctx.scalers, ctx.F
        need = ctx.needs_input_grad
        N, dev = g.fwd.N, gout.device
        S, A = len(scalers), len(names)
        T = gout.size(1) // (S * A * F)
        d = T * F
        rowptr = g.fwd.rowptr
        deg = (rowptr[1:] - rowptr[:-1]).to(torch.float32)[:, None]
        inv_n = 1.0 / deg.clamp(min=1)
        # G_k = sum_s scale_s g_out[(s, k)], [N, T, A, F]
        G = (gout.reshape(N, T, S, A, F) * pna_scales(g, scalers, avg).view(N, 1, S, 1, 1)).sum(2)
        Gk = lambda n: G[:, :, names.index(n), :].reshape(N, d) if n in names else None
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        B = A_row = None
        if "std" in names:  # d std / d u_p = (u_p - mean) / (n std); 0 where the clamp or the mask is active
            B = torch.where(std > 0, Gk("std") * inv_n / std, zero)
        if "var" in names:  # d var / d u_p = 2 (u_p - mean) / n
            t = Gk("var") * (2.0 * inv_n)
            B = t if B is None else B + t
        b_k = b
        if B is not None:
            # a row of one slot has u_p = mean_u exactly: var and std are constant there and B contributes nothing. Left in,
            # B u_p - B mean_u cancels at the size of B, which is largest exactly there (2 / n, times lin / 1 under
            # inverse_linear): 5e-4 off a gradient that is 0
            B = torch.where(deg > 1, B, zero)
            # B (u_p - mean_u) as B u_p - B mean_u cancels on messages with an offset: both halves are taken relative to
            # the column mean s of mean_u (the same number), so the kernels' b is b - s
            s = mean_u.mean(0, keepdim=True)
            A_row = -B * (mean_u - s)
            b_k = b - s
        if "sum" in names:
            A_row = Gk("sum") if A_row is None else A_row + Gk("sum")
        if "mean" in names:
            t = Gk("mean") * inv_n
            A_row = t if A_row is None else A_row + t
        terms = {"A": A_row, "B": B, "gmax": Gk("max"), "argmax": amax, "gmin": Gk("min"), "argmin": amin}
        terms = {k: _rows_on_grid(v) for k, v in terms.items() if v is not None}
        has_a, has_c = ctx.has
        g_a = None
        if has_a and need[0]:  # the second-moment terms sum to zero over a row
            g_a = torch.zeros((N, d), dtype=torch.float32, device=dev)
            if "sum" in names:
                g_a = g_a + deg * Gk("sum")
            for n in ("mean", "max", "min"):
                if n in names:
                    g_a = g_a + Gk(n)
            g_a = torch.where(deg > 0, g_a, zero)
        g_b, g_c = pna_bwd_raw(g, terms, b_k, c, F, want_b=need[1], want_c=has_c and need[2])
        return g_a, g_b, g_c, None, None, None, None, None, None


def pna_supported(d, F):
    return bool(_lib.load().rgbx_pna_supported(d, F))


def pna_aggregate(a, b, c_slot, graph, aggregators, scalers, avg_deg, F):
    """PNAConv's message, aggregation and degree scaling in one pass: with u_p = b_j + c_p for the edge j -> i in forward
    CSR slot p, out[i, t*S*A*F + (s*A + k)*F + f] = scale_s(i) * stat_k(i)[t*F + f] — PyG's DegreeScalerAggregation
    layout (tower, then scaler, then aggregator), float32 [N, T*S*A*F].
      a [N, d] or None: the target part of the message; mean, max, min are shifted by a_i and the sum by n_i a_i
      b [N, d]: the source part;  c_slot [nnz, d] or None: the edge part, one row per forward CSR slot (edge_rows_to_slots)
      aggregators: distinct names out of sum / add, mean, var, std, max, min, in output order
      scalers: distinct names out of identity, amplification, attenuation, linear, inverse_linear, in output order
      avg_deg: float32 [2] on the device, [avg_lin, avg_log] (degree_averages(graph) for the graph's own)
      F: the tower width; F % 4 == 0 and F divides d = T * F
    The graph is in mode LOOPS_KEEP (edges as given; a node without in-edges gets zeros in every block). Column blocks of
    wider matrices are read in place; d above 256 runs as column blocks cut at tower boundaries (F <= 256). Gradients
    flow to a, b and c_slot, each pass run only where one is asked for; avg_deg takes none."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("PNAConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(a, b, c_slot, avg_deg)
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError(f"pna_aggregate: the graph must be in mode LOOPS_KEEP (got loops_mode="
                           f"{getattr(graph, 'loops_mode', None)!r})")
    names, scalers = multi_names(aggregators), pna_scaler_names(scalers)
    N, nnz = graph.fwd.N, graph.fwd.nnz
    if b.dim() != 2 or b.size(0) != N or b.dtype != torch.float32:
        raise RuntimeError(f"pna_aggregate: b {b.dtype} {tuple(b.shape)} for a graph of {N} nodes (float32 [N, d])")
    d = b.size(1)
    if a is not None and (tuple(a.shape) != (N, d) or a.dtype != torch.float32):
        raise RuntimeError(f"pna_aggregate: a {a.dtype} {tuple(a.shape)} for a graph of {N} nodes and b [N, {d}]")
    if c_slot is not None and (tuple(c_slot.shape) != (nnz, d) or c_slot.dtype != torch.float32):
        raise RuntimeError(f"pna_aggregate: c_slot {c_slot.dtype} {tuple(c_slot.shape)} for a graph of {nnz} slots and "
                           f"b [N, {d}] (float32 [nnz, d])")
    if avg_deg.numel() != 2 or avg_deg.dtype != torch.float32:
        raise RuntimeError(f"pna_aggregate: avg_deg {avg_deg.dtype} {tuple(avg_deg.shape)} (two float32: [lin, log])")
    F = int(F)
    if F < 4 or F % 4 or d % F or F > PNA_BLOCK:
        raise RuntimeError(f"pna_aggregate: tower width F = {F} for d = {d}: the kernels take F % 4 == 0 up to "
                           f"{PNA_BLOCK} with F dividing d; pad the tower width (PNAConv does)")
    want = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (a, b, c_slot))
    return _PNAAggregate.apply(a, b, c_slot, avg_deg, graph, names, scalers, F, want)


_TYPED_VIEWS_MAX = 4  # cached typed views per graph (each holds a handful of [E] vectors)


class TypedView:
    """What a relation per edge adds to a LOOPS_KEEP graph (typed_view builds it): `etype_f` / `etype_t` int32, the
    relation of every forward / transposed CSR slot; `w_f` / `w_t` float32, the slot weights of the mean per (target,
    relation), w_f[p] = 1 / #{p' in the row of p with p's relation} (rgbx_rgcn_slot_norm_f32) and w_t = w_f[t2f];
    `ones` for aggr="add"; `rel`, the forward slots grouped by relation as a CSR of R rows (rel_ptr [R + 1], rel_slots
    [E], a stable grouping: slot order inside a relation), which the reduction of g_comp walks. `select` holds the index
    sets of the select form and `expand_fwd` the relation-expanded forward CSR (FiLMConv's film pass); each is built on
    first use."""

    def __init__(self, graph, R, etype_f, etype_t, w_f, w_t, rel, etype_edge):
        self.graph, self.R = graph, R
        self.etype_f, self.etype_t, self.w_f, self.w_t, self.rel = etype_f, etype_t, w_f, w_t, rel
        self.ones = torch.ones_like(w_f)
        self._etype_edge = etype_edge  # int64 [E], per input edge
        self._select = None
        self._expand_fwd = None

    def weights(self, aggr, transposed=False):
        if aggr != "mean":
            return self.ones
        return self.w_t if transposed else self.w_f

    @property
    def select(self):
        """(fwd, bwd, w_bwd) of the select form. fwd: the forward CSR with col'[p] = col[p] * R + type(p), which reads
        row (j, r) of h viewed as [N * R, C]. bwd: the relation-expanded transposed CSR of N * R rows, row j * R + r
        holding the out-edges of j with relation r (rgbx_csr_build on the keys j * R + r, with its own hub plan); w_bwd:
        the mean weights in its slot order. Built on first use, once per view (a CSR build: its read-backs of the slot count
        and the longest row happen here, not in a step)."""
        if self._select is None:
            from .graph import CSR, LOOPS_KEEP, build_csr
            g, R = self.graph, self.R
            E = g.fwd.nnz
            col = (g.fwd.col[:max(E, 1)].long() * R + self.etype_f.long()).to(torch.int32).contiguous()
            fwd = CSR(g.fwd.rowptr, col, None, g.fwd.N, E, g.fwd.split)
            bwd = build_csr(g._src * R + self._etype_edge, g._dst, g.N * R, LOOPS_KEEP)
            if E:
                w_bwd = self.w_f[_slot_to_edge(g)[1][bwd.perm[:E].long()].long()].contiguous()
            else:
                w_bwd = self.w_f
            self._select = (fwd, bwd, w_bwd)
        return self._select

    @property
    def expand_fwd(self):
        """The relation-expanded FORWARD CSR of N * R rows: row i * R + r holds the in-edges of i with relation r, its
        columns are their sources (rgbx_csr_build on the keys i * R + r, with its own hub plan). A row's length is the
        count behind the mean weight of its slots, so the film pass of FiLMConv takes ONE weight per row, 1 / len. With one
        relation it is the graph's forward CSR itself. N * R >= 2^31 is refused. Built on first use, once per view."""
        if self._expand_fwd is None:
            from .graph import LOOPS_KEEP, build_csr
            g, R = self.graph, self.R
            if g.N * R >= 2 ** 31:
                raise RuntimeError(f"typed_view: the relation-expanded index sets hold N * R = {g.N} * {R} rows, beyond "
                                   "int32")
            self._expand_fwd = g.fwd if R == 1 else build_csr(g._dst * R + self._etype_edge, g._src, g.N * R,
                                                              LOOPS_KEEP)
        return self._expand_fwd


def typed_view(graph, edge_type, num_relations):
    """The TypedView of `graph` under `edge_type` (int64 [E], one relation in [0, num_relations) per INPUT edge), cached on
    the graph per (storage, shape, in-place version, R), at most 4 entries. Only for graphs in mode LOOPS_KEEP, where every
    input edge owns exactly one slot; other modes and the partitioned graph raise, as edge_rows_to_slots does. A relation
    outside the range is refused here, once: the one device synchronisation of the typed path, paid per cache entry (the
    same read-back brings the slot count of every relation, from which the hub plan of `rel` is laid out on the host)."""
    from .graph import CSR, LOOPS_KEEP, make_row_split
    if _is_dist(graph):
        raise RuntimeError("edge types have no node-partitioned form: run it on one GPU")
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("typed_view: only a graph in mode LOOPS_KEEP maps every input edge to exactly one CSR slot "
                           f"(got loops_mode={getattr(graph, 'loops_mode', None)!r})")
    R = int(num_relations)
    if R <= 0:
        raise ValueError(f"typed_view: num_relations must be positive, got {num_relations}")
    if not torch.is_tensor(edge_type) or edge_type.dtype != torch.int64 or edge_type.dim() != 1 \
            or edge_type.numel() != graph.E:
        got = f"{edge_type.dtype} {tuple(edge_type.shape)}" if torch.is_tensor(edge_type) else type(edge_type).__name__
        raise ValueError(f"typed_view: edge_type must be int64 [E] = [{graph.E}], got {got}")
    _lib.require_device(edge_type)
    if graph.fwd.nnz != graph.E:
        raise RuntimeError(f"typed_view: {graph.fwd.nnz} CSR slots for {graph.E} input edges")
    cache = graph.__dict__.setdefault("_typed_views", {})
    key = (edge_type.data_ptr(), tuple(edge_type.shape), edge_type._version, R)
    hit = cache.get(key)
    if hit is not None:
        return hit[1]
    dev, E = graph.fwd.rowptr.device, graph.E
    if E:
        et = edge_type.detach().contiguous()
        counts = torch.bincount(et.clamp(0, R - 1), minlength=R)
        host = torch.cat([et.min().reshape(1), et.max().reshape(1), counts]).cpu()  # the one synchronisation
        lo, hi = int(host[0]), int(host[1])
        if lo < 0 or hi >= R:
            raise ValueError(f"edge_type values [{lo}, {hi}] outside [0, num_relations) = [0, {R})")
        t2f = graph.t2f.long()
        etype_f = et[_slot_to_edge(graph)[0].long()].to(torch.int32).contiguous()
        etype_t = etype_f[t2f].contiguous()
        w_f = torch.empty(E, dtype=torch.float32, device=dev)
        split, _scratch = graph.fwd.split_arg(1, dev)  # the plan only: the count leaves no chunk record
        _launch("rgcn_slot_norm", "rgbx_rgcn_slot_norm_f32", graph.fwd.rowptr, etype_f, w_f, graph.fwd.N, R, split)
        w_t = w_f[t2f].contiguous()
        rel_ptr = torch.zeros(R + 1, dtype=torch.int64)
        rel_ptr[1:] = torch.cumsum(host[2:], 0)
        plan = make_row_split(rel_ptr)  # on the host: no further read-back
        if plan is not None:
            plan = {k: v.to(dev) if torch.is_tensor(v) else v for k, v in plan.items()}
        rel_slots = torch.sort(etype_f, stable=True)[1].to(torch.int32).contiguous()
        rel = CSR(rel_ptr.to(torch.int32).to(dev), rel_slots, None, R, E, plan)
    else:  # no slot is ever read: one-element placeholders the entry points accept
        et = edge_type.detach()
        etype_f = etype_t = torch.zeros(1, dtype=torch.int32, device=dev)
        w_f = w_t = torch.ones(1, dtype=torch.float32, device=dev)
        rel = CSR(torch.zeros(R + 1, dtype=torch.int32, device=dev), etype_f, None, R, 0, None)
    view = TypedView(graph, R, etype_f, etype_t, w_f, w_t, rel, et)
    cache[key] = (edge_type, view)  # the key holds the tensor's data_ptr: keep its storage alive beside the view
    while len(cache) > _TYPED_VIEWS_MAX:
        cache.pop(next(iter(cache)))
    return view


class _RGCNSelect(torch.autograd.Function):
    """RGCNConv's aggregation without a basis: h = x @ [W_0 | ... | W_{R-1}] viewed as [N * R, C], and the existing
    weighted SpMM with col' = col * R + type; backward = the same SpMM over the relation-expanded transposed CSR."""

    @staticmethod
    def forward(ctx, h, y0, view, aggr):
        N, R = view.graph.fwd.N, view.R
        C = h.size(1) // R
        fwd = view.select[0]
        hv = h.contiguous().view(N * R, C)
        w = view.w_f if aggr == "mean" else None
        ctx.view, ctx.aggr, ctx.C = view, aggr, C
        if y0 is None:
            return spmm_raw(fwd, w, None, hv, kind="rgcn_select_fwd")
        return spmm_raw(fwd, w, None, hv, y=y0.contiguous(), a=1.0, b=1.0, kind="rgcn_select_fwd")

    @staticmethod
    def backward(ctx, gout):
        view, need = ctx.view, ctx.needs_input_grad
        g_h = None
        if need[0]:
            _, bwd, w_bwd = view.select
            g_h = spmm_raw(bwd, w_bwd if ctx.aggr == "mean" else None, None, gout.contiguous(), kind="rgcn_select_bwd")
            g_h = g_h.view(view.graph.fwd.N, view.R * ctx.C)
        return g_h, (gout if need[1] else None), None, None


class _RGCNMix(torch.autograd.Function):
    """RGCNConv's aggregation under a basis decomposition as one autograd node: out = y0 + sum_p sum_b w[p]
    comp[type(p), b] h[col[p], b, :] in rgbx_rgcn_mix_fwd_f32; backward = the source pass over the transposed CSR (g_h,
    only when h asks), the coefficient pass over the forward CSR plus the fixed-order reduction by relation (g_comp, only
    when comp asks), g_y0 = gout. Saves h and comp and nothing per edge; the kernels read comp on the device."""

    @staticmethod
    def forward(ctx, h, comp, y0, view, aggr):
        _lib.require_device(h, comp, y0)
        R, B = comp.shape
        C = h.size(1) // B
        g = view.graph
        csr, N, dev = g.fwd, g.fwd.N, h.device
        vec = _head_vec(C)
        h = _rows_on_grid(h, vec)
        compv = comp.detach().contiguous()  # a contiguous parameter's own storage: a captured launch follows it
        y = None if y0 is None else _rows_on_grid(y0, vec)
        out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written
        split, _scratch = csr.split_arg(C, dev)
        _launch("rgcn_mix_fwd", "rgbx_rgcn_mix_fwd_f32", csr.rowptr, csr.col, view.etype_f, view.weights(aggr), compv,
                _lib.mat(h, "h"), _lib.mat_opt(y, "y0"), _lib.mat(out, "out"), N, R, B, C, split)
        ctx.view, ctx.aggr, ctx.dims = view, aggr, (R, B, C)
        ctx.save_for_backward(h, compv)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, compv = ctx.saved_tensors
        view, aggr, (R, B, C) = ctx.view, ctx.aggr, ctx.dims
        g = view.graph
        N, dev = g.fwd.N, h.device
        need = ctx.needs_input_grad
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        gm = _lib.mat(gout, "gout")
        g_h = g_comp = None
        if need[0]:
            g_h = torch.empty((N, B * C), dtype=torch.float32, device=dev)  # every row is written (no out-edge: zeros)
            split, _scratch = g.bwd.split_arg(B * C, dev)
            _launch("rgcn_mix_bwd_src", "rgbx_rgcn_mix_bwd_src_f32", g.bwd.rowptr, g.bwd.col, view.etype_t,
                    view.weights(aggr, True), compv, gm, _lib.mat(g_h, "g_h"), N, R, B, C, split)
        if need[1]:
            nnz = g.fwd.nnz
            if nnz:
                d = torch.empty((nnz, B), dtype=torch.float32, device=dev)  # every (slot, head) is written
                split, _scratch2 = g.fwd.split_arg(1, dev)  # the plan only: this pass leaves no chunk record
                _launch("rgcn_mix_bwd_coef", "rgbx_rgcn_mix_bwd_coef_f32", g.fwd.rowptr, g.fwd.col, view.weights(aggr),
                        _lib.mat(h, "h"), gm, d, N, R, B, C, split)
                g_comp = spmm_raw(view.rel, None, None, d, kind="rgcn_comp_reduce")  # a relation without slots: zeros
            else:
                g_comp = torch.zeros((R, B), dtype=torch.float32, device=dev)
        return g_h, g_comp, (gout if need[2] else None), None, None


def rgcn_mix_supported(B, C):
    return bool(_lib.load().rgbx_rgcn_mix_supported(B, C))


_EDGE_AGGRS = {"mean": "mean", "add": "add", "sum": "add"}  # what rgcn / film / gmm_aggregate take as `aggr`


def rgcn_aggregate(h, graph, edge_type, num_relations, comp=None, aggr="mean", y0=None):
    """RGCNConv's aggregation over a LOOPS_KEEP graph whose input edge e has relation edge_type[e] (int64 [E], values in
    [0, num_relations)); the edges as given: duplicates count twice, self-loops are ordinary edges, a (target, relation)
    pair without an edge contributes 0. `aggr` "mean" is the mean per (target, relation), "add" / "sum" the sum. `y0`
    [N, C] (optional) is added to every row: the layer's dense root + bias term, so that the output is written once.

    Select form (comp=None): h [N, R * C] = x @ [W_0 | ... | W_{R-1}]; out_i = y0_i + sum_p w[p] h[col[p], type(p), :]
    through the weighted SpMM with col' = col * R + type, its gradient through the same SpMM over the relation-expanded
    transposed CSR. IT MATERIALISES N * R * C FLOATS (h, and as many again for its gradient); a basis decomposition is the
    answer for large R. N * R >= 2^31 is refused before any launch.

    Mix form (comp [R, B], float32, on the device; it may take a gradient): h [N, B * C] = x @ [V_0 | ... | V_{B-1}];
    out_i = y0_i + sum_p sum_b w[p] comp[type(p), b] h[col[p], b, :] in the rgbx_rgcn_mix_* kernels, which read comp from
    device memory. Gradients for h, comp and y0, each pass only when asked for; nothing per edge is saved. No float
    atomics in either form: two runs are bit-identical. Timing names: rgcn_select_fwd / rgcn_select_bwd; rgcn_mix_fwd,
    rgcn_mix_bwd_src, rgcn_mix_bwd_coef, rgcn_comp_reduce."""
    if _is_dist(graph):
        raise RuntimeError("RGCNConv has no node-partitioned form: run it on one GPU")
    if aggr not in _EDGE_AGGRS:
        raise ValueError(f"rgcn_aggregate: aggr={aggr!r} (mean, add or sum)")
    aggr = _EDGE_AGGRS[aggr]
    R = int(num_relations)
    N = graph.fwd.N
    heads = R if comp is None else (comp.size(1) if comp.dim() == 2 else -1)
    if comp is not None and (comp.dim() != 2 or comp.size(0) != R or comp.dtype != torch.float32):
        raise RuntimeError(f"rgcn_aggregate: comp {comp.dtype} {tuple(comp.shape)} (float32 [num_relations, num_bases] = "
                           f"[{R}, B])")
    if h.dim() != 2 or h.size(0) != N or heads <= 0 or h.size(1) % heads or h.size(1) == 0 or h.dtype != torch.float32:
        raise RuntimeError(f"rgcn_aggregate: h {h.dtype} {tuple(h.shape)} for a graph of {N} nodes and {heads} "
                           f"{'relations' if comp is None else 'bases'} (float32 [N, {heads} * C])")
    C = h.size(1) // heads
    if y0 is not None and (tuple(y0.shape) != (N, C) or y0.dtype != torch.float32):
        raise RuntimeError(f"rgcn_aggregate: y0 {y0.dtype} {tuple(y0.shape)} (float32 [N, C] = [{N}, {C}])")
    if comp is None and N * R >= 2 ** 31:
        raise RuntimeError(f"rgcn_aggregate: the select form indexes N * R = {N} * {R} rows, beyond int32; use a basis "
                           "decomposition (num_bases)")
    _lib.require_device(h, comp, y0)
    if comp is not None and not rgcn_mix_supported(heads, C):
        raise RuntimeError(f"rgcn_aggregate: {heads} bases of {C} channels: the kernels take 1 <= B <= 64 and any "
                           "C <= 64, even C <= 128 or C % 4 == 0 up to 256; pad the width (RGCNConv does)")
    view = typed_view(graph, edge_type, R)
    if comp is None:
        return _RGCNSelect.apply(h, y0, view, aggr)
    return _RGCNMix.apply(h, comp, y0, view, aggr)


# ---- FiLMConv: the target modulates every message per channel, before the nonlinearity ---------------------------------

_FILM_ACTS = {"relu": 1, "identity": 0, None: 0}  # the kernels' `act`
FILM_BLOCK = 256  # wider inputs run as column blocks of this many channels


def film_supported(C):
    return bool(_lib.load().rgbx_film_supported(C))


def film_fwd_raw(hv, fv, gofs, graph, view, mean, act, y0=None):
    """rgbx_film_fwd_f32 (no autograd): hv [N * R, C] and fv [N * R, gofs + C] (beta at column 0, gamma at column gofs)
    -> out [N, C]. `view`: the TypedView, or None for the single-relation call; `mean` / `act`: the kernels' ints."""
    _lib.require_device(hv, fv, y0)
    csr, N, C, dev = graph.fwd, graph.fwd.N, hv.size(1), hv.device
    R = 1 if view is None else view.R
    # the relation and the weight of every slot; one relation: none of either, the kernel divides by the row length
    etype, w = (None, None) if view is None else (view.etype_f, view.w_f if mean else view.ones)
    out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (rows without slots: y0 / zeros)
    split, _scratch = csr.split_arg(C, dev)
    _launch("film_fwd", "rgbx_film_fwd_f32", csr.rowptr, csr.col, etype, w, _lib.mat(hv, "h"), _lib.mat(fv, "fb"), gofs,
            _lib.mat_opt(y0, "y0"), _lib.mat(out, "out"), N, R, C, int(mean), int(act), split)
    return out


def film_bwd_raw(hv, fv, gofs, gout, graph, view, mean, act, want_h=True, want_fb=True):
    """rgbx_film_bwd_src_f32 and rgbx_film_bwd_film_f32 (no autograd), each launched only when asked for: (g_h [N * R, C]
    or None, g_fb in fv's shape and layout or None)."""
    _lib.require_device(hv, fv, gout)
    N, C, dev = graph.fwd.N, hv.size(1), hv.device
    R = 1 if view is None else view.R
    hm, fm, gm = _lib.mat(hv, "h"), _lib.mat(fv, "fb"), _lib.mat(gout, "gout")
    g_h = g_fb = None
    if want_h:
        if view is None:  # the plain transposed CSR; the mean weight of a slot from its target's row length
            csr, w_t, deg_rowptr = graph.bwd, None, (graph.fwd.rowptr if mean else None)
        else:             # the relation-expanded transposed CSR the RGCN select form builds: shared, not built twice
            _, csr, w_bwd = view.select
            w_t, deg_rowptr = (w_bwd if mean else None), None
        g_h = torch.empty((N * R, C), dtype=torch.float32, device=dev)  # every row is written (no out-edge: zeros)
        split, _scratch = csr.split_arg(C, dev)
        _launch("film_bwd_src", "rgbx_film_bwd_src_f32", csr.rowptr, csr.col, w_t, deg_rowptr, hm, fm, gofs, gm,
                _lib.mat(g_h, "g_h"), N, R, C, int(act), split)
    if want_fb:
        csr = graph.fwd if view is None else view.expand_fwd
        # the kernel writes the two blocks of every row; columns between them (a column block of a wider fb) stay zero
        alloc = torch.empty if gofs == C else torch.zeros
        g_fb = alloc((N * R, gofs + C), dtype=torch.float32, device=dev)
        split, _scratch2 = csr.split_arg(2 * C, dev)
        _launch("film_bwd_film", "rgbx_film_bwd_film_f32", csr.rowptr, csr.col, hm, fm, gofs, gm, _lib.mat(g_fb, "g_fb"),
                N, R, C, int(mean), int(act), split)
    return g_h, g_fb


class _FiLMAggregate(torch.autograd.Function):
    """FiLMConv's aggregation as one autograd node: out = y0 + sum_p w[p] act(gamma[i, r] h[j, r] + beta[i, r]) in
    rgbx_film_fwd_f32; backward = the source pass over the (relation-expanded) transposed CSR (g_h, only when h asks),
    the film pass over the (relation-expanded) forward CSR (g_fb, only when fb asks), g_y0 = gout. Saves h and fb and
    nothing per edge: both passes recompute the mask from the forward's own fmaf."""

    @staticmethod
    def forward(ctx, hv, fv, y0, graph, view, mean, act, gofs):
        _lib.require_device(hv, fv, y0)
        vec = _head_vec(hv.size(1))
        # column blocks of wider matrices stay views, where the row still fits a wave at the vector width they allow
        hv, fv = _rows_on_grid(hv, vec), _rows_on_grid(fv, vec)
        y = None if y0 is None else _rows_on_grid(y0, vec)
        out = film_fwd_raw(hv, fv, gofs, graph, view, mean, act, y)
        ctx.args = (graph, view, mean, act, gofs)
        ctx.save_for_backward(hv, fv)
        return out

    @staticmethod
    def backward(ctx, gout):
        hv, fv = ctx.saved_tensors
        graph, view, mean, act, gofs = ctx.args
        need = ctx.needs_input_grad
        g_h = g_fb = None
        if need[0] or need[1]:
            g = _rows_on_grid(gout.contiguous(), _head_vec(hv.size(1)))
            g_h, g_fb = film_bwd_raw(hv, fv, gofs, g, graph, view, mean, act, want_h=need[0], want_fb=need[1])
        return g_h, g_fb, (gout if need[2] else None), None, None, None, None, None


def film_aggregate(h, fb, graph, edge_type=None, num_relations=1, aggr="mean", act="relu", y0=None):
    """FiLMConv's aggregation over a LOOPS_KEEP graph (the edges as given: duplicates count twice, self-loops are ordinary
    edges), with R = num_relations and C channels:
      h  [N, R * C]  = x @ [W_0 | ... | W_{R-1}]           (column block r: the message rows under relation r)
      fb [N, R * 2C] = [film_0(x) | ... | film_{R-1}(x)]   (column block r: beta_r | gamma_r, beta FIRST)
      out_i = y0_i + sum_r AGG_{j : (j -> i) of relation r} act(gamma_r[i] * h_r[j] + beta_r[i])
    `edge_type` int64 [E] with values in [0, R), one relation per INPUT edge; None is the single-relation call (R must
    be 1: no typed view is built, the mean weights come from the row lengths). `aggr` "mean" is the mean per (target,
    relation), "add" / "sum" the sum; a (target, relation) pair without an edge contributes 0. `act`: "relu", or
    "identity" / None. `y0` [N, C] (optional) is the dense skip term, added in the kernel so that the output is written
    once. IT MATERIALISES N * R * 3C FLOATS (h and fb), and as many again for their gradients; N * R >= 2^31 is refused
    before any launch. One autograd node: g_h through the source pass, g_fb through the film pass, g_y0 = gout, each only
    when asked for; h and fb are saved and nothing per edge. The op is per channel: a width above 256 runs as column
    blocks of 256, which is exact. No float atomics: two runs are bit-identical. Timing names: film_fwd, film_bwd_src,
    film_bwd_film."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("FiLMConv has no node-partitioned form: run it on one GPU")
    if aggr not in _EDGE_AGGRS:
        raise ValueError(f"film_aggregate: aggr={aggr!r} (mean, add or sum)")
    if not (act is None or isinstance(act, str)) or act not in _FILM_ACTS:
        raise ValueError(f"film_aggregate: act={act!r} (relu, identity or None)")
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("film_aggregate: only a graph in mode LOOPS_KEEP takes the edges as given "
                           f"(got loops_mode={getattr(graph, 'loops_mode', None)!r})")
    mean, act = int(_EDGE_AGGRS[aggr] == "mean"), _FILM_ACTS[act]
    R = int(num_relations)
    if R <= 0:
        raise ValueError(f"film_aggregate: num_relations must be positive, got {num_relations}")
    if edge_type is None and R != 1:
        raise ValueError(f"film_aggregate: edge_type must be int64 [E] for num_relations={R}, got None")
    N = graph.fwd.N
    if h.dim() != 2 or h.size(0) != N or h.size(1) % R or h.size(1) == 0 or h.dtype != torch.float32:
        raise RuntimeError(f"film_aggregate: h {h.dtype} {tuple(h.shape)} for a graph of {N} nodes and {R} relations "
                           f"(float32 [N, {R} * C])")
    C = h.size(1) // R
    if tuple(fb.shape) != (N, 2 * R * C) or fb.dtype != torch.float32:
        raise RuntimeError(f"film_aggregate: fb {fb.dtype} {tuple(fb.shape)} (float32 [N, R * 2C] = [{N}, {2 * R * C}])")
    if y0 is not None and (tuple(y0.shape) != (N, C) or y0.dtype != torch.float32):
        raise RuntimeError(f"film_aggregate: y0 {y0.dtype} {tuple(y0.shape)} (float32 [N, C] = [{N}, {C}])")
    if N * R >= 2 ** 31:
        raise RuntimeError(f"film_aggregate: the operands hold N * R = {N} * {R} rows, beyond int32")
    _lib.require_device(h, fb, y0)
    blocked = C > FILM_BLOCK and film_supported(C % FILM_BLOCK or FILM_BLOCK)
    if not blocked and not film_supported(C):
        raise RuntimeError(f"film_aggregate: h {tuple(h.shape)} with {R} relations: the kernels take any C <= 64, even "
                           "C <= 128 or C % 4 == 0 up to 256 (and blocks of 256 above); pad the width (FiLMConv does)")
    view = None if edge_type is None else typed_view(graph, edge_type, R)
    # one relation: column blocks of wider matrices are taken as they are; several: the [N * R, .] views need whole rows
    hv = h if R == 1 else h.contiguous().view(N * R, C)
    fv = fb if R == 1 else fb.contiguous().view(N * R, 2 * C)
    if not blocked:
        return _FiLMAggregate.apply(hv, fv, y0, graph, view, mean, act, C)
    outs = []
    for a in range(0, C, FILM_BLOCK):
        b = min(a + FILM_BLOCK, C)
        if C % 4 == 0:   # beta's block to gamma's block as ONE view: gamma sits the full width behind beta
            fblk, gofs = fv[:, a:C + b], C
        else:            # the vector width of a 256-wide block needs gamma on its grid: the two blocks side by side
            fblk, gofs = torch.cat([fv[:, a:b], fv[:, C + a:C + b]], dim=1), b - a
        outs.append(_FiLMAggregate.apply(hv[:, a:b], fblk, None if y0 is None else y0[:, a:b], graph, view, mean, act,
                                         gofs))
    return torch.cat(outs, dim=1)


class _GMMAggregate(torch.autograd.Function):
    """GMMConv's aggregation as one autograd node: out = y0 + rs * sum_p sum_k gauss[p, k] h[col[p], k, :] in
    rgbx_gmm_fwd_f32, gauss evaluated in registers from mu and sigma on the device; backward = the source pass over the
    transposed CSR (g_h, only when h asks) and the edge pass over the forward CSR (g_e when e_slot asks, g_mu and g_sigma
    when either parameter asks), g_y0 = gout. Saves h, e_slot, mu and sigma and nothing per edge beyond them."""

    @staticmethod
    def forward(ctx, h, e_slot, mu, sigma, y0, graph, aggr):
        _lib.require_device(h, e_slot, mu, sigma, y0)
        K, D = mu.shape
        M = h.size(1) // K
        csr, N, dev = graph.fwd, graph.fwd.N, h.device
        vec = _head_vec(M)
        h = _rows_on_grid(h, vec)
        e = _rows_on_grid(e_slot, 1)
        if csr.nnz == 0:  # no slot row is ever read: a pointer the entry points accept
            e = torch.empty((1, D), dtype=torch.float32, device=dev)
        # a contiguous parameter's own storage: a captured launch follows it
        muv, sigv = mu.detach().contiguous(), sigma.detach().contiguous()
        y = None if y0 is None else _rows_on_grid(y0, vec)
        rs = graph.inv_deg if aggr == "mean" else None
        out = torch.empty((N, M), dtype=torch.float32, device=dev)  # every row is written
        split, _scratch = csr.split_arg(M, dev)
        _launch("gmm_fwd", "rgbx_gmm_fwd_f32", csr.rowptr, csr.col, _lib.mat(e, "e_slot"), muv, sigv, rs, _lib.mat(h, "h"),
                _lib.mat_opt(y, "y0"), _lib.mat(out, "out"), N, K, M, D, split)
        ctx.graph, ctx.aggr, ctx.dims = graph, aggr, (K, M, D)
        ctx.save_for_backward(h, e, muv, sigv)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, e, muv, sigv = ctx.saved_tensors
        g, aggr, (K, M, D) = ctx.graph, ctx.aggr, ctx.dims
        N, nnz, dev = g.fwd.N, g.fwd.nnz, h.device
        need = ctx.needs_input_grad
        gout = _rows_on_grid(gout.contiguous(), _head_vec(M))
        gm, em = _lib.mat(gout, "gout"), _lib.mat(e, "e_slot")
        g_h = g_e = g_mu = g_sigma = None
        if need[0]:
            g_h = torch.empty((N, K * M), dtype=torch.float32, device=dev)  # every row is written (no out-edge: zeros)
            w_t = g.w_mean_t if aggr == "mean" else None
            split, _scratch = g.bwd.split_arg(K * M, dev)
            _launch("gmm_bwd_src", "rgbx_gmm_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.t2f, w_t, em, muv, sigv, gm,
                    _lib.mat(g_h, "g_h"), N, K, M, D, split)
        want_e, want_p = need[1], need[2] or need[3]
        if want_e:
            g_e = torch.empty((nnz, D), dtype=torch.float32, device=dev)  # every slot row is written
        if want_p:
            g_mu, g_sigma = (torch.zeros((K, D), dtype=torch.float32, device=dev) if nnz == 0 else
                             torch.empty((K, D), dtype=torch.float32, device=dev) for _ in range(2))
        if nnz and (want_e or want_p):
            nbytes = ctypes.c_size_t(0)
            _lib.call("rgbx_gmm_bwd_edge_workspace_bytes", nnz, K, D, ctypes.byref(nbytes))
            ws = torch.empty(max(nbytes.value // 4, 1), dtype=torch.float32, device=dev)
            rs = g.inv_deg if aggr == "mean" else None
            split, _scratch2 = g.fwd.split_arg(1, dev)  # the plan only: this pass leaves no chunk record
            _launch("gmm_bwd_edge", "rgbx_gmm_bwd_edge_f32", g.fwd.rowptr, g.fwd.col, em, muv, sigv, rs, _lib.mat(h, "h"),
                    gm, _lib.mat(g_e, "g_e") if want_e else (0, 0), g_mu, g_sigma, ws, ws.numel() * 4, N, nnz, K, M, D,
                    split)
        return (g_h, g_e, g_mu if need[2] else None, g_sigma if need[3] else None, gout if need[4] else None, None,
                None)


def gmm_supported(K, M, D):
    return bool(_lib.load().rgbx_gmm_supported(K, M, D))


def gmm_aggregate(h, e_slot, mu, sigma, graph, aggr="mean", y0=None):
    """GMMConv's aggregation (MoNet; separate_gaussians=False) over a LOOPS_KEEP graph, the edges as given: self-loops
    stay, duplicates count twice. h [N, K * M] = x @ g, k-major columns (h.view(N, K, M)); e_slot [nnz, D] float32, the
    pseudo-coordinates of every forward CSR slot (edge_rows_to_slots gives the order); mu, sigma [K, D] float32 on the
    device:
        gauss[p, k] = exp(sum_d -0.5 (e[p, d] - mu[k, d])^2 / (1e-15 + sigma[k, d]^2))
        out_i       = y0_i + AGG_p sum_k gauss[p, k] h[col[p], k, :]
    AGG "mean" divides by the number of in-edges as given, "add" / "sum" does not; a node without in-edges gets y0 (or
    zeros). `y0` [N, M] (optional) is the layer's dense root + bias term, so that the output is written once. Column
    blocks of a wider matrix are taken as they are where their rows sit on the vector grid. Gradients for h, e_slot, mu,
    sigma and y0, each pass only where asked for; nothing per edge is saved and the kernels read mu and sigma from device
    memory. No float atomics: two runs are bit-identical. Timing names: gmm_fwd, gmm_bwd_src, gmm_bwd_edge."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("GMMConv has no node-partitioned form: run it on one GPU")
    if aggr not in _EDGE_AGGRS:
        raise ValueError(f"gmm_aggregate: aggr={aggr!r} (mean, add or sum)")
    aggr = _EDGE_AGGRS[aggr]
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("gmm_aggregate: only a graph in mode LOOPS_KEEP keeps one CSR slot per input edge (got "
                           f"loops_mode={getattr(graph, 'loops_mode', None)!r})")
    N, nnz = graph.fwd.N, graph.fwd.nnz
    if not all(torch.is_tensor(t) and t.dim() == 2 and t.dtype == torch.float32 for t in (mu, sigma)) \
            or mu.shape != sigma.shape or mu.size(0) == 0:
        raise RuntimeError("gmm_aggregate: mu and sigma must be float32 [K, D] of one shape")
    K, D = mu.shape
    if h.dim() != 2 or h.size(0) != N or h.size(1) == 0 or h.size(1) % K or h.dtype != torch.float32:
        raise RuntimeError(f"gmm_aggregate: h {h.dtype} {tuple(h.shape)} for a graph of {N} nodes and {K} kernels "
                           f"(float32 [N, {K} * M])")
    M = h.size(1) // K
    if e_slot.dim() != 2 or tuple(e_slot.shape) != (nnz, D) or e_slot.dtype != torch.float32:
        raise RuntimeError(f"gmm_aggregate: e_slot {e_slot.dtype} {tuple(e_slot.shape)} for a graph of {nnz} slots and "
                           f"{D} coordinates (float32 [nnz, D] = [{nnz}, {D}])")
    if y0 is not None and (tuple(y0.shape) != (N, M) or y0.dtype != torch.float32):
        raise RuntimeError(f"gmm_aggregate: y0 {y0.dtype} {tuple(y0.shape)} (float32 [N, M] = [{N}, {M}])")
    _lib.require_device(h, e_slot, mu, sigma, y0)
    if not gmm_supported(K, M, D):
        raise RuntimeError(f"gmm_aggregate: {K} kernels of {M} channels over {D} coordinates: the kernels take "
                           "1 <= K <= 64, 1 <= D <= 8 and any M <= 64, even M <= 128 or M % 4 == 0 up to 256; pad the "
                           "width (GMMConv does)")
    return _GMMAggregate.apply(h, e_slot, mu, sigma, y0, graph, aggr)


def degree_pseudo(graph):
    """The MoNet paper's pseudo-coordinates of a LOOPS_KEEP graph without edge attributes, [nnz, 2] float32 in forward
    CSR slot order: u[p] = (1 / sqrt(1 + indeg(source)), 1 / sqrt(1 + indeg(target))), the in-degrees as given
    (rgbx_gmm_degree_pseudo_f32). Built once per graph and kept on it; it takes no gradient."""
    from .graph import LOOPS_KEEP
    if _is_dist(graph):
        raise RuntimeError("degree pseudo-coordinates have no node-partitioned form: run it on one GPU")
    if getattr(graph, "loops_mode", None) != LOOPS_KEEP:
        raise RuntimeError("degree_pseudo: only a graph in mode LOOPS_KEEP keeps one CSR slot per input edge (got "
                           f"loops_mode={getattr(graph, 'loops_mode', None)!r})")
    cached = graph.__dict__.get("_degree_pseudo")
    if cached is None:
        csr = graph.fwd
        _lib.require_device(csr.rowptr)
        dev = csr.rowptr.device
        u = torch.empty((csr.nnz, 2), dtype=torch.float32, device=dev)  # every slot is written
        if csr.nnz:
            split, _scratch = csr.split_arg(1, dev)  # the plan only: no chunk record
            _launch("gmm_degree_pseudo", "rgbx_gmm_degree_pseudo_f32", csr.rowptr, csr.col, u, csr.N, split)
        cached = graph._degree_pseudo = u
    return cached


class _SoftmaxAggregate(torch.autograd.Function):
    """One softmax aggregation as a single autograd node: a softmax per channel over the in-edges at temperature t, fused
    with the sum of the weighted message rows; backward = one pass over the transposed CSR (g_m, and the g_t records
    plus their reduction only when t asks for a gradient). Saves m, t, out and lse [N, C]; nothing per edge (the
    backward recomputes alpha = exp(t m_j - lse_i)). The kernels read t from device memory, so a captured launch
    follows a temperature the optimizer moves."""

    @staticmethod
    def forward(ctx, m, t, graph, want_grad):
        _lib.require_device(m, t)
        C = m.size(1)
        m = _rows_on_grid(m, _head_vec(C))
        csr, N, dev = graph.fwd, graph.fwd.N, m.device
        tv = t.detach().reshape(-1).contiguous()
        out = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (rows without slots: zeros)
        # lse is the backward's; without one the kernel runs its inference form
        lse = torch.empty((N, C), dtype=torch.float32, device=dev) if want_grad else None
        split, _scratch = csr.split_arg(3 * C, dev)
        _launch("softmax_aggr_fwd", "rgbx_softmax_aggr_fwd_f32", csr.rowptr, csr.col, _lib.mat(m, "m"), tv, tv.numel() > 1,
                _lib.mat(out, "out"), _lib.mat_opt(lse, "lse"), N, C, split)
        ctx.graph, ctx.t_shape = graph, t.shape
        ctx.save_for_backward(m, tv, out, lse)
        return out

    @staticmethod
    def backward(ctx, gout):
        m, tv, out, lse = ctx.saved_tensors
        g = ctx.graph
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None, None, None
        N, C, dev = g.fwd.N, m.size(1), m.device
        gout = _rows_on_grid(gout.contiguous(), _head_vec(C))
        g_m = torch.empty((N, C), dtype=torch.float32, device=dev)  # every row is written (sources without slots: zeros)
        split, _scratch = g.bwd.split_arg(C, dev)
        g_t = part = None
        n_part = ctypes.c_int64(0)
        if need[1]:
            _lib.call("rgbx_softmax_aggr_gt_partial_floats", N, C, split, ctypes.byref(n_part))
            g_t = torch.empty(C, dtype=torch.float32, device=dev)
            part = torch.empty(max(n_part.value, 1), dtype=torch.float32, device=dev)
        _launch("softmax_aggr_bwd", "rgbx_softmax_aggr_bwd_f32", g.bwd.rowptr, g.bwd.col, _lib.mat(m, "m"), tv,
                tv.numel() > 1, _lib.mat(out, "out"), _lib.mat(lse, "lse"), _lib.mat(gout, "gout"), _lib.mat(g_m, "g_m"),
                g_t, part, n_part.value, N, C, split, variant="g_t" if need[1] else None)
        if g_t is not None:  # the kernels leave g_t per channel: a scalar temperature's gradient is the sum
            g_t = (g_t if tv.numel() > 1 else g_t.sum()).reshape(ctx.t_shape)
        return g_m if need[0] else None, g_t, None, None


def softmax_aggregate_supported(C):
    return bool(_lib.load().rgbx_softmax_aggr_supported(C))


def softmax_aggregate(m, t, graph):
    """One softmax aggregation [PyG SoftmaxAggregation; DeeperGCN] of the messages m [N, C] (rows contiguous; a column
    block of a wider matrix is taken as it is) at the temperature t (a tensor on m's device: one element, or one per
    channel; it may take a gradient): out_i = sum_j softmax_j(t * m_j) * m_j, per channel, over the in-edges of i, the
    graph in mode LOOPS_KEEP (edges as given: self-loops stay, duplicates count twice, a node without in-edges gets
    zeros). t = 0 is the mean, large t the maximum, negative t a soft minimum. No dropout, no random state."""
    if _is_dist(graph):
        raise RuntimeError("GENConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(m, t)
    if m.dim() != 2 or not softmax_aggregate_supported(m.size(1)):
        raise RuntimeError(f"softmax_aggregate: m {tuple(m.shape)}: the kernels take [N, C] with any C <= 64, even "
                           "C <= 128 or C % 4 == 0 up to 256; pad the width (GENConv does)")
    if m.size(0) != graph.fwd.N or t.numel() not in (1, m.size(1)) or t.dtype != torch.float32:
        raise RuntimeError(f"softmax_aggregate: m {tuple(m.shape)} / t {tuple(t.shape)} for a graph of {graph.fwd.N} "
                           "nodes (t: one float32, or one per channel)")
    want_grad = torch.is_grad_enabled() and (m.requires_grad or t.requires_grad)
    return _SoftmaxAggregate.apply(m, t, graph, want_grad)


FACONV_FORMS = ("fused", "composed")


def faconv_supported(C):
    return bool(_lib.load().rgbx_faconv_supported(C))


def faconv_form(C, form=None):
    """'fused' (rgbx_faconv_fwd / bwd_dst / bwd_src: nothing per edge is written) where the kernels take the width,
    else 'composed' (per-slot coefficients written by rgbx_faconv_edge_coef_f32, then the plain weighted gather).
    `form` forces one of FACONV_FORMS (tests, tools/fagcn_bench.py); forcing 'fused' at a refused width raises."""
    if form is None:
        return "fused" if faconv_supported(C) else "composed"
    if form not in FACONV_FORMS:
        raise ValueError(f"faconv: form {form!r} not in {FACONV_FORMS}")
    if form == "fused" and not faconv_supported(C):
        raise RuntimeError(f"faconv: the fused kernels do not take width {C}; use form='composed'")
    return form


def faconv_random_choices(record, graph):
    """The dropout decisions of the training forward that filled `record` (FAConv keeps the record of its last
    forward): {'keep': bool [E'] in forward CSR slot order, 'src' / 'dst': int64 [E'] endpoints of every slot}."""
    csr = graph.fwd
    dev, nnz = csr.rowptr.device, csr.nnz
    if record.get("seed") is None:
        keep = torch.ones(nnz, dtype=torch.uint8, device=dev)
    else:
        keep = torch.empty(nnz, dtype=torch.uint8, device=dev)
        _lib.launch("rgbx_faconv_draws_u8", record["seed"], nnz, float(record["p_drop"]), keep)
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    return {"keep": keep.bool(), "src": csr.col[:nnz].long(),
            "dst": torch.repeat_interleave(torch.arange(csr.N, device=dev), deg)}


def _faconv_edge_coef(csr, w, slot, alr, transposed, seed, p_drop, want_q):
    coef = torch.empty(max(csr.nnz, 1), dtype=torch.float32, device=alr.device)
    q = torch.empty_like(coef) if want_q else None
    _launch("faconv_edge_coef", "rgbx_faconv_edge_coef_f32", csr.rowptr, csr.col, w, slot, alr, int(transposed), csr.N,
            seed, float(p_drop), coef, q)
    return coef, q


def _faconv_edge_dot(csr, q, a, b, out, column):
    """out[:, column] = per-row sums of q[p] <a[row], b[col[p]]> (out [N, 2])."""
    _launch("faconv_edge_dot", "rgbx_faconv_edge_dot_f32", csr.rowptr, csr.col, q, _lib.mat(a, "a"), _lib.mat(b, "b"),
            out.data_ptr() + 4 * column, 2, csr.N, a.size(1))


class _FAConv(torch.autograd.Function):
    """One FAConv as a single autograd node: out_i = sum_j k a_ij w_ij x_j + eps x0_i with a_ij = tanh(al_j + ar_i).
    Saves x, [al, ar], the attention vectors and the dropout seed; nothing per edge (the backward recomputes tanh and
    the keep decisions)."""

    @staticmethod
    def forward(ctx, x, x0, att_l, att_r, graph, eps, train, p_drop, form, record):
        _lib.require_device(x, x0, att_l, att_r)
        csr, N, dev = graph.fwd, graph.fwd.N, x.device
        C = x.size(1)
        vec = _width_vec(C)  # faconv.hip fa_vec: the kernels read rows that wide
        x = _rows_on_grid(x.contiguous(), vec)
        if x.size(0) != N:
            raise RuntimeError(f"faconv: {x.size(0)} feature rows for a graph of {N} nodes")
        use_x0 = x0 is not None and eps != 0.0
        x0c = _rows_on_grid(x0.contiguous(), vec) if use_x0 else None
        att = torch.cat([att_l.detach().reshape(1, C), att_r.detach().reshape(1, C)]).contiguous()  # [2, C]
        seed = None
        if train and p_drop > 0.0:
            # two 32-bit words from torch's device generator (torch.manual_seed makes the run repeatable; under a
            # hipGraph capture the generator's offset advances with every replay); they stay on the device
            seed = torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=dev)
        if record is not None:
            record.update(seed=seed, p_drop=float(p_drop))
        alr = torch.empty((N, 2), dtype=torch.float32, device=dev)
        xm = _lib.mat(x, "x")
        _launch("faconv_scores", "rgbx_faconv_scores_f32", xm, att[0], att[1], alr, N, C)
        if form == "fused":
            out = torch.empty((N, C), dtype=torch.float32, device=dev)
            split, _scratch = csr.split_arg(C + 1, dev)
            _launch("faconv_fwd", "rgbx_faconv_fwd_f32", csr.rowptr, csr.col, graph.w, xm, alr,
                    _lib.mat(x0c, "x_0") if use_x0 else (0, 0), float(eps), _lib.mat(out, "out"), N, C, seed, float(p_drop),
                    split)
        else:
            coef, _ = _faconv_edge_coef(csr, graph.w, None, alr, 0, seed, p_drop, False)
            out = spmm_raw(csr, coef, None, x, y=x0c, a=1.0, b=float(eps), kind="faconv_fwd_composed")
        ctx.graph, ctx.eps, ctx.p_drop, ctx.form, ctx.use_x0 = graph, float(eps), float(p_drop), form, use_x0
        ctx.att_shapes = (att_l.shape, att_r.shape)
        ctx.save_for_backward(x, alr, att, seed)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, alr, att, seed = ctx.saved_tensors
        g, p_drop = ctx.graph, ctx.p_drop
        N, C, dev = x.size(0), x.size(1), x.device
        gout = _rows_on_grid(gout.contiguous(), _width_vec(C))
        g_alr = torch.empty((N, 2), dtype=torch.float32, device=dev)
        xm, gm = _lib.mat(x, "x"), _lib.mat(gout, "gout")
        t2f = g.t2f if seed is not None else None
        if ctx.form == "fused":
            g_x = torch.empty_like(x)
            split, _scratch = g.fwd.split_arg(C + 1, dev)
            _launch("faconv_bwd_dst", "rgbx_faconv_bwd_dst_f32", g.fwd.rowptr, g.fwd.col, g.w, xm, alr, gm, g_alr, N, C,
                    seed, p_drop, split)
            split, _scratch2 = g.bwd.split_arg(C + 1, dev)
            _launch("faconv_bwd_src", "rgbx_faconv_bwd_src_f32", g.bwd.rowptr, g.bwd.col, g.w_t, t2f, xm, alr, gm, att[0],
                    att[1], g_alr, _lib.mat(g_x, "g_x"), N, C, seed, p_drop, split)
        else:
            _, q = _faconv_edge_coef(g.fwd, g.w, None, alr, 0, seed, p_drop, True)
            _faconv_edge_dot(g.fwd, q, gout, x, g_alr, 1)
            coef_t, q_t = _faconv_edge_coef(g.bwd, g.w_t, t2f, alr, 1, seed, p_drop, True)
            _faconv_edge_dot(g.bwd, q_t, x, gout, g_alr, 0)
            g_x = torch.addmm(spmm_raw(g.bwd, coef_t, None, gout, kind="faconv_bwd_composed"), g_alr, att)
        g_att = gemm_tn(g_alr, x)  # [2, C]: rows g_att_l, g_att_r, summed in slab order
        g_x0 = gout * ctx.eps if ctx.use_x0 and ctx.needs_input_grad[1] else None
        return (g_x, g_x0, g_att[0].reshape(ctx.att_shapes[0]), g_att[1].reshape(ctx.att_shapes[1]), None, None, None,
                None, None, None)


def faconv(x, x0, att_l, att_r, graph, eps=0.1, training=False, p_drop=0.0, form=None, record=None):
    """FAConv on the GCN-weighted graph (graph mode LOOPS_ADD_REMAINING): out_i = sum_j k_ij tanh(<x_j, att_l> +
    <x_i, att_r>) w_ij x_j + eps x0_i. In training mode with p_drop > 0 the layer draws its dropout seed from torch's
    device generator; `record` (a dict) receives it, for faconv_random_choices. `form`: see faconv_form."""
    if _is_dist(graph):
        raise RuntimeError("FAConv has no node-partitioned form: run it on one GPU")
    _lib.require_device(x, x0, att_l, att_r)
    if not (0.0 <= p_drop < 1.0):
        raise ValueError("faconv: dropout must be in [0, 1)")
    return _FAConv.apply(x, x0, att_l, att_r, graph, float(eps), bool(training), float(p_drop),
                         faconv_form(x.size(1), form), record)


def _scores_in_kernel(C):
    """Forming <h_j, att_src> from the gathered row costs log2(lanes per head) cross-lane adds per
    neighbour and saves the a_src[j] cache-line request. Measured at |V|=2M, |E|=60M: 4 lanes per head
    (H=8, C=16) 6.20 -> 5.51 ms; 32 lanes per head (H=1, C=128) 5.71 -> 6.02 ms. Use it up to 8 lanes."""
    vec = _width_vec(C)
    lanes = 1
    while lanes * vec < C:
        lanes *= 2
    return lanes <= 8


def gather_rows(src, idx, out=None):
    """out[r] = src[idx[r]] (idx int32, device)."""
    _lib.require_device(src, idx)
    sm = _lib.mat(src, "src")
    n, d = idx.numel(), src.size(1)
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=src.device)
    _lib.launch("rgbx_gather_rows_f32", sm, idx, n, d, _lib.mat(out, "dst"))
    return out


def scatter_add_rows(src, idx, dst):
    """dst[idx[r]] += src[r]; idx entries unique."""
    _lib.require_device(src, idx, dst)
    _lib.launch("rgbx_scatter_add_rows_f32", _lib.mat(src, "src"), idx, idx.numel(), src.size(1), _lib.mat(dst, "dst"))
    return dst


# ---- dense layers: forward through hipBLASLt, weight gradient through the split-K MFMA kernel --------

def gemm_tn(a, b, alpha=1.0, colsum=False, out=None, sums_out=None):
    """a^T b for a [K,M], b [K,N] (fp32, device): rgbx_gemm_tn_f32. With `colsum` also the column sums of `a`
    ([M], from the same pass): returns (a^T b, a.sum(0)). `out` ([M, N] contiguous) / `sums_out` ([M]): write there
    (e.g. views of one flat gradient buffer)."""
    _lib.require_device(a, b)
    a = a if a.stride(-1) == 1 and _rows_padded_readable(a) else a.contiguous()
    b = b if b.stride(-1) == 1 and _rows_padded_readable(b) else b.contiguous()
    # rows off the 16-byte grid (width % 4 != 0 at its natural stride: dY [N, 7], a dropout copy of [N, 1433] features) take
    # the kernel's 4-byte path: 16.5 ms against 5.0 for 2 M x 64 x 1433, 0.83 against 0.37 for 2 M x 7 x 64. One padded copy
    # (align_rows: a read and a write of the operand) buys the 16-byte path — 3 ms for the 11.5 GB operand.
    if a.size(0) >= 4096:
        a, b = (_aligned_rows(t) for t in (a, b))
    am, bm = _lib.mat(a, "a"), _lib.mat(b, "b")
    K, M, N = a.size(0), a.size(1), b.size(1)
    nbytes = ctypes.c_size_t(0)
    _lib.call("rgbx_gemm_tn_workspace_bytes", K, M, N, ctypes.byref(nbytes))
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=a.device)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    elif tuple(out.shape) != (M, N) or not out.is_contiguous() or out.dtype != torch.float32:
        raise RuntimeError(f"gemm_tn: out must be a contiguous float32 [{M}, {N}] tensor")
    sums = None
    if colsum:
        sums = sums_out if sums_out is not None else torch.empty(M, dtype=torch.float32, device=a.device)
        if tuple(sums.shape) != (M,) or not sums.is_contiguous() or sums.dtype != torch.float32:
            raise RuntimeError(f"gemm_tn: sums_out must be a contiguous float32 [{M}] tensor")
    _launch("gemm_tn", "rgbx_gemm_tn_f32", am, bm, out, N, sums, K, M, N, float(alpha), ws, ws.numel(),
            variant=f"{M}x{N}" if _EVENT_SINK is not None else None)
    return (out, sums) if colsum else out


def _gemm_tn_v4(*mats):
    """Operands the 16-byte-only forms of the GEMM take as they are: float32 device matrices, contiguous 16-byte aligned
    rows, widths that are multiples of 4."""
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.size(1) % 4 == 0
               and t.stride(0) % 4 == 0 and t.stride(0) >= t.size(1) and t.data_ptr() % 16 == 0 for t in mats)


def _gemm_tn_buffers(K, M, N, device, colsum):
    nbytes = ctypes.c_size_t(0)
    _lib.call("rgbx_gemm_tn_workspace_bytes", K, M, N, ctypes.byref(nbytes))
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=device)
    out = torch.empty((M, N), dtype=torch.float32, device=device)
    return ws, out, torch.empty(M, dtype=torch.float32, device=device) if colsum else None


def gemm_tn_bn_bwd(g, x, mean, rstd, ca, cb, ck, b, colsum=False):
    """gemm_tn(gx, b, colsum=colsum) for gx = BatchNorm's input gradient bwd_apply(g, x, mean, rstd, ca, cb, ck), which
    is formed inside the GEMM as its A tiles are staged (rgbx_gemm_tn_bn_bwd_f32) instead of being written and read
    back: same result, bit for bit. Operands off the 16-byte path take the two launches."""
    from .nn import batchnorm as B
    _lib.require_device(g, x, b)
    if not _gemm_tn_v4(g, x, b) or g.shape != x.shape:
        res = gemm_tn(B.bwd_apply(g, x, mean, rstd, ca, cb, ck), b, colsum=colsum)
        return res if colsum else (res, None)
    K, M, N = g.size(0), g.size(1), b.size(1)
    consts = [t.contiguous() for t in (mean, rstd, ca, cb, ck)]
    ws, out, sums = _gemm_tn_buffers(K, M, N, g.device, colsum)
    _launch("gemm_tn", "rgbx_gemm_tn_bn_bwd_f32", _lib.mat(g, "g"), _lib.mat(x, "x"), *consts, _lib.mat(b, "b"), out, N,
            sums, K, M, N, 1.0, ws, ws.numel(), variant=f"{M}x{N}+bn_bwd" if _EVENT_SINK is not None else None)
    return out, sums


def gemm_tn_rows(a, b, rows, colsum=False, rows_only=False):
    """gemm_tn(a, b, colsum=colsum) for an `a` that is zero outside the rows of the ascending int32 device list `rows`
    (selected_rows): only those rows of a and b are read (rgbx_gemm_tn_rows_f32), every non-zero product is added where
    the full product adds it: same result, bit for bit. rows = None, or operands off the 16-byte path: the full
    product — an error with `rows_only` (the other rows of a and b were never written)."""
    _lib.require_device(a, b)
    if rows is None or not _gemm_tn_v4(a, b) or a.size(0) != b.size(0) or a.size(0) >= 2**31:
        if rows_only:
            raise RuntimeError("gemm_tn_rows: the row-list form cannot take these operands and the full product may not "
                               "read them")
        return gemm_tn(a, b, colsum=colsum)
    K, M, N = a.size(0), a.size(1), b.size(1)
    ws, out, sums = _gemm_tn_buffers(K, M, N, a.device, colsum)
    _launch("gemm_tn", "rgbx_gemm_tn_rows_f32", _lib.mat(a, "a"), _lib.mat(b, "b"), rows, rows.numel(), out, N, sums, K, M,
            N, 1.0, ws, ws.numel(), variant=f"{M}x{N}+rows" if _EVENT_SINK is not None else None)
    return (out, sums) if colsum else out


class _Linear(torch.autograd.Function):
    """y = x W^T (+ b). dW = dy^T x runs on rgbx_gemm_tn_f32 when the tensors are on the GPU."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if _EVENT_SINK is None or not x.is_cuda:
            return torch.nn.functional.linear(x, weight, bias)
        with _Timed("linear_fwd", f"{weight.size(1)}->{weight.size(0)}"):  # hipBLASLt; timed only for bench.py's tables
            return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gy @ weight if ctx.needs_input_grad[0] else None
        gw = gb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] and gy.is_cuda and want_b:
            gw, gb = gemm_tn(gy, x, colsum=True)  # dy is read once for dW and db
        else:
            if ctx.needs_input_grad[1]:
                gw = gemm_tn(gy, x) if gy.is_cuda else gy.t() @ x
            gb = gy.sum(0) if want_b else None
        return gx, gw, gb


def linear(x, weight, bias=None):
    sp = getattr(x, "_rgbx_sparse", None)
    if sp is not None and not x.requires_grad:  # static features with few non-zeros (prepare_features)
        return _SparseRowsLinear.apply(sp, weight, bias)
    return _Linear.apply(x, weight, bias)


SHORT_ROWS_TABLE_BYTES = 2 << 20  # half of one XCD's 4 MB L2: the gathered table must stay cache-resident beside the streams
SHORT_ROWS_MEAN_SLOTS = 64


def short_rows_ok(csr, table):
    """rgbx_spmm_csr_short_rows_f32 (a lane group per target row) is the better form: rows of tens of slots over a table that
    stays in L2 — the product over a bag-of-words matrix's non-zeros. Measured at N = 2 M, 36 M non-zeros (profiles/
    r05_short_rows.txt)."""
    d = table.size(1)
    # d <= 64: beyond, both forms read nnz * d * 4 bytes from L2 at its rate (d = 128: 1.13 ms row per wave, 1.20 ms here)
    return (table.is_cuda and d % 4 == 0 and 4 <= d <= 64 and table.numel() * 4 <= SHORT_ROWS_TABLE_BYTES
            and csr.nnz <= SHORT_ROWS_MEAN_SLOTS * max(csr.N, 1))


def spmm_short_rows_raw(csr, w, x, bias=None, kind="spmm"):
    """out[i,:] = sum_p w[p] x[col[p],:] (+ bias) on rgbx_spmm_csr_short_rows_f32 (no autograd)."""
    _lib.require_device(x, w, bias)
    xm = _lib.mat(x, "x")
    N, d = csr.N, x.size(1)
    out = torch.empty((N, d), dtype=torch.float32, device=x.device)
    _launch(kind, "rgbx_spmm_csr_short_rows_f32", csr.rowptr, csr.col, w, xm, bias, out, d, N, d,
            variant=f"shortrows+d{d}" if _EVENT_SINK is not None else None)
    return out


class SparseFeatures:
    """What ops.dropout returns for features that ride on their non-zeros: not a tensor — only ops.linear (nn.Linear of this
    package) takes it; anything else fails loudly instead of reading undropped dense values."""
    requires_grad = False

    def __init__(self, sp, like):
        self._rgbx_sparse, self.shape, self.device, self.dtype, self.is_cuda = sp, like.shape, like.device, like.dtype, True

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return len(self.shape)


def dropout(x, p, training):
    """F.dropout for a model's INPUT features (reference models/dagnn.py:72: dropout before the first Linear). Dense
    features: torch's. Features carried by their non-zeros (prepare_features) in a training forward: dropout leaves a zero a
    zero, so the Bernoulli mask is drawn for the non-zeros alone — the same distribution of outputs, from nnz draws instead
    of a fresh dense [N, F] matrix per step (11.5 GB written and read again at N = 2 M, F = 1433) — and the product stays on
    the non-zeros. (The mask comes from torch's device generator: reproducible under manual_seed; no implementation on
    another device reproduces the reference's CUDA Philox stream anyway.)"""
    sp = getattr(x, "_rgbx_sparse", None)
    if sp is None or not training or p <= 0.0 or x.requires_grad:
        return torch.nn.functional.dropout(x, p=p, training=training)
    if p >= 1.0:
        return SparseFeatures(sp.with_values(torch.zeros_like(sp.val)), x)
    keep = torch.rand(sp.val.numel(), device=sp.val.device) >= p
    return SparseFeatures(sp.with_values(sp.val * keep * (1.0 / (1.0 - p))), x)


class SparseRows:
    """The non-zeros of a STATIC feature matrix [n, f] as a CSR (rows -> (column, value)) and its transpose (columns ->
    (row, value)), built once per matrix with torch index ops (plumbing: one pass over the matrix and one stable sort of the
    non-zeros). The reference's datasets are bag-of-words (Cora: 18 non-zeros of F = 1433 per row) that it multiplies as
    dense matrices; x W^T and dW = dY^T x over the non-zeros alone are two launches of the row-gather kernel
    (rgbx_spmm_csr_f32: the weights are the feature values, the gathered table W^T [f, out] resp. dY [n, out]) and read
    nnz * out * 4 bytes instead of n * f * 4 — the same sums up to float32 rounding order (zeros contribute exactly 0)."""

    def __init__(self, x):
        from .graph import CSR, make_row_split
        _lib.require_device(x)
        n, f = x.shape
        # row-major order, in row blocks of at most 2^28 entries: torch's nonzero() indexes with 32 bits (2 M x 1433 entries
        # in one call ended in an allocation of 2^56 bytes, round 5)
        step = max(1, (1 << 28) // max(f, 1))
        rows, cols, vals = [], [], []
        for r0 in range(0, n, step):
            blk = x[r0:r0 + step]
            nz = blk.nonzero(as_tuple=False)
            rows.append(nz[:, 0] + r0)
            cols.append(nz[:, 1].contiguous())
            vals.append(blk[nz[:, 0], nz[:, 1]])
        rows, cols, vals = (torch.cat(t).contiguous() if t else x.new_zeros(0, dtype=dt)
                            for t, dt in ((rows, torch.int64), (cols, torch.int64), (vals, x.dtype)))
        self.n, self.f, self.nnz = n, f, int(rows.numel())
        if self.nnz >= 2 ** 31 - 1:
            raise RuntimeError("SparseRows: more than 2^31 non-zeros")
        i32 = lambda t: t.to(torch.int32).contiguous()

        def rowptr_of(idx, m):
            ptr = torch.zeros(m + 1, dtype=torch.int64, device=x.device)
            ptr[1:] = torch.cumsum(torch.bincount(idx, minlength=m), 0)
            return i32(ptr)

        pad = lambda t: t if t.numel() else t.new_zeros(1)  # (the kernels take a non-null pointer)
        ptr = rowptr_of(rows, n)
        self.fwd = CSR(ptr, pad(i32(cols)), None, n, self.nnz, make_row_split(ptr))
        self.val = pad(vals)
        order = torch.argsort(cols, stable=True)
        self.order = order  # slot of the transposed CSR -> slot of the forward CSR
        ptr_t = rowptr_of(cols, f)
        self.bwd = CSR(ptr_t, pad(i32(rows[order])), None, f, self.nnz, make_row_split(ptr_t))
        self.val_t = pad(vals[order].contiguous())

    def with_values(self, vals):
        """The same structure (shared, not copied) under other values per non-zero, given in the forward CSR's slot order."""
        import copy
        other = copy.copy(self)
        other.val = vals.contiguous()
        other.val_t = vals[self.order].contiguous() if self.nnz else vals
        return other


class _SparseRowsLinear(torch.autograd.Function):
    """y = x W^T (+ b) and dW = dY^T x, db = column sums of dY, for x given by its non-zeros (SparseRows). x takes no gradient."""

    @staticmethod
    def forward(ctx, sp, weight, bias):
        ctx.sp, ctx.has_bias = sp, bias is not None
        wt = weight.detach().t().contiguous()  # [f, out]: the gathered table (L2-resident: 367 KB for 1433 x 64)
        b = None if bias is None else bias.detach().contiguous()
        if short_rows_ok(sp.fwd, wt):
            return spmm_short_rows_raw(sp.fwd, sp.val, wt, bias=b, kind="features_fwd")
        return spmm_raw(sp.fwd, sp.val, None, wt, kind="features_fwd", bias=b)

    @staticmethod
    def backward(ctx, gy):
        sp = ctx.sp
        gy = gy.contiguous()
        gw = gb = None
        if ctx.needs_input_grad[1]:
            gw = spmm_raw(sp.bwd, sp.val_t, None, gy, kind="features_bwd").t()  # [f, out] -> dW [out, f]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(0)
        return None, gw, gb


def prepare_features(x, max_density=0.1):
    """The layout experiment() gives the static input features on the GPU: rows on 16-byte boundaries (align_rows) and,
    when at most `max_density` of the entries are non-zero (bag-of-words features: Cora 1.3 %), their non-zeros as a
    SparseRows riding on the tensor — ops.linear then multiplies over the non-zeros alone. Same values, same shape."""
    x = align_rows(x)
    if x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad and x.numel():
        step = max(1, (1 << 28) // x.size(1))  # (row blocks: see SparseRows)
        nnz = sum(int(torch.count_nonzero(x[r0:r0 + step])) for r0 in range(0, x.size(0), step))
        if nnz <= max_density * x.numel() and nnz < 2 ** 31 - 1:
            x._rgbx_sparse = SparseRows(x)  # (this Python object only: a slice or a copy is an ordinary dense tensor)
    return x


# ---- masked NLL + accuracy ------------------------------------------------------------------------

def _nll_stats(logp, y, mask, want_acc):
    _lib.require_device(logp, y, mask)
    if y.dtype != torch.int64:
        raise RuntimeError(f"labels must be int64, got {y.dtype}")
    if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"mask must be bool, got {mask.dtype}")
    lm = _lib.mat(logp, "logp")
    stats = torch.empty(3, dtype=torch.float64, device=logp.device)
    n_scr = ctypes.c_int64(0)
    _lib.call("rgbx_masked_nll_scratch_doubles", logp.size(0), int(want_acc), ctypes.byref(n_scr))
    scratch = torch.empty(n_scr.value, dtype=torch.float64, device=logp.device)
    y = y.contiguous()
    mask = None if mask is None else mask.contiguous()
    _lib.launch("rgbx_masked_nll_fwd_f32", lm, y, mask, logp.size(0), logp.size(1), stats, scratch, n_scr.value,
                int(want_acc))
    return stats, y, mask


class _MaskedNLL(torch.autograd.Function):
    """nn.NLLLoss()(logp[mask], y[mask]) without materialising the selection (itexperiments.py:400,429).
    reduction 'mean' divides by the number of selected rows, 'sum' does not."""

    @staticmethod
    def forward(ctx, logp, y, mask, reduction):
        logp = logp if logp.stride(-1) == 1 else logp.contiguous()
        stats, y, mask = _nll_stats(logp, y, mask, False)
        ctx.y, ctx.mask, ctx.shape, ctx.reduction = y, mask, logp.shape, reduction
        ctx.count = stats[1]
        return (stats[0] / stats[1] if reduction == "mean" else stats[0]).float()

    @staticmethod
    def backward(ctx, g):
        scale = (g.double() / ctx.count if ctx.reduction == "mean" else g.double()).float().reshape(1).contiguous()
        N, C = ctx.shape
        grad = torch.empty((N, C), dtype=torch.float32, device=g.device)
        _lib.launch("rgbx_masked_nll_bwd_f32", ctx.y, ctx.mask, N, C, scale, grad, C)
        return grad, None, None, None


def masked_nll_loss(logp, y, mask=None, reduction="mean"):
    return _MaskedNLL.apply(logp, y, mask, reduction)


def _ce_stats(logits, y, mask):
    _lib.require_device(logits, y, mask)
    if y.dtype != torch.int64:
        raise RuntimeError(f"labels must be int64, got {y.dtype}")
    if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"mask must be bool, got {mask.dtype}")
    zm = _lib.mat(logits, "logits")
    stats = torch.empty(3, dtype=torch.float64, device=logits.device)
    n_scr = ctypes.c_int64(0)
    _lib.call("rgbx_masked_nll_scratch_doubles", logits.size(0), 1, ctypes.byref(n_scr))
    scratch = torch.empty(n_scr.value, dtype=torch.float64, device=logits.device)
    y = y.contiguous()
    mask = None if mask is None else mask.contiguous()
    _lib.launch("rgbx_masked_ce_fwd_f32", zm, y, mask, logits.size(0), logits.size(1), stats, scratch, n_scr.value)
    return stats, y, mask


class _MaskedCE(torch.autograd.Function):
    """NLLLoss(log_softmax(z)[mask], y[mask]) taken from the logits z: the loss, its gradient
    scale * (softmax - onehot) and (stats[2]) the arg-max hits, without writing log-softmax or a one-hot
    gradient. Returns (loss, stats [3] float64: nll sum, selected rows, correct)."""

    @staticmethod
    def forward(ctx, logits, y, mask, reduction):
        logits = logits if logits.stride(-1) == 1 else logits.contiguous()
        stats, y, mask = _ce_stats(logits, y, mask)
        ctx.save_for_backward(logits)
        ctx.y, ctx.mask, ctx.reduction = y, mask, reduction
        ctx.count = stats[1]
        ctx.mark_non_differentiable(stats)
        return (stats[0] / stats[1] if reduction == "mean" else stats[0]).float(), stats

    @staticmethod
    def backward(ctx, g, _g_stats):
        (logits,) = ctx.saved_tensors
        scale = (g.double() / ctx.count if ctx.reduction == "mean" else g.double()).float().reshape(1).contiguous()
        N, C = logits.shape
        grad = torch.empty((N, C), dtype=torch.float32, device=g.device)
        _lib.launch("rgbx_masked_ce_bwd_f32", _lib.mat(logits, "logits"), ctx.y, ctx.mask, N, C, scale, grad, C)
        return grad, None, None, None


def masked_ce_loss(logits, y, mask=None, reduction="mean", with_stats=False):
    """Cross-entropy of the raw logits on the masked rows = masked_nll_loss(log_softmax(logits), ...), in one
    pass each way. `with_stats`: also the [nll sum, count, correct] tensor of the same pass."""
    loss, stats = _MaskedCE.apply(logits, y, mask, reduction)
    return (loss, stats) if with_stats else loss


def masked_ce_accuracy(logits, y, mask=None):
    """masked_nll_accuracy(log_softmax(logits), ...) from the logits: float64 device tensor [3]."""
    logits = logits.detach()
    logits = logits if logits.stride(-1) == 1 else logits.contiguous()
    return _ce_stats(logits, y, mask)[0]


def masked_ce_accuracy_blocked(blk, y, mask=None, bias=None):
    """masked_ce_accuracy of logits held BLOCKED ([B, n, C / B]: the column slices a node-partitioned run's exchange
    delivers) plus `bias` per column, read in place — only the selected rows are touched (rgbx_masked_ce_fwd_blocked_f32)."""
    _lib.require_device(blk, y, mask, bias)
    if y.dtype != torch.int64:
        raise RuntimeError(f"labels must be int64, got {y.dtype}")
    if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"mask must be bool, got {mask.dtype}")
    ptr, bc, bs = _blocked(blk, "logits")
    n, C = blk.size(1), blk.size(0) * blk.size(2)
    stats = torch.empty(3, dtype=torch.float64, device=blk.device)
    n_scr = ctypes.c_int64(0)
    _lib.call("rgbx_masked_nll_scratch_doubles", n, 1, ctypes.byref(n_scr))
    scratch = torch.empty(n_scr.value, dtype=torch.float64, device=blk.device)
    y = y.contiguous()
    mask = None if mask is None else mask.contiguous()
    b = None if bias is None else bias.detach().contiguous()
    _lib.launch("rgbx_masked_ce_fwd_blocked_f32", ptr, bc, bs, b, y, mask, n, C, stats, scratch, n_scr.value)
    return stats


def masked_nll_accuracy(logp, y, mask=None):
    """(sum of -logp[i,y_i], selected-row count, correct arg-max count) as a float64 device tensor [3]."""
    logp = logp.detach()
    logp = logp if logp.stride(-1) == 1 else logp.contiguous()
    return _nll_stats(logp, y, mask, True)[0]


# ---- neighbour sampling: fan-out mini-batches (csrc/sample.hip) -----------------------------------

SAMPLE_STREAM = 0x082EFA98        # kStreamSample: the stream word of hop 0 (hop h: + h, modulo 2^32)
SAMPLE_SHORT_ROW_SLOTS = 64       # rows up to here: 16 lanes per row
SAMPLE_WAVE_ROW_SLOTS = 1024      # rows up to here: a wave per row; longer ones a workgroup per row


def check_fanout(fanout):
    """A fan-out is an int >= 1, or -1 for every slot (ValueError otherwise)."""
    if isinstance(fanout, bool) or not isinstance(fanout, int) or fanout == 0 or fanout < -1:
        raise ValueError(f"fan-out must be an int >= 1, or -1 for all neighbours; got {fanout!r}")
    return fanout


def sample_seed(device):
    """Two 32-bit seed words on the device, from torch's device generator (as the attention dropouts take theirs)."""
    return torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32, device=device)


def _sample_workspace(n_rows, n_cand, N, device):
    nbytes = ctypes.c_size_t(0)
    _lib.call("rgbx_sample_workspace_bytes", n_rows, n_cand, N, ctypes.byref(nbytes))
    return torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=device)


def sample_hop_raw(csr, rows, fanout, seed, hop):
    """One hop over `csr` for the int32 device vector `rows`: (rowptr int32 [n_rows + 1], col int32 [n_e], slot int32
    [n_e]). One read-back: the hop's edge count (with the two row-length class counts, which decide the kernels)."""
    n_rows, dev = rows.numel(), rows.device
    head = torch.empty(n_rows + 3, dtype=torch.int32, device=dev)  # the row pointer, then the two class counts
    ws = _sample_workspace(n_rows, 0, csr.N, dev)
    _launch("sample_count", "rgbx_sample_count", csr.rowptr, csr.N, rows, n_rows, fanout, head, head[n_rows + 1:], ws,
            ws.numel())
    n_edges, n_wave, n_hub = head[n_rows:].tolist()
    if n_edges < 0 or n_edges > csr.nnz:  # distinct rows keep at most every slot once
        raise RuntimeError(f"sample_neighbors: {n_edges} sampled slots of {csr.nnz}: the rows are not distinct")
    col = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)  # (an empty tensor has no pointer to pass)
    slot = torch.empty(max(n_edges, 1), dtype=torch.int32, device=dev)
    classes = 1 | (2 if n_wave else 0) | (4 if n_hub else 0)
    _launch("sample_pick", "rgbx_sample_pick", csr.rowptr, csr.col, csr.N, rows, n_rows, fanout, seed, hop, head, col, slot,
            classes)
    return head[:n_rows + 1], col[:n_edges], slot[:n_edges]


def sample_neighbors(graph, rows, fanout, seed, hop):
    """One hop of the neighbour sampler over `graph.fwd` (a graph.Graph in LOOPS_KEEP mode: nothing added, duplicate edges
    are separate slots): row g of `rows` (distinct global ids, device) keeps min(fanout, deg) of its slots (fanout = -1:
    all) — the ones with the smallest keys draw32(seed[0], seed[1], SAMPLE_STREAM + hop, g, t) << 32 | t — in ascending
    slot order. Returns (rowptr int32 [n_rows + 1], col int32 [n_e] global source ids, slot int32 [n_e] CSR slots).
    `seed`: two int32 words on the device. There is no CPU fallback."""
    from .graph import LOOPS_KEEP
    check_fanout(fanout)
    if isinstance(hop, bool) or not isinstance(hop, int) or hop < 0:
        raise ValueError(f"hop must be an int >= 0, got {hop!r}")
    if getattr(graph, "is_distributed", False):
        raise NotImplementedError("neighbour sampling on a partitioned graph is not implemented")
    if graph.loops_mode != LOOPS_KEEP:
        raise ValueError("sample_neighbors draws from the input edges: the graph must be built with LOOPS_KEEP")
    _lib.require_device(rows, seed)
    if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"rows must be a 1-D int32 / int64 tensor, got {rows.dtype} {tuple(rows.shape)}")
    if seed.dtype != torch.int32 or seed.numel() != 2:
        raise ValueError("seed must hold two int32 words")
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= graph.N):
        raise ValueError(f"rows outside [0, {graph.N})")
    return sample_hop_raw(graph.fwd, rows.to(torch.int32).contiguous(), fanout, seed.contiguous(), hop)


def sample_frontier(cand, local_of, first_local):
    """The distinct ids of `cand` (int32, device) that are not in the batch yet (local_of < 0), ascending: they get the
    local ids first_local, first_local + 1, ... in `local_of` and are returned (int32). One read-back: their count."""
    n, dev = cand.numel(), cand.device
    new_ids = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = _sample_workspace(0, n, local_of.numel(), dev)
    _launch("sample_frontier", "rgbx_sample_frontier", cand.data_ptr(), n, local_of, local_of.numel(), first_local, new_ids,
            count, ws, ws.numel())
    return new_ids[:int(count.item())]


def sample_set_local(ids, first_local, local_of):
    """local_of[ids[i]] = first_local + i; first_local = -1 resets them to -1 (touches len(ids) entries)."""
    _launch("sample_local", "rgbx_sample_set_local", ids.data_ptr(), ids.numel(), first_local, local_of, local_of.numel())


def sample_relabel(rowptr, col, slot, local_of, perm, first_row):
    """A hop's edges in batch ids: (edge_index int64 [2, n_e] with source row 0 and target row 1, e_id int64 [n_e])."""
    n_e, dev = col.numel(), col.device
    ei = torch.empty((2, max(n_e, 1)), dtype=torch.int64, device=dev)
    e_id = torch.empty(max(n_e, 1), dtype=torch.int64, device=dev)
    _launch("sample_relabel", "rgbx_sample_relabel", rowptr, rowptr.numel() - 1, col.data_ptr(), slot.data_ptr(), n_e,
            local_of, local_of.numel(), perm, first_row, ei[0], ei[1], e_id)
    return ei[:, :n_e], e_id[:n_e]
