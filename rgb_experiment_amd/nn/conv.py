"""Conv layers with the parameter names and semantics of the PyG layers the reference imports,
computing their ``propagate`` in HIP kernels (rgb_experiment_amd.ops).

  GCNConv    <- torch_geometric.nn.conv.GCNConv   (reference models/gcn.py:3,18-21)
  SAGEConv   <- torch_geometric.nn.conv.SAGEConv  (reference models/graphsage2.py:5,20-23)
  MySAGEConv <- my_SAGEConv                       (reference models/graphsage.py:36-62)
  GATConv    <- torch_geometric.nn.conv.GATConv   (reference models/gat.py:3,18-21)
  APPNP      <- torch_geometric.nn.conv.APPNP     (reference models/appnp_stack.py:3,22)
  GatedGraphConv <- torch_geometric.nn.GatedGraphConv (reference models/ggnn.py:3,18)
  SuperGATConv <- torch_geometric.nn.SuperGATConv   (reference models/supergat.py)
  FAConv     <- torch_geometric.nn.conv.FAConv    (reference models/fagcn.py)

Dense X·W^T products go through hipBLASLt (forward, input gradient) and rgbx_gemm_tn_f32 (weight
gradient, split-K fp32 MFMA); everything indexed by edge_index goes through librgbx_hip.so.
"""
import copy
import math

import torch
import torch.nn as nn

from .. import _lib, ops
from .batchnorm import BatchNorm1d
from .linear import Linear
from ..graph import LOOPS_ADD_REMAINING, LOOPS_KEEP, LOOPS_REMOVE_ADD, get_graph


def glorot_(t):
    """PyG's glorot: U(-a, a), a = sqrt(6 / (size(-2) + size(-1)))."""
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)
    return t


def _no_weight_grad(edge_weight, who):
    if edge_weight is not None and edge_weight.requires_grad:
        raise ValueError(f"{who}: edge_weight must not require grad (the gradient in the edge weights is implemented for "
                         "GCNConv only)")


# accepted keyword -> canonical name
AGGRS = {"mean": "mean", "max": "max", "min": "min", "add": "add", "sum": "add", "std": "std", "var": "var"}


def _set_aggr(conv, aggr, lists=False):
    """The `aggr` keyword of the SAGE layers (reference models/graphsage.py:38-40: kwargs.setdefault('aggr', 'mean'), the
    caller may choose; PyG's SAGEConv takes the same keyword). 'mean' leaves the layer exactly as it is. The others run
    composed (ops.propagate_max / propagate_min / propagate_sum / propagate_std / propagate_var between the dense
    products): the loss-in-kernel, folded, cached-aggregate and fused aggregate + transform forms are all forms of a
    weighted row SUM with rows that sum to 1, so this instance switches them off.

    `lists`: the layer also takes a non-empty list / tuple of distinct names (PyG's MultiAggregation, mode='cat');
    conv.aggr is then the tuple of canonical names, aggregated in one pass by ops.propagate_multi — ['mean'] as well: only
    the STRING 'mean' keeps the layer's own routes. Returns the number of aggregates."""
    if isinstance(aggr, (list, tuple)):
        if not lists:
            raise ValueError(f"{type(conv).__name__}: aggr must be one name out of {sorted(AGGRS)} (the layer has no "
                             f"projection for a concatenation of aggregates), got {aggr!r}")
        names = tuple(AGGRS.get(a) if isinstance(a, str) else None for a in aggr)
        if not names or None in names or len(set(names)) != len(names):
            raise ValueError(f"{type(conv).__name__}: aggr must be one of {sorted(AGGRS)} or a non-empty list of distinct "
                             f"ones, got {aggr!r}")
        conv.aggr = names
    elif not isinstance(aggr, str) or aggr not in AGGRS:
        raise ValueError(f"{type(conv).__name__}: aggr must be one of {sorted(AGGRS)}, got {aggr!r}")
    else:
        conv.aggr = AGGRS[aggr]
    if conv.aggr != "mean":
        conv.accepts_ce = conv.accepts_ce_pair = conv.folds_post_affine = conv.emits_colsums = False
    return len(conv.aggr) if isinstance(conv.aggr, tuple) else 1


# accepted gather_dtype keyword -> storage dtype of the gathered matrix
GATHER_DTYPES = {torch.bfloat16: torch.bfloat16, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


def _set_gather_dtype(conv, gather_dtype):
    """The `gather_dtype` keyword of GCNConv / SAGEConv / MySAGEConv. None leaves the layer exactly as it is. torch.bfloat16
    ('bf16', 'bfloat16'): the neighbour rows are gathered from a bfloat16 copy (rounded once, to nearest-even) with fp32
    sums — ops.propagate_rows_bf16 / propagate_bf16, at the narrower of the layer's two widths, between the dense products.
    Every form that would gather fp32 rows instead (loss-in-kernel, column sums, the BatchNorm hand-over, folded,
    cached-aggregate, collapsed and fused aggregate + transform) is switched off for this instance, as _set_aggr does."""
    if gather_dtype is None:
        return
    known = isinstance(gather_dtype, (str, torch.dtype)) and gather_dtype in GATHER_DTYPES
    if not known:
        raise ValueError(f"{type(conv).__name__}: gather_dtype must be None, torch.bfloat16, 'bf16' or 'bfloat16', got "
                         f"{gather_dtype!r}")
    if getattr(conv, "aggr", "mean") != "mean":
        raise ValueError(f"{type(conv).__name__}: gather_dtype is implemented for aggr='mean' only, got aggr="
                         f"{conv.aggr!r}")
    conv.gather_dtype = GATHER_DTYPES[gather_dtype]
    conv.accepts_ce = conv.accepts_ce_pair = conv.emits_colsums = conv.owns_next_bn_backward = False


def _aggregate(x, graph, aggr):
    """The non-mean neighbourhood reductions of the SAGE layers over `graph` (single GPU); a tuple of names: their
    concatenation [N, k * d] from one gather pass."""
    if getattr(graph, "is_distributed", False):
        raise NotImplementedError(f"aggr={aggr!r} is not implemented on the partitioned (distributed) route")
    if isinstance(aggr, tuple):
        return ops.propagate_multi(x, graph, aggr)
    if aggr == "add":
        return ops.propagate_sum(x, graph)
    if aggr in ("std", "var"):
        return ops.propagate_std(x, graph) if aggr == "std" else ops.propagate_var(x, graph)
    return ops.propagate_max(x, graph) if aggr == "max" else ops.propagate_min(x, graph)


def _finish_composed(out, post_affine, ce):
    """What a caller of the composed forward may still have asked of the layer (the conv stack asks neither of an instance
    that reports no such form): an eval BatchNorm's affine map on the output, the masked cross-entropy from the logits."""
    if post_affine is not None:
        out = out * post_affine[0] + post_affine[1]
    return out if ce is None else ops.ce_from_logits(out, ce[0], ce[1])


def _forward_folded(conv, x, edge_index, operands, ce, loops_mode, kind, root, edge_weight=None):
    """Eval forward of a GCN / SAGE layer from prepared operands (W'^T, b', Wr'^T): ONE rgbx_fused_layer_f32 launch, no
    autograd node, no weight arithmetic on the way. Returns None when the fused kernel does not apply."""
    if operands is None or torch.is_grad_enabled() or not x.is_cuda:
        return None
    graph = get_graph(edge_index, x.size(0), loops_mode, edge_weight)
    if getattr(graph, "is_distributed", False) or not ops.fused_linear_ok(graph, conv.in_channels, conv.out_channels,
                                                                          root=root, x=x):
        return None
    wt, b, wtr = operands
    w = graph.w if kind == "gcn" else None
    rs = graph.inv_deg if kind == "mean" else None
    if ce is not None:
        y, mask = ce
        if not ops.fused_ce_ok(graph, conv.in_channels, conv.out_channels, root, x, y):
            return None
        _, _, stats = ops.fused_layer(x, wt, csr=graph.fwd, w=w, rs=rs, bias=b, x_root=x if root else None,
                                      wt_root=wtr if root else None, ce=(y, mask, None), kind=f"{kind}_linear_fwd",
                                      select_rows=True)
        return None, stats  # an eval forward is read through its statistics; the mean loss is stats[0] / stats[1]
    out, _, _ = ops.fused_layer(x, wt, csr=graph.fwd, w=w, rs=rs, bias=b, x_root=x if root else None,
                                wt_root=wtr if root else None, kind=f"{kind}_linear_fwd")
    return out


def _aggregate_input(x, edge_index, loops_mode, kind, edge_weight=None):
    """P x of the static input features (no autograd), or None where the cached-aggregate route does not apply."""
    if edge_weight is not None and edge_weight.requires_grad:
        return None  # the aggregate depends on weights that are being learned
    graph = get_graph(edge_index, x.size(0), loops_mode, edge_weight)
    if getattr(graph, "is_distributed", False) or not x.is_cuda or x.requires_grad:
        return None
    with torch.no_grad():
        return ops.propagate_gcn(x, graph) if kind == "gcn" else ops.propagate_mean(x, graph)


def _folded_from_aggregate(z, x, operands, root):
    """Eval forward from the kept aggregate and prepared operands (W'^T, b', Wr'^T): one DENSE launch."""
    wt, b, wtr = operands
    out, _, _ = ops.fused_layer(z, wt, bias=b, x_root=x if root else None, wt_root=wtr if root else None,
                                kind="cached_aggregate_linear_fwd")
    return out


class GCNConv(nn.Module):
    """out = A_hat (x W^T) + b, A_hat = D^-1/2 (A ∪ I) D^-1/2 with in-degree over the target index
    (gcn_norm restated at reference models/dagnn.py:12-31; message norm*x_j at dagnn.py:57-59).
    Parameters: ``lin.weight`` [out, in] (glorot, no bias), ``bias`` [out] (zeros).

    ``edge_weight`` (float32 [E], PyG's third argument) enters the normalisation as in gcn_norm(edge_index, edge_weight)
    (dagnn.py:12-31): an existing self-loop keeps its weight, added ones get 1, the degree is the weighted in-degree.
    Constant weights take every route of the unweighted layer on the weighted graph's per-slot weights. A weight that
    REQUIRES GRAD takes the transform-first route propagate(lin(x)) through ops.propagate_gcn_edge_weight, whose backward
    also returns dL/d edge_weight; the fused aggregate + transform kernels and the loss-in-kernel forms are skipped then."""

    folds_post_affine = True  # forward(..., post_affine=(scale, shift)): see models/_stack.py
    emits_colsums = True      # forward(..., want_colsums=True): the output may carry its column sums (ops.COLSUMS)
    owns_next_bn_backward = True  # forward(..., next_bn=bn): see ops.propagate_linear
    gather_dtype = None       # torch.bfloat16: the neighbour rows are gathered from a bfloat16 copy (_set_gather_dtype)

    def __init__(self, in_channels, out_channels, gather_dtype=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        _set_gather_dtype(self, gather_dtype)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.lin.weight)
        nn.init.zeros_(self.bias)

    accepts_ce = True         # forward(..., ce=(y, mask)): the model's last layer may take the loss into its kernel
    accepts_ce_pair = True    # ... and mask may be (mask_a, mask_b): (None, [2, 3] statistics) of one eval forward

    def forward(self, x, edge_index, edge_weight=None, post_affine=None, want_colsums=False, ce=None, next_bn=None):
        """`post_affine` = (scale, shift) of an eval-mode BatchNorm that follows this layer (no_grad only): a
        per-column affine map of a linear layer's output is the same layer with rows of W and b rescaled, so the
        normalisation costs two [out]-sized vector ops instead of a pass over [N, out].
        `want_colsums`: a training-mode BatchNorm follows; where the fused kernel runs, the output carries the column
        sums that BatchNorm needs (attribute ops.COLSUMS), taken from the MFMA tiles instead of a pass over it.
        `ce` = (y, mask): this is the model's last layer and the caller wants the masked cross-entropy of its logits,
        not the logits: returns (loss, stats [nll sum, selected rows, correct]); where the fused kernel runs the loss
        is taken from the output tiles and the logits are never written (ops.propagate_linear_ce).
        `next_bn`: the training-mode BatchNorm1d this output goes through into the next conv's forward_after_bn, and
        nowhere else; where the fused kernel runs, this layer's autograd node then owns that BatchNorm's backward
        (ops.propagate_linear)."""
        if self.gather_dtype is not None:
            return _finish_composed(self._forward_bf16(x, edge_index, edge_weight), post_affine, ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, None, None, edge_weight)
        weight, bias = self.lin.weight, self.bias
        if post_affine is not None:
            scale, shift = post_affine
            weight, bias = weight * scale[:, None], bias * scale + shift
        return self._conv(x, edge_index, weight, bias, want_colsums, edge_weight, next_bn)

    def eval_operands(self, bn=None):
        """(W'^T, b', None) of this layer for an eval forward, the eval-mode BatchNorm `bn` behind it folded in."""
        if self.gather_dtype is not None:
            return None
        return ops.fold_bn_linear(self.lin.weight, self.bias, bn=bn)

    # opt-in cache of the static input features' aggregate (models/_stack.ConvStack.cache_input_aggregate)
    def aggregate_input(self, x, edge_index, edge_weight=None):
        if (self.gather_dtype is not None or self.in_channels > self.out_channels
                or not ops.aggregate_linear_ok(self.in_channels, self.out_channels)):
            return None
        return _aggregate_input(x, edge_index, LOOPS_ADD_REMAINING, "gcn", edge_weight)

    def forward_from_aggregate(self, z, x, want_colsums=False, folded=None):
        if folded is not None:
            return _folded_from_aggregate(z, x, folded, False)
        return ops.aggregate_linear(z, self.lin.weight, self.bias, want_colsums=want_colsums)

    def forward_folded(self, x, edge_index, operands, ce=None, edge_weight=None):
        """Eval forward (no_grad) from prepared operands (eval_operands; models/_stack.ConvStack keeps them per
        parameter state): one fused launch. `ce` = (y, mask): returns (None, stats). None when this layer / graph does
        not take the fused kernel (the caller then runs the ordinary forward)."""
        if self.gather_dtype is not None:
            return None
        return _forward_folded(self, x, edge_index, operands, ce, LOOPS_ADD_REMAINING, "gcn", False, edge_weight)

    def _forward_bf16(self, x, edge_index, edge_weight=None):
        """gather_dtype=torch.bfloat16: A_hat gathers bfloat16 rows at the narrower width — A_hat bf16(x W^T) + b for
        in > out (the columns padded to a multiple of 8), (A_hat bf16(x)) W^T + b otherwise."""
        if edge_weight is not None and edge_weight.requires_grad:
            raise ValueError("GCNConv: gather_dtype and an edge_weight that requires grad exclude each other (the gradient "
                             "in the edge weights is taken over fp32 rows)")
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING, edge_weight)
        if self.in_channels > self.out_channels:
            weight, bias, n = ops.pad_rows8(self.lin.weight, self.bias)
            out = ops.propagate_rows_bf16(ops.linear(x, weight), graph, "gcn", bias=bias)
            return out if n == self.out_channels else out[:, :self.out_channels]
        return ops.linear(ops.propagate_bf16(x, graph, "gcn"), self.lin.weight, self.bias)

    @staticmethod
    def _learned(edge_weight):
        return edge_weight is not None and edge_weight.requires_grad and torch.is_grad_enabled()

    def _ce(self, x, edge_index, ce, bn, colsums, edge_weight=None):
        y, mask = ce
        if self._learned(edge_weight):  # the loss-in-kernel forms have no gradient in the edge weights
            if bn is not None:
                x = bn(x, colsums=colsums)
            return ops.ce_from_logits(self.forward(x, edge_index, edge_weight), y, mask)
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING, edge_weight)
        hand_over = bn is not None and bn.folds_into_next_layer(x)
        if ops.fused_ce_ok(graph, self.in_channels, self.out_channels, False, x, y) and (bn is None or hand_over):
            return ops.propagate_linear_ce(x, graph, "gcn", self.lin.weight, self.bias, None, y, mask, bn=bn,
                                           colsums=colsums)
        if bn is not None:
            x = bn(x, colsums=colsums)
        weight, bias, n = ops.pad_rows4(self.lin.weight, self.bias)
        if ops.rows_epilogue_ok(graph, n, x, y) and not ops.fused_linear_ok(graph, self.in_channels, self.out_channels, x=x):
            # transform first (the reference's shapes: hidden 64 -> C = 7, initial_params.py:25), then aggregate the
            # [N, 8] rows with the loss taken in the gather kernel: no logits, no log-softmax / NLL / arg-max passes
            return ops.propagate_rows_ce(ops.linear(x, weight), graph, "gcn", n, self.out_channels, y, mask, bias=bias)
        return ops.ce_from_logits(self.forward(x, edge_index, edge_weight), y, mask)

    def forward_after_bn(self, x, edge_index, bn, colsums=None, want_colsums=False, ce=None, edge_weight=None):
        """self(bn(x), edge_index) for the BatchNorm1d in front of this layer. In a training forward on one GPU the
        normalised matrix is not written: the fused kernel gathers the raw rows and applies BatchNorm's affine map to
        the aggregate (ops.bn_propagate_linear). `colsums`: the column sums of x if its producer took them."""
        if self.gather_dtype is not None:
            return self.forward(bn(x, colsums=colsums), edge_index, edge_weight, ce=ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, bn, colsums, edge_weight)
        if self._learned(edge_weight):
            return self.forward(bn(x, colsums=colsums), edge_index, edge_weight, want_colsums=want_colsums)
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING, edge_weight)
        if (bn.folds_into_next_layer(x) and not getattr(graph, "is_distributed", False)
                and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, x=x)):
            return ops.bn_propagate_linear(x, bn, graph, "gcn", self.lin.weight, self.bias, colsums=colsums,
                                           want_colsums=want_colsums)
        return self.forward(bn(x, colsums=colsums), edge_index, edge_weight, want_colsums=want_colsums)

    def _conv(self, x, edge_index, weight, bias, want_colsums=False, edge_weight=None, next_bn=None):
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING, edge_weight)
        if self._learned(edge_weight):
            # transform first, then the gather whose backward also differentiates the normalisation in the weights
            return ops.propagate_gcn_edge_weight(ops.linear(x, weight), edge_weight, graph, bias=bias)
        if ops.fused_linear_ok(graph, self.in_channels, self.out_channels, x=x):
            # A_hat (x W^T) + b = (A_hat x) W^T + b in one kernel: the aggregate stays in LDS and the GEMM
            # runs on the MFMA units underneath the gather (ops._PropagateLinear)
            return ops.propagate_linear(x, graph, "gcn", weight, bias, want_colsums=want_colsums, next_bn=next_bn)
        if not x.requires_grad and self.in_channels <= self.out_channels:
            # Input layer (and every layer under no_grad): A_hat (x W^T) = (A_hat x) W^T. Aggregating first
            # costs the same forward (in <= out) and makes dW = dy^T (A_hat x) a plain weight-gradient GEMM: no
            # gradient has to travel back through A_hat^T, because x needs none (one transposed SpMM less per
            # step). On a partitioned graph the aggregated tensor is then the static feature matrix, whose
            # boundary rows are resident (dist.DistGraph.pin_resident): no exchange either.
            return ops.linear(ops.propagate_gcn(x, graph), weight, bias)
        if want_colsums and ops.rows_epilogue_ok(graph, self.out_channels, x):
            # transform first; the BatchNorm behind the layer gets its column sums from the gather kernel
            return ops.propagate_rows(ops.linear(x, weight), graph, "gcn", bias=bias, want_colsums=True)
        return ops.propagate_gcn(ops.linear(x, weight), graph, bias=bias)


class SAGEConv(nn.Module):
    """out = lin_l(mean_{j in N(i)} x_j) + lin_r(x_i); no self-loops; nodes without in-edges
    aggregate 0 [PyG SAGEConv defaults: aggr='mean', root_weight=True, lin_l bias, lin_r no bias].

    ``aggr`` in {'mean', 'max', 'min', 'add', 'std', 'var'} ('sum' = 'add'): PyG's keyword. Other than 'mean' the layer runs
    in PyG's order on separate kernels — aggregate the raw x (ops.propagate_max / propagate_min / propagate_sum /
    propagate_std / propagate_var), then lin_l(agg) + lin_r(x) — and reports none of the fused forms (see _set_aggr).
    A list or tuple of k distinct names (PyG's MultiAggregation, mode='cat', e.g. ['mean', 'max', 'min', 'std']): the k
    aggregates come from ONE gather pass (ops.propagate_multi), concatenated, and lin_l takes k * in_channels columns."""

    folds_post_affine = True  # forward(..., post_affine=(scale, shift)): see models/_stack.py
    emits_colsums = True      # see GCNConv
    owns_next_bn_backward = True  # see GCNConv

    gather_dtype = None       # see GCNConv

    def __init__(self, in_channels, out_channels, aggr="mean", gather_dtype=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        k = _set_aggr(self, aggr, lists=True)
        _set_gather_dtype(self, gather_dtype)
        self.lin_l = nn.Linear(k * in_channels, out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)

    accepts_ce = True         # see GCNConv
    accepts_ce_pair = True

    def eval_operands(self, bn=None):
        if self.aggr != "mean" or self.gather_dtype is not None:
            return None
        return ops.fold_bn_linear(self.lin_l.weight, self.lin_l.bias, root_weight=self.lin_r.weight, bn=bn)

    def aggregate_input(self, x, edge_index):
        if (self.aggr != "mean" or self.gather_dtype is not None or self.in_channels > self.out_channels
                or not ops.aggregate_linear_ok(self.in_channels, self.out_channels, True)):
            return None
        return _aggregate_input(x, edge_index, LOOPS_KEEP, "mean")

    def _forward_composed(self, x, edge_index):
        """aggr != 'mean': PyG's order — the reduction over the raw rows, then both Linears."""
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        agg = _aggregate(x, graph, self.aggr)
        return ops.linear(agg, self.lin_l.weight, self.lin_l.bias) + ops.linear(x, self.lin_r.weight)

    def _forward_bf16(self, x, edge_index):
        """gather_dtype=torch.bfloat16: the mean gathers bfloat16 rows at the narrower width — for in > out one product
        x [W_l; W_r]^T whose left half is rounded and gathered, the root half (with lin_l's bias) being the fp32 addend;
        otherwise lin_l(mean bf16(x)) + lin_r(x)."""
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        w_l, b_l, w_r = self.lin_l.weight, self.lin_l.bias, self.lin_r.weight
        if self.in_channels > self.out_channels:
            h, n = self._transform_first(x, w_l, b_l, w_r, pad=ops.pad_rows8)
            out = ops.propagate_rows_bf16(h, graph, "mean", n=n)
            return out if n == self.out_channels else out[:, :self.out_channels]
        return ops.linear(ops.propagate_bf16(x, graph, "mean"), w_l, b_l) + ops.linear(x, w_r)

    def forward_from_aggregate(self, z, x, want_colsums=False, folded=None):
        if folded is not None:
            return _folded_from_aggregate(z, x, folded, True)
        return ops.aggregate_linear(z, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, x, want_colsums)

    def forward_folded(self, x, edge_index, operands, ce=None):
        """See GCNConv.forward_folded."""
        if self.aggr != "mean" or self.gather_dtype is not None:
            return None
        return _forward_folded(self, x, edge_index, operands, ce, LOOPS_KEEP, "mean", True)

    def _ce(self, x, edge_index, ce, bn, colsums):
        y, mask = ce
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        hand_over = bn is not None and bn.folds_into_next_layer(x)
        if ops.fused_ce_ok(graph, self.in_channels, self.out_channels, True, x, y) and (bn is None or hand_over):
            return ops.propagate_linear_ce(x, graph, "mean", self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, y,
                                           mask, bn=bn, colsums=colsums)
        if bn is not None:
            x = bn(x, colsums=colsums)
        if (ops.rows_epilogue_ok(graph, (self.out_channels + 3) // 4 * 4, x, y)
                and not ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x)):
            h, n = self._transform_first(x, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight)
            return ops.propagate_rows_ce(h, graph, "mean", n, self.out_channels, y, mask)
        return ops.ce_from_logits(self.forward(x, edge_index), y, mask)

    @staticmethod
    def _transform_first(x, w_l, b_l, w_r, pad=ops.pad_rows4):
        """h = x [W_l; W_r]^T + [0; b_l] as ONE product ([N, 2 n], n = out rounded up to a multiple of 4): the left half is
        what the mean runs over, the right half the root term plus lin_l's bias (which PyG adds after the aggregation:
        a node without in-edges gets b_l + W_r x_i). The wide input (F = 1433 on Cora) is read once for both Linears."""
        w_l, b_l, n = pad(w_l, b_l)
        w_r = pad(w_r)[0]
        return ops.linear(x, torch.cat([w_l, w_r]), torch.cat([torch.zeros_like(b_l), b_l])), n

    def forward_after_bn(self, x, edge_index, bn, colsums=None, want_colsums=False, ce=None):
        """See GCNConv.forward_after_bn; the root term lin_r(bn(x)_i) gets the affine map as its rows are loaded."""
        if self.gather_dtype is not None:
            return self.forward(bn(x, colsums=colsums), edge_index, ce=ce)
        if self.aggr != "mean":
            return _finish_composed(self._forward_composed(bn(x, colsums=colsums), edge_index), None, ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, bn, colsums)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        if (bn.folds_into_next_layer(x) and not getattr(graph, "is_distributed", False)
                and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x)):
            return ops.bn_propagate_linear(x, bn, graph, "mean", self.lin_l.weight, self.lin_l.bias,
                                           root_weight=self.lin_r.weight, colsums=colsums, want_colsums=want_colsums)
        return self.forward(bn(x, colsums=colsums), edge_index, want_colsums=want_colsums)

    def forward(self, x, edge_index, post_affine=None, want_colsums=False, ce=None, next_bn=None):
        if self.gather_dtype is not None:
            return _finish_composed(self._forward_bf16(x, edge_index), post_affine, ce)
        if self.aggr != "mean":
            return _finish_composed(self._forward_composed(x, edge_index), post_affine, ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, None, None)
        w_l, b_l, w_r = self.lin_l.weight, self.lin_l.bias, self.lin_r.weight
        if post_affine is not None:  # see GCNConv.forward
            scale, shift = post_affine
            w_l, b_l, w_r = w_l * scale[:, None], b_l * scale + shift, w_r * scale[:, None]
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        if ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x):
            # lin_l(mean_j x_j) + lin_r(x_i) in one kernel: both products accumulate in the same MFMA tile
            return ops.propagate_linear(x, graph, "mean", w_l, b_l, root_weight=w_r, want_colsums=want_colsums,
                                        next_bn=next_bn)
        if self.in_channels > self.out_channels and x.is_cuda and not getattr(graph, "is_distributed", False):
            # in > out (the reference's defaults: F -> 64 -> C; graphsage2 at F = 1433 is the row its README marks OOM,
            # README.md:74): mean_j(x_j) W_l^T = mean_j(x_j W_l^T) — transform first, gather at the OUTPUT width
            h, n = self._transform_first(x, w_l, b_l, w_r)
            out = ops.propagate_rows(h, graph, "mean", n=n, want_colsums=want_colsums and n == self.out_channels)
            return out if n == self.out_channels else out[:, :self.out_channels]
        x_r = ops.linear(ops.target_rows(x, graph), w_r)  # the targets' own rows (all of x except on a dist.ReplicaGraph)
        if ops.fused_linear_ok(graph, self.in_channels, self.out_channels, x=x):
            return ops.propagate_linear(x, graph, "mean", w_l, b_l) + x_r
        if self.in_channels > self.out_channels:
            return ops.propagate_mean(ops.linear(x, w_l), graph) + b_l + x_r
        agg = ops.propagate_mean(x, graph)
        return ops.linear(agg, w_l, b_l) + x_r


class MySAGEConv(nn.Module):
    """reference models/graphsage.py:36-62: x_l = lin_l(x), x_r = lin_r(x) (both with bias),
    remove_self_loops + add_self_loops, mean over N(i) ∪ {i} of x_l, then += x_r.

    ``aggr`` in {'mean', 'max', 'min', 'add', 'std', 'var'} ('sum' = 'add'): the keyword the reference leaves to the caller
    (graphsage.py:38-40). Other than 'mean' the layer runs in the reference's order on separate kernels — [lin_l(x),
    lin_r(x)] in one product, the reduction over the left half (ops.propagate_max / propagate_min / propagate_sum /
    propagate_std / propagate_var), += x_r — and reports none of the fused forms (see _set_aggr). A list of aggregators
    is refused: the reference's layer has no projection for their concatenation."""

    folds_post_affine = True  # forward(..., post_affine=(scale, shift)): see models/_stack.py
    emits_colsums = True      # see GCNConv
    owns_next_bn_backward = True  # see GCNConv

    gather_dtype = None       # see GCNConv

    def __init__(self, in_channels, out_channels, add_self_loops=True, aggr="mean", gather_dtype=None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.add_self_loops = add_self_loops
        _set_aggr(self, aggr)
        _set_gather_dtype(self, gather_dtype)
        self.lin_l = nn.Linear(in_channels, out_channels)
        self.lin_r = nn.Linear(in_channels, out_channels)

    accepts_ce = True         # see GCNConv
    accepts_ce_pair = True

    def _forward_composed(self, x, edge_index):
        """aggr != 'mean': the reference's order (graphsage.py:49-60) — transform, reduce x_l over N(i) (and i itself
        with add_self_loops), += x_r."""
        graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD if self.add_self_loops else LOOPS_KEEP)
        h, n = self._transform_both(x, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, self.lin_r.bias)
        out = _aggregate(h[:, :n], graph, self.aggr) + h[:, n:]
        return out if n == self.out_channels else out[:, :self.out_channels]

    def _forward_bf16(self, x, edge_index):
        """gather_dtype=torch.bfloat16: the mean gathers bfloat16 rows at the narrower width — [lin_l(x), lin_r(x)] in one
        product, the left half rounded and gathered, the right half the fp32 addend, for in > out; lin_l(mean bf16(x)) +
        lin_r(x) otherwise (with the self-loop a row's mean weights sum to 1, so b_l passes through the mean; without
        add_self_loops the layer always transforms first: a row without entries must get no b_l)."""
        graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD if self.add_self_loops else LOOPS_KEEP)
        w_l, b_l, w_r, b_r = self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, self.lin_r.bias
        if self.in_channels > self.out_channels or not self.add_self_loops:
            h, n = self._transform_both(x, w_l, b_l, w_r, b_r, pad=ops.pad_rows8)
            out = ops.propagate_rows_bf16(h, graph, "mean", n=n)
            return out if n == self.out_channels else out[:, :self.out_channels]
        return ops.linear(ops.propagate_bf16(x, graph, "mean"), w_l, b_l) + ops.linear(x, w_r, b_r)

    def eval_operands(self, bn=None):
        if not self.add_self_loops or self.aggr != "mean" or self.gather_dtype is not None:
            return None
        return ops.fold_bn_linear(self.lin_l.weight, self.lin_l.bias, self.lin_r.bias, root_weight=self.lin_r.weight,
                                  bn=bn)

    def aggregate_input(self, x, edge_index):
        if (not self.add_self_loops or self.aggr != "mean" or self.gather_dtype is not None
                or self.in_channels > self.out_channels or not ops.aggregate_linear_ok(self.in_channels, self.out_channels, True)):
            return None
        return _aggregate_input(x, edge_index, LOOPS_REMOVE_ADD, "mean")

    def forward_from_aggregate(self, z, x, want_colsums=False, folded=None):
        if folded is not None:
            return _folded_from_aggregate(z, x, folded, True)
        return ops.aggregate_linear(z, self.lin_l.weight, self.lin_l.bias + self.lin_r.bias, self.lin_r.weight, x,
                                    want_colsums)

    def forward_folded(self, x, edge_index, operands, ce=None):
        """See GCNConv.forward_folded (mean over N(i) + {i}: the weights of a row sum to 1, so both biases and the
        BatchNorm shift ride in the kernel's bias)."""
        if self.aggr != "mean" or self.gather_dtype is not None:
            return None
        return _forward_folded(self, x, edge_index, operands, ce, LOOPS_REMOVE_ADD, "mean", True)

    def _ce(self, x, edge_index, ce, bn, colsums):
        y, mask = ce
        if self.add_self_loops:
            graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD)
            hand_over = bn is not None and bn.folds_into_next_layer(x)
            if ops.fused_ce_ok(graph, self.in_channels, self.out_channels, True, x, y) and (bn is None or hand_over):
                return ops.propagate_linear_ce(x, graph, "mean", self.lin_l.weight, self.lin_l.bias + self.lin_r.bias,
                                               self.lin_r.weight, y, mask, bn=bn, colsums=colsums)
        if bn is not None:
            x = bn(x, colsums=colsums)
        mode = LOOPS_REMOVE_ADD if self.add_self_loops else LOOPS_KEEP
        graph = get_graph(edge_index, x.size(0), mode)
        fused = self.add_self_loops and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x)
        if ops.rows_epilogue_ok(graph, (self.out_channels + 3) // 4 * 4, x, y) and not fused:
            h, n = self._transform_both(x, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, self.lin_r.bias)
            return ops.propagate_rows_ce(h, graph, "mean", n, self.out_channels, y, mask)
        return ops.ce_from_logits(self.forward(x, edge_index), y, mask)

    @staticmethod
    def _transform_both(x, w_l, b_l, w_r, b_r, pad=ops.pad_rows4):
        """h = [lin_l(x), lin_r(x)] as ONE product (models/graphsage.py:49-50 runs two Linears over the same x): [N, 2 n],
        n = out rounded up to a multiple of 4. b_l stays inside the mean, as in the reference (a row without entries —
        add_self_loops=False and no in-edge — gets no b_l)."""
        w_l, b_l, n = pad(w_l, b_l)
        w_r, b_r, _ = pad(w_r, b_r)
        return ops.linear(x, torch.cat([w_l, w_r]), torch.cat([b_l, b_r])), n

    def forward_after_bn(self, x, edge_index, bn, colsums=None, want_colsums=False, ce=None):
        """See GCNConv.forward_after_bn."""
        if self.gather_dtype is not None:
            return self.forward(bn(x, colsums=colsums), edge_index, ce=ce)
        if self.aggr != "mean":
            return _finish_composed(self._forward_composed(bn(x, colsums=colsums), edge_index), None, ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, bn, colsums)
        if self.add_self_loops:
            graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD)
            if (bn.folds_into_next_layer(x) and not getattr(graph, "is_distributed", False)
                    and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x)):
                return ops.bn_propagate_linear(x, bn, graph, "mean", self.lin_l.weight,
                                               self.lin_l.bias + self.lin_r.bias, root_weight=self.lin_r.weight,
                                               colsums=colsums, want_colsums=want_colsums)
        return self.forward(bn(x, colsums=colsums), edge_index, want_colsums=want_colsums)

    def forward(self, x, edge_index, post_affine=None, want_colsums=False, ce=None, next_bn=None):
        if self.gather_dtype is not None:
            return _finish_composed(self._forward_bf16(x, edge_index), post_affine, ce)
        if self.aggr != "mean":
            return _finish_composed(self._forward_composed(x, edge_index), post_affine, ce)
        if ce is not None:
            return self._ce(x, edge_index, ce, None, None)
        w_l, b_l, w_r, b_r = self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, self.lin_r.bias
        if post_affine is not None and self.add_self_loops:  # see GCNConv.forward; the mean weights sum to 1
            scale, shift = post_affine
            w_l, b_l = w_l * scale[:, None], b_l * scale
            w_r, b_r = w_r * scale[:, None], b_r * scale + shift
        out = self._conv(x, edge_index, w_l, b_l, w_r, b_r, want_colsums, next_bn)
        if post_affine is not None and not self.add_self_loops:
            out = out * post_affine[0] + post_affine[1]
        return out

    def _conv(self, x, edge_index, w_l, b_l, w_r, b_r, want_colsums=False, next_bn=None):
        mode = LOOPS_REMOVE_ADD if self.add_self_loops else LOOPS_KEEP
        graph = get_graph(edge_index, x.size(0), mode)
        if self.add_self_loops and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, root=True, x=x):
            # mean_j(lin_l(x_j)) + lin_r(x_i) = (mean_j x_j) Wl^T + x_i Wr^T + (b_l + b_r), one kernel
            return ops.propagate_linear(x, graph, "mean", w_l, b_l + b_r, root_weight=w_r, want_colsums=want_colsums,
                                        next_bn=next_bn)
        fused_left = self.add_self_loops and ops.fused_linear_ok(graph, self.in_channels, self.out_channels, x=x)
        input_layer = not x.requires_grad and self.add_self_loops and self.in_channels <= self.out_channels
        if x.is_cuda and not getattr(graph, "is_distributed", False) and not fused_left and not input_layer:
            # transform first, as the reference writes the layer (in > out is its default shape: F -> 64 -> C)
            return self._conv_rows(x, graph, w_l, b_l, w_r, b_r, want_colsums)
        x_r = ops.linear(ops.target_rows(x, graph), w_r, b_r)
        if fused_left:
            return ops.propagate_linear(x, graph, "mean", w_l, b_l) + x_r
        if input_layer:
            # Input layer (see GCNConv.forward): with the self-loop every row's mean weights
            # sum to 1, so mean_j(W x_j + b) = W mean_j(x_j) + b exactly; aggregating first removes the
            # transposed SpMM from this layer's backward.
            return ops.linear(ops.propagate_mean(x, graph), w_l, b_l) + x_r
        x_l = ops.linear(x, w_l, b_l)
        return ops.propagate_mean(x_l, graph) + x_r

    def _conv_rows(self, x, graph, w_l, b_l, w_r, b_r, want_colsums):
        """The layer as the reference writes it — transform, then the mean, then += x_r (graphsage.py:49-60) — on one
        product and one gather: the add is the gather kernel's additive operand."""
        h, n = self._transform_both(x, w_l, b_l, w_r, b_r)
        out = ops.propagate_rows(h, graph, "mean", n=n, want_colsums=want_colsums and n == self.out_channels)
        return out if n == self.out_channels else out[:, :self.out_channels]


class GATConv(nn.Module):
    """h = x W^T viewed [N,H,C]; e_ij = LeakyReLU(<h_j,att_src> + <h_i,att_dst>, 0.2); softmax over
    the in-edges of i (self-loops removed then re-added); out_i = sum_j alpha_ij h_j; heads
    concatenated (or averaged when concat=False); + bias [PyG GATConv defaults; dropout 0 as the
    reference never sets it, models/gat.py:18-21]."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.heads, self.concat, self.negative_slope = heads, concat, negative_slope
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src  # shared, as PyG does for a single feature matrix
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.lin_src.weight)
        glorot_(self.att_src)
        glorot_(self.att_dst)
        nn.init.zeros_(self.bias)

    folds_post_affine = True  # forward(..., post_affine=(scale, shift)): see models/_stack.py
    accepts_ce = True  # forward(..., ce=(y, mask)) returns (loss, stats): see models/_stack.py

    @staticmethod
    def kernel_channels(C):
        """Channels per head the attention kernels run with. A wave holds one head's channels on at most 64 lanes of
        4 / 2 / 1 floats (csrc/gat.hip make_layout: C % 4 == 0 up to 256, C % 2 == 0 up to 128, any C up to 64); other
        widths — 130 classes on the single-head output layer, an odd 67 — are padded per head to the next multiple of 4
        with zero weight rows, zero attention entries and zero bias, which changes neither a score nor a kept column
        (PyG's GATConv has no such bound)."""
        if C <= 64 or (C % 2 == 0 and C <= 128) or (C % 4 == 0 and C <= 256):
            return C
        Cp = (C + 3) // 4 * 4
        if Cp > 256:
            raise NotImplementedError(f"GATConv: {C} channels per head; the attention kernels take at most 256")
        return Cp

    def forward(self, x, edge_index, post_affine=None, ce=None):
        """`post_affine` = (scale, shift) of an eval-mode BatchNorm that follows this layer (no_grad only): applied in
        the aggregation kernel's store, out = aggregate * scale + (bias * scale + shift), when the bias rides there
        too; otherwise after the layer. `ce` = (y, mask): the layer is the model's last; returns (loss, stats) of the
        masked cross-entropy of its output instead of the output."""
        H, C = self.heads, self.out_channels
        Cp = self.kernel_channels(C)
        if Cp == C:
            return self._forward(x, edge_index, self.lin_src.weight, self.att_src, self.att_dst, self.bias, C, post_affine, ce)
        pad = torch.nn.functional.pad
        in_kernel = self.concat or H == 1
        weight = pad(self.lin_src.weight.view(H, C, -1), (0, 0, 0, Cp - C)).reshape(H * Cp, -1)
        bias = pad(self.bias.view(H, C), (0, Cp - C)).reshape(-1) if in_kernel else pad(self.bias, (0, Cp - C))
        out = self._forward(x, edge_index, weight, pad(self.att_src, (0, Cp - C)), pad(self.att_dst, (0, Cp - C)), bias, Cp,
                            None, None)
        out = out.view(-1, H, Cp)[:, :, :C].reshape(-1, H * C) if (self.concat and H > 1) else out[:, :C]
        if post_affine is not None:
            out = out * post_affine[0] + post_affine[1]
        return out if ce is None else ops.ce_from_logits(out, ce[0], ce[1])

    def _forward(self, x, edge_index, weight, att_src, att_dst, bias, C, post_affine, ce):
        H = self.heads
        graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD)
        if (H == 1 and post_affine is None
                and ops.gat_linear_ok(graph, self.in_channels, C, x, None if ce is None else ce[0])):
            # one head: sum_j alpha_ij (W x_j) = W sum_j alpha_ij x_j — scores from x, the coefficients as a per-edge
            # vector, then aggregation + transform (+ loss) in ONE launch of the fused kernel; no h = x W^T product
            return ops.gat_attend_linear(x, weight, att_src, att_dst, graph, self.negative_slope, bias=bias, ce=ce)
        if ce is not None:
            return ops.ce_from_logits(self._forward(x, edge_index, weight, att_src, att_dst, bias, C, post_affine, None),
                                      ce[0], ce[1])
        # the bias rides in the aggregation kernel's store when it applies to the stored row as is
        # (concatenated heads, or a single head, whose "mean over heads" is the identity)
        in_kernel = self.concat or H == 1
        dist_resident = getattr(graph, "is_distributed", False) and graph.is_resident(x)
        if dist_resident:
            out = graph.gat(x, att_src, att_dst, H, C, self.negative_slope, weight=weight)
            out = out + bias if in_kernel else out.view(-1, H, C).mean(dim=1) + bias
        else:
            h = ops.linear(x, weight)
            if in_kernel and post_affine is not None and not getattr(graph, "is_distributed", False):
                scale, shift = post_affine
                return ops.gat_attend(h, att_src, att_dst, graph, H, C, self.negative_slope,
                                      bias=bias * scale + shift, out_scale=scale)
            out = ops.gat_attend(h, att_src, att_dst, graph, H, C, self.negative_slope,
                                 bias=bias if in_kernel else None)
            if not in_kernel:
                out = out.view(-1, H, C).mean(dim=1) + bias
        if post_affine is not None:
            out = out * post_affine[0] + post_affine[1]
        return out


class APPNP(nn.Module):
    """z^0 = x; z^{k+1} = (1-alpha) A_hat z^k + alpha x, K times (in-repo twin of the recurrence:
    reference models/pta.py:79-84); gcn_norm computed once per graph. `edge_weight` (float32 [E], constant: a weight that
    requires grad raises ValueError) enters gcn_norm as in GCNConv."""

    def __init__(self, K, alpha):
        super().__init__()
        self.K, self.alpha = K, alpha

    def forward(self, x, edge_index, edge_weight=None):
        _no_weight_grad(edge_weight, "APPNP")
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING, edge_weight)
        return ops.appnp_propagate(x, graph, self.K, self.alpha)


class SGConv(nn.Module):
    """x' = lin(A_hat^K x) with gcn_norm (self-loops added unless add_self_loops=False) and the
    propagated features cached after the first call when cached=True [PyG SGConv, as built at reference
    models/sgc.py:9-10]. The K propagates run as one rgbx_appnp_f32 call with alpha = 0. `edge_weight` (float32 [E],
    constant: a weight that requires grad raises ValueError) enters gcn_norm as in GCNConv; with cached=True the kept
    propagate is that of the FIRST call's weights, as in PyG — later calls ignore their edge_weight."""

    def __init__(self, in_channels, out_channels, K=1, cached=False, add_self_loops=True, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.cached, self.add_self_loops = cached, add_self_loops
        self.lin = nn.Linear(in_channels, out_channels, bias=bias)
        self._cached_x = None

    def forward(self, x, edge_index, edge_weight=None):
        _no_weight_grad(edge_weight, "SGConv")
        h = self._cached_x
        if h is None:
            mode = LOOPS_ADD_REMAINING if self.add_self_loops else LOOPS_KEEP
            graph = get_graph(edge_index, x.size(0), mode, edge_weight)
            if not self.cached and self.in_channels > self.out_channels:
                # nothing is kept between calls, so A_hat^K (x W^T) = (A_hat^K x) W^T runs the K gathers at the
                # OUTPUT width (F = 1433 -> C = 7 on Cora: 1/180 of the bytes)
                out = ops.appnp_propagate(ops.linear(x, self.lin.weight), graph, self.K, 0.0)
                return out if self.lin.bias is None else out + self.lin.bias
            h = ops.appnp_propagate(x, graph, self.K, 0.0)
            if self.cached:
                self._cached_x = h if h.requires_grad else h.detach()
        return ops.linear(h, self.lin.weight, self.lin.bias)


class GINConv(nn.Module):
    """out = nn((1 + eps) * x_i + sum_{j in N(i)} x_j), edges as given, eps learnable when train_eps
    [PyG GINConv, as built at reference models/gin.py:14-34]."""

    def __init__(self, nn_module, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = nn_module
        self.initial_eps = eps
        if train_eps:
            self.eps = nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))

    def forward(self, x, edge_index):
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        first = self.nn[0] if isinstance(self.nn, nn.Sequential) and len(self.nn) else None
        if (isinstance(first, nn.Linear) and x.is_cuda
                and ops.fused_linear_ok(graph, first.in_features, first.out_features, root=True, x=x)):
            # nn's first Linear applied to (sum_j x_j + (1 + eps) x_i) = (sum_j x_j) W^T + x_i ((1 + eps) W)^T + b:
            # aggregation, the root term and that Linear in one launch (rgbx_spmm_linear_f32), no [N, in] sum
            # written, no scale / add passes; eps gets its gradient through the root operand
            h = ops.propagate_linear(x, graph, "sum", first.weight, first.bias,
                                     root_weight=(1 + self.eps) * first.weight)
            for layer in list(self.nn)[1:]:
                h = layer(h)
            return h
        if isinstance(first, nn.Linear) and first.in_features > first.out_features:
            # (sum_j x_j + (1 + eps) x_i) W^T + b = sum_j (x_j W^T) + (1 + eps) (x_i W^T) + b: transform first, gather at
            # the output width of nn's first Linear (in > out: the reference's first block, F -> 64, models/gin.py:14-21)
            h = ops.linear(x, first.weight)
            h = ops.propagate_sum(h, graph) + (1 + self.eps) * h
            if first.bias is not None:
                h = h + first.bias
            for layer in list(self.nn)[1:]:
                h = layer(h)
            return h
        return self.nn(ops.propagate_sum(x, graph) + (1 + self.eps) * x)


class GINEConv(nn.Module):
    """GIN with edge features [PyG GINEConv; Hu et al., "Strategies for Pre-training Graph Neural Networks"; the layer
    of the OGB baselines]: out = nn((1 + eps) * x_i + sum_{j -> i} relu(x_j + e_ji)), the edges AS GIVEN (self-loops
    stay, duplicates count twice, a node without in-edges aggregates zeros, so nn sees (1 + eps) x_i). `edge_attr`
    [E, D] holds one row per input edge. With edge_dim=D, e = lin(edge_attr), lin = Linear(D, in_channels) with bias and
    in_channels read from the first Linear of `nn_module`; with edge_dim=None edge_attr must already be in_channels
    wide (ValueError before any launch otherwise). eps is a Parameter with train_eps, a buffer otherwise, as in GINConv.
    Parameter names are PyG's (nn.*, eps, lin.*).

    The attribute rows are permuted into CSR slot order once, at their raw width (ops.edge_rows_to_slots), so lin yields
    the per-slot rows directly and dW_lin comes out of the Linear's own backward; message, sum and root term run in the
    rgbx_gine_* kernels (ops.gine_aggregate), which read eps on the device. A width outside the kernels' set is
    zero-padded in x and in lin's rows (a padded channel contributes relu(0 + 0) = 0) and sliced off again.

    Out of scope: the node-partitioned (distributed) route, edge attributes through to_undirected / coalesce."""

    def __init__(self, nn_module, eps=0.0, train_eps=False, edge_dim=None):
        super().__init__()
        self.nn = nn_module
        self.initial_eps = eps
        if train_eps:
            self.eps = nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))
        first = next((m for m in nn_module.modules() if isinstance(m, nn.Linear)), None)
        self.in_channels = None if first is None else first.in_features
        self.edge_dim = edge_dim
        if edge_dim is not None:
            if self.in_channels is None:
                raise ValueError("GINEConv: edge_dim needs the input width, read from the first Linear of nn; it has none")
            self.lin = Linear(edge_dim, self.in_channels)
        else:
            self.lin = None

    @staticmethod
    def kernel_channels(C):
        """The width the aggregation runs at: C where the kernels take it (their set up to 256, and column blocks of
        256 above it whose last block is in the set), else the next multiple of 4."""
        last = C if C <= ops.GINE_BLOCK else (C % ops.GINE_BLOCK or ops.GINE_BLOCK)
        return C if GATConv.kernel_channels(last) == last else (C + 3) // 4 * 4

    def forward(self, x, edge_index, edge_attr):
        C = x.size(1)
        want = C if self.lin is None else self.edge_dim
        if not torch.is_tensor(edge_attr) or edge_attr.dim() != 2 or edge_attr.size(1) != want \
                or edge_attr.size(0) != edge_index.size(1) or not edge_attr.is_floating_point():
            got = tuple(edge_attr.shape) if torch.is_tensor(edge_attr) else type(edge_attr).__name__
            raise ValueError(f"GINEConv: edge_attr must be float [E, {want}] = [{edge_index.size(1)}, {want}] "
                             f"({'edge_dim' if self.lin is not None else 'the node width: edge_dim=None'}), got {got}")
        if self.in_channels is not None and C != self.in_channels:
            raise ValueError(f"GINEConv: x has {C} channels, nn's first Linear takes {self.in_channels}")
        _lib.require_device(x, edge_attr)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        ea = ops.edge_rows_to_slots(edge_attr.to(torch.float32), graph)
        Cp = self.kernel_channels(C)
        pad = torch.nn.functional.pad
        if edge_index.size(1) == 0:  # no slot, no product
            e = x.new_zeros((0, Cp))
        elif self.lin is not None:
            w, b = self.lin.weight, self.lin.bias
            e = ops.linear(ea, w, b) if Cp == C else ops.linear(ea, pad(w, (0, 0, 0, Cp - C)), pad(b, (0, Cp - C)))
        else:
            e = ea if Cp == C else pad(ea, (0, Cp - C))
        out = ops.gine_aggregate(x if Cp == C else pad(x, (0, Cp - C)), e, graph, self.eps)
        return self.nn(out if Cp == C else out[:, :C])


_PNA_ACTS = {"relu": nn.ReLU, "elu": nn.ELU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "leaky_relu": nn.LeakyReLU,
             "gelu": nn.GELU, "silu": nn.SiLU}


class PNAConv(nn.Module):
    """Principal Neighbourhood Aggregation [PyG PNAConv; Corso et al., "Principal Neighbourhood Aggregation for Graph
    Nets"]: per tower t (T towers, F_in = in_channels, or in_channels / T with divide_input; F_out = out_channels / T)
        m_ji = pre_nns[t](cat[x_i, x_j, edge_encoder(e_ji)])             (one Linear: pre_layers = 1)
        agg_i = cat over the scalers s, then the aggregators k, of scale_s(deg_i) * AGG_k over the in-edges of m_ji
        out_i = lin(cat over t of post_nns[t](cat[x_i, agg_i]))
    over the edges AS GIVEN (self-loops stay, duplicates count twice, a node without in-edges aggregates zeros).
    Aggregators: sum / add, mean, var, std, max, min; scalers: identity, amplification, attenuation, linear,
    inverse_linear, with deg = max(in-degree, 1) and the averages of PyG's `deg` histogram (`deg=None`, an addition:
    the averages of the first graph the layer sees). Parameter names and shapes are PyG's (pre_nns.{t}.0.*,
    post_nns.{t}.*, edge_encoder.*, lin.*); the averages live in a non-persistent buffer.

    pre_nns[t] is linear, so the message splits into a target part a_i = W_i x_i + bias, a source part b_j = W_j x_j and
    an edge part c_ji = W_e edge_encoder(e_ji): one GEMM makes a | b for all towers, one GEMM at the RAW edge width makes c
    (the encoder folded into W_e, bias included), and ops.pna_aggregate reads every b and c row once and writes the
    T * S * A blocks in the order post_nns read them. F_in % 4 != 0 runs zero-padded (the padded channels aggregate
    zeros and meet zero columns of post_nns' first weight).

    Refused (NotImplementedError): pre_layers != 1 (a non-linear network per edge), train_norm=True, unknown aggregator
    or scaler names. Out of scope: the node-partitioned (distributed) route, towers wider than 256 channels."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg=None, edge_dim=None, towers=1, pre_layers=1,
                 post_layers=1, divide_input=False, act="relu", train_norm=False):
        super().__init__()
        if pre_layers != 1:
            raise NotImplementedError("PNAConv: pre_layers != 1 puts a non-linear network on every edge; only the "
                                      "single Linear (pre_layers=1) is implemented")
        if train_norm:
            raise NotImplementedError("PNAConv: train_norm=True (trained degree averages) is not implemented")
        try:
            self.aggregators = ops.multi_names(list(aggregators))
            self.scalers = ops.pna_scaler_names(list(scalers))
        except ValueError as err:
            raise NotImplementedError(f"PNAConv: {err}") from None
        if act not in _PNA_ACTS:
            raise NotImplementedError(f"PNAConv: act={act!r} (one of {sorted(_PNA_ACTS)})")
        if towers < 1 or post_layers < 1 or out_channels % towers or (divide_input and in_channels % towers):
            raise ValueError("PNAConv: towers must divide out_channels (and in_channels with divide_input); post_layers "
                             "must be at least 1")
        self.in_channels, self.out_channels, self.edge_dim = in_channels, out_channels, edge_dim
        self.towers, self.divide_input = towers, divide_input
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        if edge_dim is not None:
            self.edge_encoder = Linear(edge_dim, self.F_in)
        self.pre_nns, self.post_nns = nn.ModuleList(), nn.ModuleList()
        wide = (len(self.aggregators) * len(self.scalers) + 1) * self.F_in
        for _ in range(towers):
            self.pre_nns.append(nn.Sequential(Linear((3 if edge_dim is not None else 2) * self.F_in, self.F_in)))
            post = [Linear(wide, self.F_out)]
            for _ in range(post_layers - 1):
                post += [_PNA_ACTS[act](), Linear(self.F_out, self.F_out)]
            self.post_nns.append(nn.Sequential(*post))
        self.lin = Linear(out_channels, out_channels)
        avg = torch.zeros(2)
        if deg is not None:  # PyG's histogram: deg[k] = the number of nodes with in-degree k
            hist = torch.as_tensor(deg).detach().to("cpu", torch.float64).reshape(-1)
            bins = torch.arange(hist.numel(), dtype=torch.float64)
            avg = torch.stack([(bins * hist).sum(), ((bins + 1).log() * hist).sum()]) / hist.sum()
        self.register_buffer("avg_deg", avg.to(torch.float32), persistent=False)
        self._avg_known = deg is not None

    def _node_operands(self):
        """(weight [2 T Fp, in_channels], bias [2 T Fp]) of the GEMM that makes a | b for all towers: the x_i and x_j column
        blocks of every pre_nns[t] weight, rows padded to Fp, block-diagonal over the towers with divide_input."""
        Fi, pad = self.F_in, (self.F_in + 3) // 4 * 4 - self.F_in
        rows = lambda w: torch.nn.functional.pad(w, (0, 0, 0, pad)) if pad else w
        wi = [rows(p[0].weight[:, :Fi]) for p in self.pre_nns]
        wj = [rows(p[0].weight[:, Fi:2 * Fi]) for p in self.pre_nns]
        stack = (lambda ws: torch.block_diag(*ws)) if self.divide_input else (lambda ws: torch.cat(ws, 0))
        bias = torch.cat([torch.nn.functional.pad(p[0].bias, (0, pad)) for p in self.pre_nns])
        return torch.cat([stack(wi), stack(wj)], 0), torch.cat([bias, torch.zeros_like(bias)])

    def _edge_operands(self):
        """(weight [T Fp, edge_dim], bias [T Fp]): the edge encoder folded into the edge block of every pre_nns[t]."""
        Fi, pad = self.F_in, (self.F_in + 3) // 4 * 4 - self.F_in
        enc = self.edge_encoder
        ws, bs = [], []
        for p in self.pre_nns:
            we = p[0].weight[:, 2 * Fi:]
            ws.append(torch.nn.functional.pad(we @ enc.weight, (0, 0, 0, pad)))
            bs.append(torch.nn.functional.pad(we @ enc.bias, (0, pad)))
        return torch.cat(ws, 0), torch.cat(bs)

    def forward(self, x, edge_index, edge_attr=None):
        E = edge_index.size(1)
        if self.edge_dim is not None:
            if not torch.is_tensor(edge_attr) or edge_attr.dim() != 2 or tuple(edge_attr.shape) != (E, self.edge_dim) \
                    or not edge_attr.is_floating_point():
                got = tuple(edge_attr.shape) if torch.is_tensor(edge_attr) else type(edge_attr).__name__
                raise ValueError(f"PNAConv: edge_attr must be float [E, edge_dim] = [{E}, {self.edge_dim}], got {got}")
        elif edge_attr is not None:
            raise ValueError("PNAConv: edge_attr given to a layer built with edge_dim=None")
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"PNAConv: x {tuple(x.shape)} for in_channels={self.in_channels}")
        _lib.require_device(x, edge_attr)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        if not self._avg_known:  # the averages of the first graph seen, copied on the device
            with torch.no_grad():
                self.avg_deg.copy_(ops.degree_averages(graph))
            self._avg_known = True
        T, Fi = self.towers, self.F_in
        Fp = (Fi + 3) // 4 * 4
        d = T * Fp
        ab = ops.linear(x, *self._node_operands())
        c = None
        if self.edge_dim is not None and E > 0:
            ea = ops.edge_rows_to_slots(edge_attr.to(torch.float32), graph)
            c = ops.linear(ea, *self._edge_operands())
        out = ops.pna_aggregate(ab[:, :d], ab[:, d:], c, graph, self.aggregators, self.scalers, self.avg_deg, Fp)
        blocks = len(self.aggregators) * len(self.scalers)
        outs = []
        for t, post in enumerate(self.post_nns):  # post_nns[t] on cat[x_t, out_t], read in place
            first = post[0]
            wx, wo = first.weight[:, :Fi], first.weight[:, Fi:]
            if Fp != Fi:
                wo = torch.nn.functional.pad(wo.reshape(-1, blocks, Fi), (0, Fp - Fi)).reshape(-1, blocks * Fp)
            x_t = x[:, t * Fi:(t + 1) * Fi] if self.divide_input else x
            h = ops.linear(out[:, t * blocks * Fp:(t + 1) * blocks * Fp], wo.contiguous()) \
                + ops.linear(x_t, wx.contiguous(), first.bias)
            for layer in list(post)[1:]:
                h = layer(h)
            outs.append(h)
        return self.lin(outs[0] if T == 1 else torch.cat(outs, dim=1))


class RGCNConv(nn.Module):
    """Relational graph convolution [PyG RGCNConv; Schlichtkrull et al., "Modeling Relational Data with Graph
    Convolutional Networks"]: every edge carries a relation, edge_type[e] in [0, num_relations), and
        out_i = x_i @ root + bias + sum_r AGG_{j : (j -> i) has relation r} x_j @ W_r
    with AGG the mean per (target, relation) over the edges AS GIVEN (duplicates count twice, self-loops are ordinary
    edges; a (target, relation) pair without an edge contributes 0, a node without in-edges gets the root term alone), or
    the sum with aggr="add" / "sum". W_r = weight[r], or sum_b comp[r, b] weight[b] with num_bases=B. Parameter names and
    shapes are PyG's: weight [num_bases or num_relations, in, out], comp [num_relations, num_bases] (only with
    num_bases), root [in, out] (root_weight), bias [out]; glorot, bias zeros.

    Both forms run the dense products first and touch the edges once (ops.rgcn_aggregate). Without a basis, the SELECT
    form: h = x @ [W_0 | ... | W_{R-1}] and the weighted SpMM picks column block type(p) of the source's row. IT
    MATERIALISES N * R * out FLOATS; num_bases is the answer for large R. With a basis, the MIX form: h = x @ [V_0 | ... |
    V_{B-1}] and the rgbx_rgcn_mix_* kernels mix the B rows of a source with comp[type(p), :], read on the device. An
    output width outside the kernels' set is zero-padded and sliced off again; a basis the kernels do not take (more than
    64 bases, more than 256 channels) composes W_r and runs the select form.

    Refused: num_blocks (NotImplementedError), x=None (featureless input), a tuple in_channels, any other aggr.
    Out of scope: FastRGCNConv, heterogeneous node types, the node-partitioned (distributed) route."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, *, num_blocks=None, aggr="mean",
                 root_weight=True, bias=True):
        super().__init__()
        if num_blocks is not None:
            raise NotImplementedError("RGCNConv: num_blocks (the block-diagonal decomposition) is not implemented; "
                                      "num_bases is")
        if not isinstance(in_channels, int) or isinstance(in_channels, bool):
            raise ValueError(f"RGCNConv: in_channels must be one int (got {in_channels!r}): bipartite and featureless "
                             "inputs are not implemented")
        if aggr not in ("mean", "add", "sum"):
            raise ValueError(f"RGCNConv: aggr={aggr!r} (mean, add or sum)")
        if num_relations < 1 or (num_bases is not None and num_bases < 1):
            raise ValueError("RGCNConv: num_relations and num_bases must be at least 1")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_relations, self.num_bases, self.aggr = num_relations, num_bases, aggr
        self.weight = nn.Parameter(torch.empty(num_bases or num_relations, in_channels, out_channels))
        if num_bases is not None:
            self.comp = nn.Parameter(torch.empty(num_relations, num_bases))
        else:
            self.register_parameter("comp", None)
        if root_weight:
            self.root = nn.Parameter(torch.empty(in_channels, out_channels))
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.weight)
        if self.comp is not None:
            glorot_(self.comp)
        if self.root is not None:
            glorot_(self.root)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def mix_channels(self):
        """The width the mix kernels run at for this layer (out_channels, or the next multiple of 4 where the layout
        does not take it), or None where the layer runs the select form."""
        C, B = self.out_channels, self.num_bases
        if B is None or C > 256:
            return None
        Cp = GATConv.kernel_channels(C)
        return Cp if ops.rgcn_mix_supported(B, Cp) else None

    def forward(self, x, edge_index, edge_type):
        if x is None:
            raise ValueError("RGCNConv: x=None (a featureless input) is not implemented")
        if not torch.is_tensor(edge_type) or edge_type.dtype != torch.int64 or edge_type.dim() != 1 \
                or edge_type.numel() != edge_index.size(1):
            got = f"{edge_type.dtype} {tuple(edge_type.shape)}" if torch.is_tensor(edge_type) else type(edge_type).__name__
            raise ValueError(f"RGCNConv: edge_type must be int64 [E] = [{edge_index.size(1)}], got {got}")
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"RGCNConv: x {tuple(x.shape)} for in_channels={self.in_channels}")
        _lib.require_device(x, edge_type)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        C, R, B = self.out_channels, self.num_relations, self.num_bases
        pad = torch.nn.functional.pad
        Cp = self.mix_channels()
        if Cp is None:
            w = self.weight if B is None else (self.comp @ self.weight.view(B, -1)).view(R, self.in_channels, C)
            comp, heads, Cp = None, R, C
        else:
            w = self.weight if Cp == C else pad(self.weight, (0, Cp - C))
            comp, heads = self.comp, B
        # [in, heads * Cp]: column block k is the k-th matrix
        h = ops.linear(x, w.permute(0, 2, 1).reshape(heads * Cp, self.in_channels))
        y0 = None
        if self.root is not None:
            y0 = ops.linear(x, self.root.t(), self.bias)
            y0 = y0 if Cp == C else pad(y0, (0, Cp - C))
        out = ops.rgcn_aggregate(h, graph, edge_type, R, comp=comp, aggr=self.aggr, y0=y0)
        out = out if Cp == C else out[:, :C]
        if self.root is None and self.bias is not None:
            out = out + self.bias
        return out


def _reset_module(module):
    """PyG's `reset`: a module's own reset_parameters, else that of its children, recursively."""
    if hasattr(module, "reset_parameters"):
        module.reset_parameters()
    else:
        for child in module.children():
            _reset_module(child)


class FiLMConv(nn.Module):
    """Feature-wise linear modulation [PyG FiLMConv; Brockschmidt, "GNN-FiLM: Graph Neural Networks with Feature-wise
    Linear Modulation"]: the TARGET node modulates every incoming message per channel, before the nonlinearity,
        beta_r, gamma_r = films[r](x).split(out, dim=-1)               (beta FIRST, then gamma: PyG's order)
        beta_s, gamma_s = film_skip(x).split(out, dim=-1)
        out_i = act(gamma_s[i] * lin_skip(x)[i] + beta_s[i])
              + sum_r AGG_{j : (j -> i) has relation r} act(gamma_r[i] * lins[r](x)[j] + beta_r[i])
    with AGG the mean per (target, relation) over the edges AS GIVEN (duplicates count twice, self-loops are ordinary
    edges; a (target, relation) pair without an edge contributes 0, a node without in-edges gets the skip term alone), or
    the sum with aggr="add" / "sum". Module names and shapes are PyG's: lins[r] = Linear(in, out, bias=False), films[r] =
    Linear(in, 2 * out) with bias or a deep copy of `nn`, lin_skip = Linear(in, out, bias=False), film_skip = Linear(in,
    2 * out, bias=False) or a deep copy of `nn`. `act`: "relu" (an nn.ReLU instance is accepted), None or "identity".
    With num_relations=1 `edge_type` is not needed (and ignored, as in PyG).

    The dense products run first (h and fb are each ONE product over the concatenated weights when `nn` is None) and the
    edges are touched once, in the rgbx_film_* kernels (ops.film_aggregate); the skip term is dense per-node work on
    torch, handed to the kernel as y0. THE FORM MATERIALISES N * R * 3 * out FLOATS (h: N * R * out, fb: N * R * 2 * out).
    An output width outside the kernels' set is zero-padded and sliced off again. Parity with PyG's implementation is
    unpinned (PyG is not installed where this project runs): the formulas above are the contract.

    Refused: a tuple in_channels (ValueError), an aggr other than mean / add / sum (ValueError), any other act
    (NotImplementedError). Out of scope: bipartite inputs, bf16 storage, the node-partitioned (distributed) route."""

    def __init__(self, in_channels, out_channels, num_relations=1, nn=None, act="relu", aggr="mean"):
        super().__init__()
        tnn = torch.nn  # the argument `nn` (PyG's name) shadows the module in here
        if not isinstance(in_channels, int) or isinstance(in_channels, bool):
            raise ValueError(f"FiLMConv: in_channels must be one int (got {in_channels!r}): bipartite inputs are not "
                             "implemented")
        if aggr not in ("mean", "add", "sum"):
            raise ValueError(f"FiLMConv: aggr={aggr!r} (mean, add or sum)")
        if isinstance(act, tnn.ReLU):
            act = "relu"
        if not (act is None or isinstance(act, str)) or act not in ("relu", "identity", None):
            raise NotImplementedError(f"FiLMConv: act={act!r} is not built (relu, None or identity: the nonlinearity "
                                      "lives in the kernels)")
        if num_relations < 1:
            raise ValueError("FiLMConv: num_relations must be at least 1")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_relations, self.act, self.aggr = num_relations, act, aggr
        self.custom_film = nn is not None
        self.lins, self.films = tnn.ModuleList(), tnn.ModuleList()
        for _ in range(num_relations):
            self.lins.append(Linear(in_channels, out_channels, bias=False))
            self.films.append(copy.deepcopy(nn) if nn is not None else Linear(in_channels, 2 * out_channels))
        self.lin_skip = Linear(in_channels, out_channels, bias=False)
        self.film_skip = copy.deepcopy(nn) if nn is not None else Linear(in_channels, 2 * out_channels, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        for module in list(self.lins) + list(self.films) + [self.lin_skip, self.film_skip]:
            _reset_module(module)  # the Linear's own default, as in PyG's layer

    def kernel_channels(self):
        """The width the aggregation runs at: out_channels where the kernels take it (their set up to 256, and column
        blocks of 256 above it whose last block is in the set), else the next multiple of 4."""
        C = self.out_channels
        last = C if C <= ops.FILM_BLOCK else (C % ops.FILM_BLOCK or ops.FILM_BLOCK)
        return C if GATConv.kernel_channels(last) == last else (C + 3) // 4 * 4

    def forward(self, x, edge_index, edge_type=None):
        R, C = self.num_relations, self.out_channels
        if R > 1 and (not torch.is_tensor(edge_type) or edge_type.dtype != torch.int64 or edge_type.dim() != 1
                      or edge_type.numel() != edge_index.size(1)):
            got = f"{edge_type.dtype} {tuple(edge_type.shape)}" if torch.is_tensor(edge_type) else type(edge_type).__name__
            raise ValueError(f"FiLMConv: edge_type must be int64 [E] = [{edge_index.size(1)}], got {got}")
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"FiLMConv: x {tuple(x.shape)} for in_channels={self.in_channels}")
        if R == 1:
            edge_type = None  # one relation: every edge has it, whatever the caller's vector says (PyG ignores it too)
        _lib.require_device(x, edge_type)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        Cp = self.kernel_channels()
        pad = torch.nn.functional.pad
        relu = torch.relu if self.act == "relu" else (lambda t: t)
        rows = (lambda w: w) if Cp == C else (lambda w: pad(w, (0, 0, 0, Cp - C)))       # zero weight rows
        cols = (lambda t: t) if Cp == C else (lambda t: pad(t, (0, Cp - C)))             # zero columns / bias entries
        # a padded channel has h = beta = gamma = 0: z = 0, which is 0 under both activations, and its cotangent is 0
        h = ops.linear(x, torch.cat([rows(lin.weight) for lin in self.lins]))
        if self.custom_film:
            parts = []
            for film in self.films:
                beta, gamma = film(x).split(C, dim=-1)
                parts += [cols(beta), cols(gamma)]
            fb = torch.cat(parts, dim=1)
        else:   # one product: per relation the beta rows, then the gamma rows
            w = torch.cat([rows(blk) for film in self.films for blk in film.weight.split(C, dim=0)])
            b = torch.cat([cols(blk) for film in self.films for blk in film.bias.split(C, dim=0)])
            fb = ops.linear(x, w, b)
        beta_s, gamma_s = self.film_skip(x).split(C, dim=-1)
        y0 = cols(relu(gamma_s * self.lin_skip(x) + beta_s))
        out = ops.film_aggregate(h, fb, graph, edge_type, R, aggr=self.aggr, act=self.act, y0=y0)
        return out if Cp == C else out[:, :C]


class GMMConv(nn.Module):
    """Gaussian mixture model convolution [PyG GMMConv; Monti et al., "Geometric deep learning on graphs and manifolds
    using mixture model CNNs" (MoNet)]: every edge carries `dim` pseudo-coordinates, edge_attr [E, dim], and
        gauss[e, k] = exp(sum_d -0.5 (edge_attr[e, d] - mu[k, d])^2 / (1e-15 + sigma[k, d]^2))
        out_i       = root(x_i) + bias + AGG_{j -> i} sum_k gauss[e, k] (x_j @ g)[k, :]
    with x @ g viewed as [N, kernel_size, out_channels] (k-major columns, PyG's x_j.view(E, K, M)) and AGG the mean
    (PyG's default) or the sum ("add" / "sum") over the edges AS GIVEN: self-loops stay, duplicates count twice, a node
    without in-edges gets the root term alone. Parameter names and shapes are PyG's: g [in, out * kernel_size], mu and
    sigma [kernel_size, dim], root.weight [out, in] (a bias-free Linear, with root_weight), bias [out]; glorot, bias
    zeros.

    The dense product runs first, the root term and the bias are folded into the aggregation's output (y0), the attribute
    rows are permuted into CSR slot order once at their raw width (ops.edge_rows_to_slots), and the mixture itself runs in
    the rgbx_gmm_* kernels (ops.gmm_aggregate), which read mu and sigma on the device: no [E, K, dim] or [E, K, out]
    tensor exists. An out_channels outside the kernels' widths is zero-padded and sliced off again.

    Refused: separate_gaussians=True (NotImplementedError); a tuple in_channels, an aggr other than mean / add / sum,
    dim > 8, kernel_size > 64, out_channels > 256, an edge_attr that is not float32 [E, dim] (ValueError).
    Out of scope: bipartite inputs, the node-partitioned (distributed) route."""

    def __init__(self, in_channels, out_channels, dim, kernel_size, separate_gaussians=False, aggr="mean",
                 root_weight=True, bias=True):
        super().__init__()
        if separate_gaussians:
            raise NotImplementedError("GMMConv: separate_gaussians=True (one mixture per input channel) is not "
                                      "implemented")
        if not isinstance(in_channels, int) or isinstance(in_channels, bool):
            raise ValueError(f"GMMConv: in_channels must be one int (got {in_channels!r}): bipartite inputs are not "
                             "implemented")
        if aggr not in ("mean", "add", "sum"):
            raise ValueError(f"GMMConv: aggr={aggr!r} (mean, add or sum)")
        if not 1 <= dim <= 8:
            raise ValueError(f"GMMConv: dim={dim}: the kernels take 1 to 8 pseudo-coordinates per edge")
        if not 1 <= kernel_size <= 64:
            raise ValueError(f"GMMConv: kernel_size={kernel_size}: the kernels take 1 to 64 Gaussian kernels")
        if not 1 <= out_channels <= 256:
            raise ValueError(f"GMMConv: out_channels={out_channels}: the kernels take 1 to 256 channels per kernel")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.dim, self.kernel_size, self.separate_gaussians, self.aggr = dim, kernel_size, False, aggr
        self.g = nn.Parameter(torch.empty(in_channels, out_channels * kernel_size))
        self.mu = nn.Parameter(torch.empty(kernel_size, dim))
        self.sigma = nn.Parameter(torch.empty(kernel_size, dim))
        if root_weight:
            self.root = Linear(in_channels, out_channels, bias=False)
        else:
            self.register_parameter("root", None)
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.g)
        glorot_(self.mu)
        glorot_(self.sigma)
        if self.root is not None:
            glorot_(self.root.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def kernel_channels(self):
        """The width per Gaussian kernel the aggregation runs at: out_channels, or the next multiple of 4 where the lane
        layout does not take it."""
        return GATConv.kernel_channels(self.out_channels)

    def forward(self, x, edge_index, edge_attr):
        E = edge_index.size(1)
        if not torch.is_tensor(edge_attr) or edge_attr.dim() != 2 or tuple(edge_attr.shape) != (E, self.dim) \
                or edge_attr.dtype != torch.float32:
            got = f"{edge_attr.dtype} {tuple(edge_attr.shape)}" if torch.is_tensor(edge_attr) else type(edge_attr).__name__
            raise ValueError(f"GMMConv: edge_attr must be float32 [E, dim] = [{E}, {self.dim}], got {got}")
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"GMMConv: x {tuple(x.shape)} for in_channels={self.in_channels}")
        _lib.require_device(x, edge_attr)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        e_slot = ops.edge_rows_to_slots(edge_attr, graph)
        return self.forward_slots(x, graph, e_slot)

    def forward_slots(self, x, graph, e_slot):
        """The layer on pseudo-coordinates that are already in the forward CSR slot order of `graph` (a LOOPS_KEEP
        graph): e_slot [nnz, dim] float32, what ops.edge_rows_to_slots or ops.degree_pseudo return."""
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f"GMMConv: x {tuple(x.shape)} for in_channels={self.in_channels}")
        _lib.require_device(x, e_slot)
        M, K = self.out_channels, self.kernel_size
        Mp = self.kernel_channels()
        pad = torch.nn.functional.pad
        g = self.g if Mp == M else pad(self.g.view(self.in_channels, K, M), (0, Mp - M)).reshape(self.in_channels, K * Mp)
        h = ops.linear(x, g.t())  # [N, K * Mp]: column block k is the k-th kernel's product
        y0 = None
        if self.root is not None:
            y0 = ops.linear(x, self.root.weight, self.bias)
            y0 = y0 if Mp == M else pad(y0, (0, Mp - M))
        out = ops.gmm_aggregate(h, e_slot, self.mu, self.sigma, graph, aggr=self.aggr, y0=y0)
        out = out if Mp == M else out[:, :M]
        if self.root is None and self.bias is not None:
            out = out + self.bias
        return out


class GatedGraphConv(nn.Module):
    """Gated graph convolution: the input (zero-padded to out_channels columns; wider inputs raise) runs through
    num_layers steps of m = x weight[i], agg_i = sum_{j -> i} m_j (edges as given, duplicates counted, no loops added,
    no normalisation), x = GRUCell(agg, x) [PyG GatedGraphConv(out_channels, num_layers, aggr='add', bias=True), as
    built at reference models/ggnn.py:18; parameter names weight, rnn.weight_ih / weight_hh / bias_ih / bias_hh, so a
    reference state_dict loads with strict=True]. Parity with PyG itself is not pinned (PyG is not available to the
    tests): the spec is the restatement in ops.gru_operands / csrc/gru.hip, checked against a float64 copy of it.
    Every step is one HIP launch where the fused kernel takes the width (ops.gru_step_supported), else the general form;
    state widths that are no multiple of 4 run on zero-padded state and weights, sliced off at the end."""

    def __init__(self, out_channels, num_layers, aggr="add", bias=True):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError(f"GatedGraphConv: only aggr='add' (the reference's) is implemented, got {aggr!r}")
        self.out_channels, self.num_layers, self.aggr = out_channels, num_layers, aggr
        self.weight = nn.Parameter(torch.empty(num_layers, out_channels, out_channels))
        self.rnn = nn.GRUCell(out_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_channels)  # PyG's uniform(size, tensor)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)
        self.rnn.reset_parameters()

    def forward(self, x, edge_index):
        C = self.out_channels
        if x.size(-1) > C:
            raise ValueError(f"GatedGraphConv: the number of input channels ({x.size(-1)}) must not exceed "
                             f"out_channels ({C})")
        if not x.is_cuda:
            _lib.require_device(x)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        Cp = (C + 3) // 4 * 4
        if x.size(-1) < Cp:  # PyG's zero columns up to C, and the pad columns up to Cp in the same copy
            x = torch.nn.functional.pad(x, (0, Cp - x.size(-1)))
        rnn = self.rnn
        for i in range(self.num_layers):
            weff, wroot, b = ops.gru_operands(self.weight[i], rnn.weight_ih, rnn.weight_hh, rnn.bias_ih, rnn.bias_hh, Cp)
            x = ops.gru_step(x, graph, weff, wroot, b)
        return x if Cp == C else x[:, :C]

    def __repr__(self):
        return f"{self.__class__.__name__}({self.out_channels}, num_layers={self.num_layers})"


class SuperGATConv(nn.Module):
    """SuperGAT's layer with 'MX' attention [PyG SuperGATConv; reference models/supergat.py]: h = x W^T viewed [N,H,C];
    for an edge j -> i: d = <h_i, h_j>, e = LeakyReLU((<h_j, att_l> + <h_i, att_r>) * sigmoid(d), 0.2); softmax over the
    in-edges of i (self-loops removed then re-added), dropout on the coefficients, out_i = sum_j alpha_ij h_j; heads
    concatenated or averaged; + bias. A training forward also forms the self-supervised attention loss — binary
    cross-entropy of the logits mean_h d over a sample of the edges (label 1) and sampled non-edges (label 0) — read
    with get_attention_loss(). All of it runs in the rgbx_supergat_* kernels (ops.supergat_attend)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, bias=True, attention_type="MX", edge_sample_ratio=1.0, neg_sample_ratio=0.5,
                 is_undirected=False):
        super().__init__()
        if attention_type != "MX":
            raise NotImplementedError(f"SuperGATConv: attention_type={attention_type!r}; only 'MX' (the reference's) is built")
        if not add_self_loops:
            raise NotImplementedError("SuperGATConv: add_self_loops=False is not built (the reference leaves it on)")
        if not (0.0 <= edge_sample_ratio <= 1.0 and 0.0 <= neg_sample_ratio and 0.0 <= dropout < 1.0):
            raise ValueError("SuperGATConv: edge_sample_ratio in [0, 1], neg_sample_ratio >= 0, dropout in [0, 1)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.heads, self.concat, self.negative_slope, self.dropout = heads, concat, negative_slope, dropout
        self.add_self_loops, self.attention_type = add_self_loops, attention_type
        self.edge_sample_ratio, self.neg_sample_ratio, self.is_undirected = edge_sample_ratio, neg_sample_ratio, is_undirected
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self._att_loss = None
        self.last_draw = {}  # seed and negative pairs of the last training forward (ops.supergat_random_choices)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.lin.weight)
        glorot_(self.att_l)
        glorot_(self.att_r)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def get_attention_loss(self):
        """The attention loss of the last forward (0 after an eval-mode forward)."""
        if self._att_loss is None:
            raise RuntimeError("SuperGATConv.get_attention_loss(): no forward has run yet")
        return self._att_loss

    def forward(self, x, edge_index, neg_edge_index=None):
        H, C = self.heads, self.out_channels
        Cp = GATConv.kernel_channels(C)
        graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD)
        in_kernel = self.bias is not None and (self.concat or H == 1)  # the bias rides in the aggregation kernel's store
        weight, att_l, att_r, bias = self.lin.weight, self.att_l, self.att_r, self.bias
        if Cp != C:  # pad every head with zero weight rows / attention entries: no score, logit or kept column changes
            pad = torch.nn.functional.pad
            weight = pad(weight.view(H, C, -1), (0, 0, 0, Cp - C)).reshape(H * Cp, -1)
            att_l, att_r = pad(att_l, (0, Cp - C)), pad(att_r, (0, Cp - C))
            if in_kernel:
                bias = pad(bias.view(H, C), (0, Cp - C)).reshape(-1)
        h = ops.linear(x, weight)
        self.last_draw = {}
        out, self._att_loss = ops.supergat_attend(
            h, att_l, att_r, graph, H, Cp, self.negative_slope, bias=bias if in_kernel else None, training=self.training,
            p_drop=self.dropout, pos_ratio=self.edge_sample_ratio, neg_ratio=self.neg_sample_ratio,
            neg_edge_index=neg_edge_index, record=self.last_draw)
        if Cp != C:
            out = out.view(-1, H, Cp)[:, :, :C].reshape(-1, H * C)
        if not self.concat and H > 1:
            out = out.view(-1, H, C).mean(dim=1)
        if self.bias is not None and not in_kernel:
            out = out + self.bias
        return out


class GATv2Conv(nn.Module):
    """GATv2's layer [PyG GATv2Conv; Brody et al., "How Attentive are Graph Attention Networks?"]: x_l = lin_l(x),
    x_r = lin_r(x) viewed [N,H,C]; for an edge j -> i: e_ij = <att, LeakyReLU(x_l[j] + x_r[i])> per head — the
    non-linearity in front of the attention vector, so the ranking of the neighbours depends on the target; softmax over
    the in-edges of i (self-loops removed then re-added), dropout on the coefficients, out_i = sum_j alpha_ij x_l[j];
    heads concatenated or averaged; + bias. Parameter names are PyG's (lin_l, lin_r, att, bias; lin_r is lin_l with
    share_weights). All of it runs in the rgbx_gatv2_* kernels (ops.gatv2_attend)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, bias=True, share_weights=False, *, edge_dim=None, residual=False):
        super().__init__()
        if not add_self_loops:
            raise NotImplementedError("GATv2Conv: add_self_loops=False is not built")
        if edge_dim is not None:
            raise NotImplementedError("GATv2Conv: edge features (edge_dim) are not built")
        if residual:
            raise NotImplementedError("GATv2Conv: residual=True is not built")
        if not (0.0 <= dropout < 1.0):
            raise ValueError("GATv2Conv: dropout in [0, 1)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.heads, self.concat, self.negative_slope, self.dropout = heads, concat, negative_slope, dropout
        self.add_self_loops, self.share_weights = add_self_loops, share_weights
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter("bias", None)
        self.last_draw = {}  # dropout seed of the last forward (ops.gatv2_random_choices)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r):
            glorot_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        glorot_(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _padded(self, lin, Cp):
        """(weight, bias) of a projection with every head padded to Cp channels by zero rows / entries."""
        H, C = self.heads, self.out_channels
        if Cp == C:
            return lin.weight, lin.bias
        pad = torch.nn.functional.pad
        weight = pad(lin.weight.view(H, C, -1), (0, 0, 0, Cp - C)).reshape(H * Cp, -1)
        return weight, None if lin.bias is None else pad(lin.bias.view(H, C), (0, Cp - C)).reshape(-1)

    def forward(self, x, edge_index):
        _lib.require_device(x)
        H, C = self.heads, self.out_channels
        Cp = GATConv.kernel_channels(C)  # other widths: zero weight rows, attention entries and bias per head
        F = H * Cp
        graph = get_graph(edge_index, x.size(0), LOOPS_REMOVE_ADD)
        in_kernel = self.bias is not None and (self.concat or H == 1)  # the bias rides in the aggregation kernel's store
        att, bias = self.att, self.bias
        w_l, b_l = self._padded(self.lin_l, Cp)
        if Cp != C:
            pad = torch.nn.functional.pad
            att = pad(att, (0, Cp - C))
            if in_kernel:
                bias = pad(bias.view(H, C), (0, Cp - C)).reshape(-1)
        if self.share_weights:
            xl = xr = ops.linear(x, w_l, b_l)
        else:  # one product over [W_l; W_r]; x_l and x_r are its column blocks
            w_r, b_r = self._padded(self.lin_r, Cp)
            h = ops.linear(x, torch.cat([w_l, w_r]), None if b_l is None else torch.cat([b_l, b_r]))
            xl, xr = h[:, :F], h[:, F:]
        self.last_draw = {}
        out = ops.gatv2_attend(xl, xr, att, graph, H, Cp, self.negative_slope, bias=bias if in_kernel else None,
                               training=self.training, p_drop=self.dropout, record=self.last_draw)
        if Cp != C:
            out = out.view(-1, H, Cp)[:, :, :C].reshape(-1, H * C)
        if not self.concat and H > 1:
            out = out.view(-1, H, C).mean(dim=1)
        if self.bias is not None and not in_kernel:
            out = out + self.bias
        return out


class TransformerConv(nn.Module):
    """UniMP's layer [PyG TransformerConv; Shi et al., "Masked Label Prediction"]: q = lin_query(x), k = lin_key(x),
    v = lin_value(x) viewed [N,H,C]; for an edge j -> i: e_ij = <q_i, k_j> / sqrt(C) per head, softmax over the in-edges
    of i — the edges AS GIVEN (self-loops stay, duplicates count twice, a node without in-edges aggregates zeros) —
    dropout on the coefficients, out_i = sum_j alpha_ij v_j; heads concatenated or averaged; root skip
    x_r = lin_skip(x): out + x_r, or with beta: b = sigmoid(lin_beta([out, x_r, out - x_r])), b x_r + (1 - b) out.
    Parameter names are PyG's (lin_key, lin_query, lin_value, lin_skip, lin_beta; `bias` is lin_skip's, the three
    projections always carry one; lin_skip exists without root_weight too, unused, as in PyG). The attention runs in
    the rgbx_transformer_* kernels (ops.transformer_attend); the root / gate arithmetic is dense per-node work."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("TransformerConv: edge features (edge_dim) are not built")
        if not (0.0 <= dropout < 1.0):
            raise ValueError("TransformerConv: dropout in [0, 1)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.heads, self.concat, self.dropout, self.edge_dim = heads, concat, dropout, edge_dim
        self.root_weight, self.beta = root_weight, bool(beta and root_weight)
        wide = heads * out_channels
        self.lin_key = nn.Linear(in_channels, wide)
        self.lin_query = nn.Linear(in_channels, wide)
        self.lin_value = nn.Linear(in_channels, wide)
        self.lin_skip = nn.Linear(in_channels, wide if concat else out_channels, bias=bias)
        if self.beta:
            self.lin_beta = nn.Linear(3 * (wide if concat else out_channels), 1, bias=False)
        else:
            self.lin_beta = None
        self.last_draw = {}  # dropout seed of the last forward (ops.transformer_random_choices)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()  # the Linear's own default, as in PyG's layer

    def _padded(self, lin, Cp):
        """(weight, bias) of a projection with every head padded to Cp channels by zero rows / entries."""
        H, C = self.heads, self.out_channels
        if Cp == C:
            return lin.weight, lin.bias
        pad = torch.nn.functional.pad
        weight = pad(lin.weight.view(H, C, -1), (0, 0, 0, Cp - C)).reshape(H * Cp, -1)
        return weight, pad(lin.bias.view(H, C), (0, Cp - C)).reshape(-1)

    def forward(self, x, edge_index):
        _lib.require_device(x)
        H, C = self.heads, self.out_channels
        Cp = GATConv.kernel_channels(C)  # other widths: zero weight rows and bias entries per head
        F = H * Cp
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        # one product over [W_q; W_k; W_v; W_skip]: the four projections are its column blocks, k and v of a source
        # side by side
        blocks = [self._padded(lin, Cp) for lin in (self.lin_query, self.lin_key, self.lin_value)]
        S = self.lin_skip.weight.size(0)
        if self.root_weight:
            # the skip block is padded to a multiple of 4 columns with zero weight rows: the rows of q, k and v (views
            # into the product) keep the 16-byte alignment the wide head widths (C > 128: 4 floats per lane) need
            w_skip, b_skip, extra = self.lin_skip.weight, self.lin_skip.bias, -S % 4
            if b_skip is None:
                b_skip = torch.zeros(S, dtype=x.dtype, device=x.device)
            if extra:
                pad = torch.nn.functional.pad
                w_skip, b_skip = pad(w_skip, (0, 0, 0, extra)), pad(b_skip, (0, extra))
            blocks.append((w_skip, b_skip))
        h = ops.linear(x, torch.cat([w for w, _ in blocks]), torch.cat([b for _, b in blocks]))
        self.last_draw = {}
        # the scale is that of the true head width: zero-padded channels add nothing to a dot product
        out = ops.transformer_attend(h[:, :F], h[:, F:2 * F], h[:, 2 * F:3 * F], graph, H, Cp, 1.0 / math.sqrt(C),
                                     training=self.training, p_drop=self.dropout, record=self.last_draw)
        if Cp != C:
            out = out.view(-1, H, Cp)[:, :, :C].reshape(-1, H * C)
        if not self.concat:
            out = out.view(-1, H, C).mean(dim=1)
        if self.root_weight:
            x_r = h[:, 3 * F:3 * F + S]
            if self.beta:
                b = torch.sigmoid(ops.linear(torch.cat([out, x_r, out - x_r], dim=-1), self.lin_beta.weight))
                out = b * x_r + (1.0 - b) * out
            else:
                out = out + x_r
        return out


class ResGatedGraphConv(nn.Module):
    """The residual gated graph convolution [PyG ResGatedGraphConv; Bresson & Laurent, "Residual Gated Graph ConvNets";
    GatedGCN in the benchmarking literature]: k = lin_key(x), q = lin_query(x), v = lin_value(x), all [N, C]; for an
    edge j -> i the message is sigmoid(k_i + q_j) * v_j, elementwise over the C channels — a gate per channel, not a
    scalar per head, and no normalisation; summed over the in-edges of i, the edges AS GIVEN (self-loops stay,
    duplicates count twice, a node without in-edges aggregates zeros); + lin_skip(x) with root_weight; + bias.
    Parameter names are PyG's (lin_key / lin_query / lin_value with bias, lin_skip without, present only with
    root_weight; `bias` only with bias). The aggregation runs in the rgbx_resgated_* kernels (ops.resgated_aggregate);
    the skip and bias adds are dense per-node work.

    Out of scope: edge features (`edge_dim`), activations other than the sigmoid default (`act`), the node-partitioned
    (distributed) route, and any kernel tuning beyond what the first measurement showed to be needed."""

    def __init__(self, in_channels, out_channels, act=None, edge_dim=None, root_weight=True, bias=True):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("ResGatedGraphConv: edge features (edge_dim) are not built")
        if not (act is None or act is torch.sigmoid or act is torch.nn.functional.sigmoid or isinstance(act, nn.Sigmoid)):
            raise NotImplementedError("ResGatedGraphConv: act other than the sigmoid default is not built (the gate's "
                                      "sigmoid lives in the kernels)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.edge_dim, self.root_weight = edge_dim, root_weight
        self.lin_key = nn.Linear(in_channels, out_channels)
        self.lin_query = nn.Linear(in_channels, out_channels)
        self.lin_value = nn.Linear(in_channels, out_channels)
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False) if root_weight else None
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            if lin is not None:
                lin.reset_parameters()  # the Linear's own default, as in PyG's layer
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index):
        _lib.require_device(x)
        C = self.out_channels
        Cp = GATConv.kernel_channels(C)  # other widths: zero weight rows and bias entries
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        pad = torch.nn.functional.pad
        # one product over [W_k; W_q; W_v; W_skip]: the four projections are its column blocks, q and v of a source side
        # by side. A padded channel has k = q = v = 0: sigmoid(0) * 0 = 0 forward and a zero gradient.
        blocks = [(lin.weight, lin.bias) if Cp == C else (pad(lin.weight, (0, 0, 0, Cp - C)), pad(lin.bias, (0, Cp - C)))
                  for lin in (self.lin_key, self.lin_query, self.lin_value)]
        if self.root_weight:
            # the skip block is padded to a multiple of 4 columns with zero weight rows: the product's leading dimension
            # stays a multiple of 4, and with it the 16-byte alignment the wide widths (C > 128: 4 floats per lane) need
            blocks.append((pad(self.lin_skip.weight, (0, 0, 0, -C % 4)),
                           torch.zeros(C + -C % 4, dtype=x.dtype, device=x.device)))
        h = ops.linear(x, torch.cat([w for w, _ in blocks]), torch.cat([b for _, b in blocks]))
        out = ops.resgated_aggregate(h[:, :Cp], h[:, Cp:2 * Cp], h[:, 2 * Cp:3 * Cp], graph)
        if Cp != C:
            out = out[:, :C]
        if self.root_weight:
            out = out + h[:, 3 * Cp:3 * Cp + C]
        if self.bias is not None:
            out = out + self.bias
        return out


class CGConv(nn.Module):
    """The crystal graph convolution [PyG CGConv; Xie & Grossman, "Crystal Graph Convolutional Neural Networks for an
    Accurate and Interpretable Prediction of Material Properties"]: with z_ij = [x_i, x_j, e_ij] (e_ij absent when
    dim = 0), out_i = x_i + bn(aggr_j sigmoid(lin_f(z_ij)) * softplus(lin_s(z_ij))), elementwise over the C channels,
    over the in-edges of i, the edges AS GIVEN (self-loops stay, duplicates count twice, a node without in-edges
    aggregates zeros, so it gets bn(0) + x_i). `edge_attr` [E, dim] holds one row per input edge. Parameter names are
    PyG's: lin_f, lin_s = Linear(2C + dim, C, bias=bias), bn (BatchNorm1d(C)) only with batch_norm.

    A Linear over a concatenation is a sum of three: the target and source terms of both maps are the column blocks of
    ONE product over x, the edge terms ONE product over the attribute rows, permuted into CSR slot order once at their
    raw width (ops.edge_rows_to_slots); gate, softplus, sum or mean and, without batch_norm, the root term x_i run in
    the rgbx_cgconv_* kernels (ops.cgconv_aggregate). A width outside the kernels' set is padded with zero weight rows
    and sliced off again.

    Out of scope: aggr="max" (the kernels form sums), bipartite `channels`, the node-partitioned (distributed) route,
    edge attributes through to_undirected / coalesce."""

    def __init__(self, channels, dim=0, aggr="add", batch_norm=False, bias=True):
        super().__init__()
        if isinstance(channels, (tuple, list)):
            raise NotImplementedError("CGConv: bipartite channels (a pair of widths) are not built")
        if aggr not in ("add", "mean"):
            raise NotImplementedError(f"CGConv: aggr={aggr!r} is not built (the kernels form sums: 'add' or 'mean')")
        self.channels, self.dim, self.aggr, self.batch_norm = int(channels), int(dim), aggr, batch_norm
        self.lin_f = Linear(2 * self.channels + self.dim, self.channels, bias=bias)
        self.lin_s = Linear(2 * self.channels + self.dim, self.channels, bias=bias)
        self.bn = BatchNorm1d(self.channels) if batch_norm else None
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_f.reset_parameters()
        self.lin_s.reset_parameters()
        if self.bn is not None:
            self.bn.reset_parameters()

    def forward(self, x, edge_index, edge_attr=None):
        C, D = self.channels, self.dim
        if x.dim() != 2 or x.size(1) != C:
            raise ValueError(f"CGConv: x must be [N, {C}], got {tuple(x.shape)}")
        if D == 0 and edge_attr is not None:
            raise ValueError("CGConv: built with dim=0, it takes no edge_attr")
        if D > 0 and (not torch.is_tensor(edge_attr) or edge_attr.dim() != 2 or edge_attr.size(1) != D
                      or edge_attr.size(0) != edge_index.size(1) or not edge_attr.is_floating_point()):
            got = tuple(edge_attr.shape) if torch.is_tensor(edge_attr) else type(edge_attr).__name__
            raise ValueError(f"CGConv: edge_attr must be float [E, dim] = [{edge_index.size(1)}, {D}], got {got}")
        _lib.require_device(x, edge_attr)
        Cp = GATConv.kernel_channels(C)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        pad = torch.nn.functional.pad
        rows = (lambda w: w) if Cp == C else (lambda w: pad(w, (0, 0, 0, Cp - C)))
        wf, ws = self.lin_f.weight, self.lin_s.weight
        # One product over [W_f^i; W_s^i; W_f^j; W_s^j]: a = its first 2 Cp columns (f half | s half, with the biases),
        # b the other 2 Cp. A padded channel has zf = zs = 0, so its message is sigmoid(0) softplus(0) = 0.5 ln 2, NOT
        # zero: it is harmless only because it is sliced off here and its gout is therefore zero.
        w_ab = torch.cat([rows(wf[:, :C]), rows(ws[:, :C]), rows(wf[:, C:2 * C]), rows(ws[:, C:2 * C])])
        b_ab = None
        if self.lin_f.bias is not None:
            vec = (lambda v: v) if Cp == C else (lambda v: pad(v, (0, Cp - C)))
            b_ab = torch.cat([vec(self.lin_f.bias), vec(self.lin_s.bias), x.new_zeros(2 * Cp)])
        h = ops.linear(x, w_ab, b_ab)
        c = None
        if D > 0 and edge_index.size(1) > 0:  # (no slot, no product)
            ea = ops.edge_rows_to_slots(edge_attr.to(torch.float32), graph)
            c = ops.linear(ea, torch.cat([rows(wf[:, 2 * C:]), rows(ws[:, 2 * C:])]))
        fused_root = self.bn is None and Cp == C
        out = ops.cgconv_aggregate(h[:, :2 * Cp], h[:, 2 * Cp:], c, graph, Cp, self.aggr, root=x if fused_root else None)
        if fused_root:
            return out
        if Cp != C:
            out = out[:, :C]
        return (out if self.bn is None else self.bn(out)) + x


class GENConv(nn.Module):
    """DeeperGCN's generalised graph convolution with the softmax aggregator [PyG GENConv(aggr="softmax"); Li et al.,
    "DeeperGCN: All You Need to Train Deeper GCNs"]: with xs = lin_src(x) and xd = lin_dst(x) (both layers exist only
    when in_channels != out_channels; otherwise xs = xd = x), the message of an edge j -> i is m_j = relu(xs_j) + eps,
    aggregated per channel by a softmax over the in-edges of i at temperature t — out_i = sum_j softmax_j(t m_j) m_j,
    the edges AS GIVEN (self-loops stay, duplicates count twice, a node without in-edges aggregates zeros) — then
    h = out + xd and the result is mlp(h): Linear(C, expansion C) -> BatchNorm1d over the nodes -> ReLU -> (the middle
    block again for num_layers > 2) -> Linear(expansion C, C). `t` is a Parameter with learn_t, a buffer otherwise; one
    value, or one per channel with per_channel_t. The aggregation runs in the rgbx_softmax_aggr_* kernels
    (ops.softmax_aggregate), which read t on the device; a width outside the kernels' set is padded with channels that
    hold eps everywhere and sliced off again.

    The layer follows the dataflow PyG documents for GENConv(aggr="softmax"); PyG is not a dependency here, so parity
    with its implementation (parameter names included: PyG keeps t in aggr_module and builds its MLP class) is unpinned.

    Out of scope: edge features (`edge_dim` / edge_attr), message normalisation (`msg_norm`), the power-mean and the
    other aggregators (`aggr`), the node-partitioned (distributed) route."""

    def __init__(self, in_channels, out_channels, t=1.0, learn_t=False, per_channel_t=False, eps=1e-7, num_layers=2,
                 expansion=2, bias=True, aggr="softmax", msg_norm=False, edge_dim=None):
        super().__init__()
        if aggr != "softmax":
            raise NotImplementedError(f"GENConv: aggr={aggr!r} is not built (softmax only)")
        if msg_norm:
            raise NotImplementedError("GENConv: msg_norm is not built")
        if edge_dim is not None:
            raise NotImplementedError("GENConv: edge features (edge_dim) are not built")
        if num_layers < 2 or expansion < 1:
            raise ValueError("GENConv: num_layers must be at least 2 and expansion at least 1")
        self.in_channels, self.out_channels, self.eps = in_channels, out_channels, float(eps)
        self.learn_t, self.per_channel_t, self.initial_t = learn_t, per_channel_t, float(t)
        C = out_channels
        if in_channels != out_channels:
            self.lin_src = Linear(in_channels, C, bias=bias)
            self.lin_dst = Linear(in_channels, C, bias=bias)
        else:
            self.lin_src = self.lin_dst = None
        widths = [C] + [C * expansion] * (num_layers - 1) + [C]
        layers = []
        for i in range(num_layers):
            layers.append(Linear(widths[i], widths[i + 1], bias=bias))
            if i < num_layers - 1:
                layers += [BatchNorm1d(widths[i + 1]), nn.ReLU()]
        self.mlp = nn.Sequential(*layers)
        temp = torch.full((C if per_channel_t else 1,), float(t))
        if learn_t:
            self.t = nn.Parameter(temp)
        else:
            self.register_buffer("t", temp)

    def reset_parameters(self):
        for mod in [self.lin_src, self.lin_dst] + list(self.mlp):
            if hasattr(mod, "reset_parameters"):
                mod.reset_parameters()
        with torch.no_grad():
            self.t.fill_(self.initial_t)

    def forward(self, x, edge_index):
        _lib.require_device(x)
        C = self.out_channels
        Cp = GATConv.kernel_channels(C)
        graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
        xs = x if self.lin_src is None else self.lin_src(x)
        xd = x if self.lin_dst is None else self.lin_dst(x)
        m = torch.relu(xs) + self.eps
        t = self.t
        if Cp != C:  # a padded channel holds eps in every row: it aggregates to eps and is sliced off again
            pad = torch.nn.functional.pad
            m = pad(m, (0, Cp - C), value=self.eps)
            if self.per_channel_t:
                t = pad(t, (0, Cp - C))
        out = ops.softmax_aggregate(m, t, graph)
        if Cp != C:
            out = out[:, :C]
        return self.mlp(out + xd)


class FAConv(nn.Module):
    """FAGCN's layer [PyG FAConv; reference models/fagcn.py]: for an edge j -> i of the GCN-normalised graph (self-loops
    removed then re-added, w_ij = 1/sqrt(d_i d_j)), a_ij = tanh(<x_j, att_l> + <x_i, att_r>) — signed, no softmax —
    with dropout on the coefficient, out_i = sum_j a_ij w_ij x_j + eps * x_0,i. Parameter names are PyG's
    (att_l.weight / att_r.weight [1, C], no bias). All of it runs in the rgbx_faconv_* kernels (ops.faconv);
    `form` (None | 'fused' | 'composed') forces one of the two kernel paths."""

    def __init__(self, channels, eps=0.1, dropout=0.0, add_self_loops=True, normalize=True):
        super().__init__()
        if not normalize:
            raise NotImplementedError("FAConv: normalize=False is not built (the reference leaves it on)")
        if not add_self_loops:
            raise NotImplementedError("FAConv: add_self_loops=False is not built (the reference leaves it on)")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("FAConv: dropout in [0, 1)")
        self.channels, self.eps, self.dropout = channels, eps, dropout
        self.add_self_loops, self.normalize = add_self_loops, normalize
        self.att_l = nn.Linear(channels, 1, bias=False)
        self.att_r = nn.Linear(channels, 1, bias=False)
        self.form = None
        self.last_draw = {}  # dropout seed of the last forward (ops.faconv_random_choices)

    def reset_parameters(self):
        self.att_l.reset_parameters()
        self.att_r.reset_parameters()

    def forward(self, x, x_0, edge_index):
        _lib.require_device(x, x_0)
        graph = get_graph(edge_index, x.size(0), LOOPS_ADD_REMAINING)
        self.last_draw = {}
        return ops.faconv(x, x_0, self.att_l.weight, self.att_r.weight, graph, eps=self.eps, training=self.training,
                          p_drop=self.dropout, form=self.form, record=self.last_draw)
