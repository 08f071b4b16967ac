"""Device-resident graph structures for the message-passing kernels.

The reference recomputes the self-loop rewrite and ``gcn_norm`` inside every conv call
(models/gcn.py:27 -> GCNConv.forward [PyG]; models/graphsage.py:53-56; restated at
models/dagnn.py:12-31). ``edge_index`` is constant inside ``experiment()``
(itexperiments.py:332), so here the int64 edge list is turned ONCE into a CSR grouped by target
(forward) and one grouped by source (backward), by ``rgbx_csr_build``; results are cached per
``edge_index`` tensor.

HBM layout per graph (E' = edges after the rewrite):
  rowptr  int32 [N+1]   |  col  int32 [E']  |  perm int32 [E'] (slot -> input edge id)
  dis     f32   [N]     deg^-1/2 over the target index           (GCN / APPNP)
  w       f32   [E']    dis[src]*dis[tgt] per forward slot; w_t the same per transposed slot
  inv_deg f32   [N]     1/max(deg,1) (mean);  w_mean_t f32 [E'] = inv_deg[tgt] per transposed slot

Weighted graphs (``get_graph(..., edge_weight=ew)``, the ``edge_weight`` argument of gcn_norm at models/dagnn.py:12-31)
share the unweighted entry's CSR arrays and add
  loop_w  f32   [N]     weight of every added self-loop;  loop_src int32 [N] the input self-loop it came from, or -1
  ew_slot f32   [E']    the input weight per forward slot (ew_slot_t per transposed slot)
with dis = (sum of ew_slot over the row)^-1/2 and w = dis[src] * ew * dis[tgt].
"""
import ctypes
from collections import OrderedDict

import torch

from . import _lib

LOOPS_KEEP = 0
LOOPS_ADD_REMAINING = 1
LOOPS_REMOVE_ADD = 2


LONG_ROW_SLOTS = 1024  # rows with more slots are cut into chunks of this many, summed by separate waves


class CSR:
    """CSR over `N` aggregation rows: rowptr [N+1], col / perm [E'] (int32, device); `split` is the
    hub-row plan (None when no row exceeds LONG_ROW_SLOTS)."""

    __slots__ = ("rowptr", "col", "perm", "N", "nnz", "split")

    def __init__(self, rowptr, col, perm, N, nnz, split=None):
        self.rowptr, self.col, self.perm, self.N, self.nnz, self.split = rowptr, col, perm, N, nnz, split

    def split_arg(self, d, device, hub_rows=False):
        """ctypes rgbx_row_split_t for one launch at width d (allocates the partial scratch), or None.
        `hub_rows`: room for the n_long finished hub-row aggregates after the chunk partials
        (rgbx_spmm_linear_f32); 2 = for two sets of them (rgbx_fused_layer_t.w_pos)."""
        if self.split is None:
            return None, None
        sp = self.split
        partial = torch.empty((sp["n_chunks"] + sp["n_long"] * int(hub_rows), d), dtype=torch.float32, device=device)
        st = _lib.RowSplit(sp["threshold"], sp["n_chunks"], sp["n_long"], sp["chunk_begin"].data_ptr(),
                           sp["chunk_end"].data_ptr(), sp["chunk_row"].data_ptr(), sp["long_row"].data_ptr(),
                           sp["long_chunk_ptr"].data_ptr(), partial.data_ptr())
        return st, partial


def make_row_split(rowptr, threshold=None):
    """Chunk plan for rows with more than `threshold` slots (index arithmetic on the device, once)."""
    threshold = LONG_ROW_SLOTS if threshold is None else threshold
    deg = (rowptr[1:] - rowptr[:-1]).long()
    if deg.numel() == 0 or int(deg.max().item()) <= threshold:
        return None
    long_row = (deg > threshold).nonzero(as_tuple=True)[0]
    nch = (deg[long_row] + threshold - 1) // threshold
    ptr = torch.zeros(long_row.numel() + 1, dtype=torch.int64, device=rowptr.device)
    ptr[1:] = torch.cumsum(nch, 0)
    n_chunks = int(ptr[-1].item())
    owner = torch.repeat_interleave(torch.arange(long_row.numel(), device=rowptr.device), nch)
    k = torch.arange(n_chunks, device=rowptr.device) - ptr[:-1][owner]
    begin = rowptr[long_row].long()[owner] + k * threshold
    end = torch.minimum(begin + threshold, rowptr[long_row + 1].long()[owner])
    i32 = lambda t: t.to(torch.int32).contiguous()
    return {"threshold": int(threshold), "n_chunks": n_chunks, "n_long": int(long_row.numel()),
            "chunk_begin": i32(begin), "chunk_end": i32(end), "chunk_row": i32(long_row[owner]),
            "long_row": i32(long_row), "long_chunk_ptr": i32(ptr)}


def build_csr(agg_row, other_row, N, loops_mode):
    """int64 device vectors (aggregate-into index, gather-from index) -> CSR via the HIP library."""
    _lib.require_device(agg_row, other_row)
    E = agg_row.numel()
    dev = agg_row.device
    agg_row = agg_row.contiguous()
    other_row = other_row.contiguous()
    nbytes = ctypes.c_size_t(0)
    _lib.call("rgbx_csr_workspace_bytes", E, N, ctypes.byref(nbytes))
    cap = max(E + N, 1)
    rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
    col = torch.empty(cap, dtype=torch.int32, device=dev)
    perm = torch.empty(cap, dtype=torch.int32, device=dev)
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
    _lib.launch("rgbx_csr_build", agg_row, other_row, E, N, loops_mode, rowptr, col, perm, ws, ws.numel())
    nnz = int(rowptr[N].item())  # one sync per graph; also orders `ws` lifetime after the kernels
    return CSR(rowptr, col[:max(nnz, 1)], perm[:max(nnz, 1)], N, nnz, make_row_split(rowptr))


class Graph:
    """All cached structures of one (edge_index, N, loops_mode)."""

    def __init__(self, edge_index, num_nodes, loops_mode):
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
            raise RuntimeError(f"edge_index must be int64 [2, E], got {edge_index.dtype} {tuple(edge_index.shape)}")
        _lib.require_device(edge_index)
        self.N = int(num_nodes)
        self.E = int(edge_index.size(1))
        self.loops_mode = loops_mode
        if self.E > 0:
            lo, hi = int(edge_index.min().item()), int(edge_index.max().item())
            if lo < 0 or hi >= self.N:
                raise RuntimeError(f"edge_index values [{lo}, {hi}] outside [0, {self.N})")
        self._src = edge_index[0]
        self._dst = edge_index[1]
        self.fwd = build_csr(self._dst, self._src, self.N, loops_mode)
        self._bwd = None
        self._dis = self._w = self._w_t = self._inv_deg = self._w_mean_t = None

    # transposed CSR (rows = sources) for backward
    @property
    def bwd(self):
        if self._bwd is None:
            self._bwd = build_csr(self._src, self._dst, self.N, self.loops_mode)
        return self._bwd

    def _f32(self, n):
        return torch.empty(max(n, 1), dtype=torch.float32, device=self.fwd.rowptr.device)

    @property
    def dis(self):
        if self._dis is None:
            self._dis = self._f32(self.N)
            _lib.launch("rgbx_deg_inv_sqrt_f32", self.fwd.rowptr, self.N, self._dis)
        return self._dis

    def _norm(self, csr):
        w = self._f32(csr.nnz)
        _lib.launch("rgbx_gcn_norm_f32", csr.rowptr, csr.col, self.N, self.dis, w)
        return w

    @property
    def w(self):
        if self._w is None:
            self._w = self._norm(self.fwd)
        return self._w

    @property
    def w_t(self):
        if self._w_t is None:
            self._w_t = self._norm(self.bwd)
        return self._w_t

    @property
    def inv_deg(self):
        if self._inv_deg is None:
            self._inv_deg = self._f32(self.N)
            _lib.launch("rgbx_inv_degree_f32", self.fwd.rowptr, self.N, self._inv_deg)
        return self._inv_deg

    def rowsum(self, kind):
        """Sum of the aggregation weights of every row: sum_p w[p] ('gcn') or 1 / 0 for rows with / without
        in-edges ('mean', whose weights 1/deg sum to 1). What a constant column contributes to the aggregate: the
        fused kernel needs it to push an affine map of its input through the aggregation (ops.bn_propagate_linear)."""
        cache = self.__dict__.setdefault("_rowsum", {})
        if kind not in cache:
            if kind == "gcn":
                from . import ops
                ones = torch.ones((self.N, 1), dtype=torch.float32, device=self.fwd.rowptr.device)
                cache[kind] = ops.spmm_raw(self.fwd, self.w, None, ones, kind="rowsum").reshape(-1).contiguous()
            elif kind == "mean":
                cache[kind] = ((self.fwd.rowptr[1:] - self.fwd.rowptr[:-1]) > 0).to(torch.float32).contiguous()
            else:
                raise ValueError(kind)
        return cache[kind]

    @property
    def undirected_keys(self):
        """(keys, count): the ascending distinct 64-bit keys a * N + b of the undirected edge set (both directions of every
        input edge; rgbx_coalesce_keys_i64 with mirror = 1), built once: what the SuperGAT negative sampler searches."""
        cached = self.__dict__.get("_und_keys")
        if cached is None:
            dev = self.fwd.rowptr.device
            M = 2 * self.E
            keys = torch.empty(max(M, 1), dtype=torch.int64, device=dev)
            count = 0
            if M:
                nbytes = ctypes.c_size_t(0)
                _lib.call("rgbx_coalesce_workspace_bytes", self.E, self.N, 1, ctypes.byref(nbytes))
                counts = torch.empty(2, dtype=torch.int64, device=dev)
                ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=dev)
                _lib.launch("rgbx_coalesce_keys_i64", self._src.contiguous(), self._dst.contiguous(), self.E, self.N, 1,
                            keys, counts, ws, ws.numel())
                count = int(counts[0].item())  # one read-back per graph
            cached = self._und_keys = (keys, count)
        return cached

    @property
    def t2f(self):
        """int32 [E']: the forward CSR slot of every transposed CSR slot (same edge), from the two slot -> edge-id
        permutations; the SuperGAT backward keys an edge's random decisions by its forward slot."""
        cached = self.__dict__.get("_t2f")
        if cached is None:
            f, b = self.fwd, self.bwd
            if f.nnz:
                inv = torch.empty(int(max(f.perm[:f.nnz].max(), b.perm[:b.nnz].max()).item()) + 1, dtype=torch.int32,
                                  device=f.perm.device)
                inv[f.perm[:f.nnz].long()] = torch.arange(f.nnz, dtype=torch.int32, device=inv.device)
                cached = inv[b.perm[:b.nnz].long()].contiguous()
            else:
                cached = b.col
            self._t2f = cached
        return cached

    @property
    def w_mean_t(self):
        """Per transposed slot (j -> i): 1/deg(i), the weight of dY[i] in dX[j] for aggr='mean'."""
        if self._w_mean_t is None:
            self._w_mean_t = self.inv_deg[self.bwd.col.long()].contiguous() if self.bwd.nnz else self._f32(0)
        return self._w_mean_t


def check_edge_weight(edge_weight, edge_index):
    """The contract of an `edge_weight` argument, checked before any launch: float32 [E] on edge_index's device."""
    if not isinstance(edge_weight, torch.Tensor):
        raise ValueError(f"edge_weight must be a tensor, got {type(edge_weight).__name__}")
    if edge_weight.dtype != torch.float32:
        raise ValueError(f"edge_weight must be float32, got {edge_weight.dtype}")
    if edge_weight.dim() != 1 or edge_index.dim() != 2 or edge_weight.numel() != edge_index.size(1):
        raise ValueError(f"edge_weight must have shape [E] = [{edge_index.size(-1)}], got {tuple(edge_weight.shape)}")
    if edge_weight.device != edge_index.device:
        raise ValueError(f"edge_weight is on '{edge_weight.device}', edge_index on '{edge_index.device}'")


class WeightedGraph(Graph):
    """A Graph with per-edge weights: gcn_norm(edge_index, edge_weight) of models/dagnn.py:12-31. The CSR arrays (and the
    sort behind them) are the unweighted entry's; `dis`, `w`, `w_t` and rowsum('gcn') are the weighted ones. The mean
    aggregation has no weighted form (PyG's SAGEConv takes no edge_weight): `inv_deg` / `w_mean_t` raise."""

    def __init__(self, base, edge_weight):
        check_edge_weight(edge_weight, base._keepalive)
        _lib.require_device(edge_weight)
        ew = edge_weight.detach().contiguous()
        if ew.numel() and not bool(torch.isfinite(ew).all().item()):
            raise ValueError("edge_weight holds non-finite values")
        self.base = base
        self.N, self.E, self.loops_mode = base.N, base.E, base.loops_mode
        self._src, self._dst = base._src, base._dst
        self.fwd = base.fwd
        self.ew = ew
        self._dis = self._w = self._w_t = None
        self._loops = self._ew_slot = self._ew_slot_t = None

    bwd = property(lambda self: self.base.bwd)
    t2f = property(lambda self: self.base.t2f)
    undirected_keys = property(lambda self: self.base.undirected_keys)

    @property
    def loops(self):
        """(loop_w f32 [N], loop_src int32 [N]) of the added self-loops, or (None, None) for LOOPS_KEEP."""
        if self._loops is None:
            if self.loops_mode == LOOPS_KEEP:
                self._loops = (None, None)
            else:
                loop_w = self._f32(self.N)
                loop_src = torch.empty(max(self.N, 1), dtype=torch.int32, device=loop_w.device)
                _lib.launch("rgbx_loop_weights_f32", self._src.contiguous(), self._dst.contiguous(), self.ew, self.E, self.N,
                            self.loops_mode, 1.0, loop_w, loop_src)
                self._loops = (loop_w, loop_src)
        return self._loops

    def _slot_weights(self, csr):
        out = self._f32(csr.nnz)
        _lib.launch("rgbx_edge_slot_weights_f32", csr.perm, csr.nnz, self.ew, self.E, self.loops[0], out)
        return out

    @property
    def ew_slot(self):
        if self._ew_slot is None:
            self._ew_slot = self._slot_weights(self.fwd)
        return self._ew_slot

    @property
    def ew_slot_t(self):
        if self._ew_slot_t is None:
            self._ew_slot_t = self._slot_weights(self.bwd)
        return self._ew_slot_t

    @property
    def dis(self):
        if self._dis is None:
            self._dis = self._f32(self.N)
            _lib.launch("rgbx_weighted_deg_inv_sqrt_f32", self.fwd.rowptr, self.ew_slot, self.N, self._dis)
        return self._dis

    def _norm_weighted(self, csr, ew_slot):
        w = self._f32(csr.nnz)
        _lib.launch("rgbx_gcn_norm_weighted_f32", csr.rowptr, csr.col, ew_slot, self.N, self.dis, w)
        return w

    @property
    def w(self):
        if self._w is None:
            self._w = self._norm_weighted(self.fwd, self.ew_slot)
        return self._w

    @property
    def w_t(self):
        if self._w_t is None:
            self._w_t = self._norm_weighted(self.bwd, self.ew_slot_t)
        return self._w_t

    @property
    def inv_deg(self):
        raise RuntimeError("a weighted graph has no mean aggregation: SAGEConv takes no edge_weight [PyG]")

    w_mean_t = inv_deg

    def rowsum(self, kind):
        if kind != "gcn":
            raise RuntimeError("a weighted graph has no mean aggregation: SAGEConv takes no edge_weight [PyG]")
        return Graph.rowsum(self, kind)


_CACHE = OrderedDict()
_CACHE_MAX = 16
_PINNED = {}


def _key(edge_index, num_nodes, loops_mode):
    return (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, str(edge_index.device),
            int(num_nodes), int(loops_mode))


def register_graph(edge_index, num_nodes, loops_mode, graph):
    """Bind a prepared graph object (e.g. a dist.DistGraph) to an edge_index tensor; pinned entries
    are not evicted."""
    graph._keepalive = edge_index
    _PINNED[_key(edge_index, num_nodes, loops_mode)] = graph


def get_graph(edge_index, num_nodes, loops_mode, edge_weight=None):
    """Cached Graph for this edge_index tensor (identity + in-place version), N and rewrite mode. With `edge_weight`
    (float32 [E], same device, finite; else ValueError before any launch) a WeightedGraph over the same CSR arrays, cached
    under the weight tensor's identity, shape and version as well; a weight that requires grad is prepared anew on every
    call (its values move with every optimizer step) and not cached."""
    if edge_weight is not None:
        return _get_weighted(edge_index, num_nodes, loops_mode, edge_weight)
    key = _key(edge_index, num_nodes, loops_mode)
    g = _PINNED.get(key)
    if g is not None:
        return g
    g = _CACHE.get(key)
    if g is None:
        g = Graph(edge_index, num_nodes, loops_mode)
        g._keepalive = edge_index  # the key holds data_ptr: keep the storage alive while cached
        _CACHE[key] = g
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return g


def _get_weighted(edge_index, num_nodes, loops_mode, edge_weight):
    check_edge_weight(edge_weight, edge_index)
    key = _key(edge_index, num_nodes, loops_mode) + (edge_weight.data_ptr(), tuple(edge_weight.shape),
                                                     edge_weight._version)
    g = None if edge_weight.requires_grad else _CACHE.get(key)
    if g is not None:
        _CACHE.move_to_end(key)
        return g
    base = get_graph(edge_index, num_nodes, loops_mode)
    if getattr(base, "is_distributed", False):
        raise NotImplementedError("edge weights on a partitioned graph are not implemented")
    g = WeightedGraph(base, edge_weight)
    g._keepalive = edge_index
    if not edge_weight.requires_grad:
        g._keepalive_weight = edge_weight  # the key holds its data_ptr
        _CACHE[key] = g
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    return g


def clear_cache():
    _CACHE.clear()
    _PINNED.clear()


def forget(edge_index):
    """Drop the cached (not the pinned) graphs of this edge_index tensor. A sampled mini-batch's edge list lives for one
    training step: left in the cache, sixteen of them would push the whole graph's own structures out between two
    evaluation forwards."""
    head = _key(edge_index, 0, 0)[:4]
    for key in [k for k in _CACHE if k[:4] == head]:
        del _CACHE[key]
