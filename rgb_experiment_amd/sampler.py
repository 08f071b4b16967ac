"""Neighbour sampling: fan-out mini-batches drawn by HIP kernels (csrc/sample.hip), the sampler of the GraphSAGE paper.

A sampled batch is an ordinary ``(x, edge_index)`` pair over local ids, so every layer and model of the package runs on it
unchanged. Hop h draws, for exactly the nodes that entered the batch at hop h - 1 (hop 0: the seeds), at most
``num_neighbors[h]`` of their in-edges (-1: all of them) — a node's in-edges are drawn once. The draw is a hash of
(seed, hop, node, position in the node's CSR row): see ops.sample_neighbors; it does not depend on launch geometry.

Per hop the host waits twice: for the hop's edge count (it sizes the outputs and picks the kernels) and for the number of
new nodes (it sizes the next hop); each of the two also asks the library for its workspace size and allocates it.
``sample`` adds, once per batch, the check of its seeds: three more read-backs (min, max, and the count of a
``torch.unique``, a sort). ``sample_unchecked`` leaves them out for a caller whose seeds are distinct and in range by
construction (``experiment()``: slices of a permutation of the training rows). Everything else — the draw, the sort of
the candidates, the relabelling — stays on the device.

A batch's ``edge_index`` is a fresh tensor, and every layer that runs on it builds and caches that batch's graph
structures (``graph.get_graph`` keeps up to 16 edge lists alive). A training loop calls ``graph.forget(batch.edge_index)``
after its step, as ``experiment()`` does, so that batches do not pile up in the cache or push the whole graph's
structures out of it.

Layers that keep state from their first call (``SGConv(cached=True)``) must not run on batches: the kept rows are the first
batch's. ``experiment()`` refuses them.

What a batch forward computes. Layers that normalise by the TARGET only (mean / sum / max SAGE, GIN, the attention
families) are exact on the seed rows once there are as many hops as layers and every fan-out is -1: every seed then sees
its whole L-hop neighbourhood. Layers that normalise by the SOURCE's degree too (``GCNConv``'s ``gcn_norm``) see the
batch's degrees: a node of the batch's outer ring has none of its in-edges in the batch, so its degree there is not its
degree in the graph, and the result is not exact even with full fan-outs — as with PyG's NeighborLoader.
"""
import torch

from . import _lib, ops
from .graph import LOOPS_KEEP, get_graph


def check_num_neighbors(num_neighbors):
    """A non-empty list of fan-outs, each an int >= 1 or -1 (ValueError otherwise); returned as a list."""
    if isinstance(num_neighbors, (str, bytes)) or not hasattr(num_neighbors, "__iter__"):
        raise ValueError(f"num_neighbors must be a non-empty list of ints, got {num_neighbors!r}")
    fanouts = list(num_neighbors)
    if not fanouts:
        raise ValueError("num_neighbors must name at least one hop")
    for k in fanouts:
        ops.check_fanout(k)
    return fanouts


class SampledBatch:
    """n_id int64 [n] (global ids: the seeds in the order given, then each hop's new nodes ascending), edge_index int64
    [2, E_b] (local ids, source row 0, target row 1; hop by hop, row by row, slot ascending), e_id int64 [E_b] (the column
    of the input edge_index behind every sampled edge), num_seeds."""

    __slots__ = ("n_id", "edge_index", "e_id", "num_seeds")

    def __init__(self, n_id, edge_index, e_id, num_seeds):
        self.n_id, self.edge_index, self.e_id, self.num_seeds = n_id, edge_index, e_id, num_seeds


class NeighborSampler:
    """``NeighborSampler(edge_index, num_nodes, num_neighbors).sample(seeds, seed=None) -> SampledBatch``.

    ``edge_index`` int64 [2, E] on the device (source row 0, target row 1); its target-grouped CSR is the cached one
    every layer in ``LOOPS_KEEP`` mode uses. The sampler owns ``local_of`` (int32 [N], global id -> id in the batch), which
    is -1 everywhere between calls: a batch sets and resets its own entries only. There is no CPU fallback."""

    def __init__(self, edge_index, num_nodes, num_neighbors):
        self.num_neighbors = check_num_neighbors(num_neighbors)
        self.graph = get_graph(edge_index, num_nodes, LOOPS_KEEP)
        if getattr(self.graph, "is_distributed", False):
            raise NotImplementedError("neighbour sampling on a partitioned graph is not implemented")
        self.N = self.graph.N
        self.device = edge_index.device
        self.local_of = torch.full((max(self.N, 1),), -1, dtype=torch.int32, device=self.device)

    def _check_seeds(self, seeds):
        if not isinstance(seeds, torch.Tensor):
            raise ValueError(f"seeds must be a tensor, got {type(seeds).__name__}")
        _lib.require_device(seeds)
        if seeds.dim() != 1 or seeds.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"seeds must be a 1-D int32 / int64 tensor, got {seeds.dtype} {tuple(seeds.shape)}")
        if seeds.device != self.device:
            raise ValueError(f"seeds are on '{seeds.device}', the graph on '{self.device}'")
        if seeds.numel():
            lo, hi = int(seeds.min()), int(seeds.max())
            if lo < 0 or hi >= self.N:
                raise ValueError(f"seeds [{lo}, {hi}] outside [0, {self.N})")
            if int(torch.unique(seeds).numel()) != seeds.numel():
                raise ValueError("seeds must be distinct")
        return seeds.to(torch.int32).contiguous()

    def _seed_words(self, seed):
        if seed is None:
            return ops.sample_seed(self.device)
        if isinstance(seed, torch.Tensor):
            _lib.require_device(seed)
            if seed.dtype != torch.int32 or seed.numel() != 2:
                raise ValueError("seed must hold two int32 words")
            return seed.contiguous()
        words = [int(w) for w in seed]
        if len(words) != 2 or any(w < -2 ** 31 or w >= 2 ** 31 for w in words):
            raise ValueError("seed must be two int32 words")
        return torch.tensor(words, dtype=torch.int32, device=self.device)

    def sample(self, seeds, seed=None):
        """One batch around the distinct, in-range `seeds` (ValueError otherwise, before any launch). `seed`: two int32
        words (a device tensor or a pair of ints); None takes them from torch's device generator."""
        return self._draw(self._check_seeds(seeds), self._seed_words(seed))

    def sample_unchecked(self, seeds, seed=None):
        """`sample` without the range and distinctness checks (and their three read-backs): for seeds that are distinct
        and in [0, N) by construction, e.g. a slice of a permutation. Seeds that are not give an undefined batch (to the kernels an id
        outside [0, N) is a row without in-edges; a hop that keeps more slots than the graph has raises)."""
        _lib.require_device(seeds)
        if seeds.dim() != 1 or seeds.dtype not in (torch.int32, torch.int64) or seeds.device != self.device:
            raise ValueError(f"seeds must be a 1-D int32 / int64 tensor on '{self.device}'")
        return self._draw(seeds.to(torch.int32).contiguous(), self._seed_words(seed))

    def _draw(self, rows, words):
        num_seeds = rows.numel()
        csr, local_of = self.graph.fwd, self.local_of
        ids, edges, e_ids = [rows], [], []
        first_row, n = 0, rows.numel()
        try:
            ops.sample_set_local(rows, 0, local_of)
            for hop, fanout in enumerate(self.num_neighbors):
                if rows.numel() == 0:
                    break
                rowptr, col, slot = ops.sample_hop_raw(csr, rows, fanout, words, hop)
                new = ops.sample_frontier(col, local_of, n)
                ei, e_id = ops.sample_relabel(rowptr, col, slot, local_of, csr.perm, first_row)
                edges.append(ei)
                e_ids.append(e_id)
                ids.append(new)
                first_row, n, rows = n, n + new.numel(), new
        except BaseException:
            local_of.fill_(-1)  # (whatever the failed hop had entered is not in `ids`)
            raise
        n_id = torch.cat(ids)
        ops.sample_set_local(n_id, -1, local_of)  # O(batch): the batch's own entries
        if edges:
            edge_index, e_id = torch.cat(edges, dim=1), torch.cat(e_ids)
        else:
            edge_index = torch.zeros((2, 0), dtype=torch.int64, device=self.device)
            e_id = torch.zeros(0, dtype=torch.int64, device=self.device)
        return SampledBatch(n_id.to(torch.int64), edge_index, e_id, num_seeds)
