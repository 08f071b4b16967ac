"""numpy restatement of the neighbour sampler (csrc/sample.hip, rgb_experiment_amd/sampler.py) and the graphs its tests
run on (a test helper shared by test_neighbor_sample_host.py and test_gpu_neighbor_sample.py; nothing here needs a GPU).

The draw: row g at hop h keeps, of the deg slots of its CSR row, the min(k, deg) with the smallest 64-bit keys
(draw32(seed0, seed1, STREAM + h, g, t) << 32) | t, t = slot - rowptr[g], in ascending slot order; k = -1 keeps all."""
import numpy as np

STREAM = 0x082EFA98
SHORT_ROW_SLOTS = 64     # row-length boundaries of the selection kernels (ops.SAMPLE_*)
WAVE_ROW_SLOTS = 1024    # = graph.LONG_ROW_SLOTS
HUB_SLOTS = 5000
FANOUTS = (1, 2, 5, 64, 100, -1)
_M = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x).astype(np.int64).astype(np.uint64) & _M


def mix32(x):
    """csrc/rgbx_rng.h: mix32, on uint64 arrays holding 32-bit values."""
    x = _u(x)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M
    x ^= x >> np.uint64(16)
    return x


def draw32(s0, s1, stream, a, b):
    """csrc/rgbx_rng.h: draw32."""
    inner = (mix32(_u(a) ^ _u(s0)) + ((_u(b) * np.uint64(0x9E3779B9)) & _M) + _u(stream)) & _M
    return mix32(mix32(inner) ^ _u(s1))


def keys(seed, hop, g, t):
    """The 64-bit keys of positions `t` of row `g`."""
    t = np.asarray(t, dtype=np.int64)
    d = draw32(seed[0], seed[1], (STREAM + hop) & 0xFFFFFFFF, np.full(t.shape, g, dtype=np.int64), t)
    return (d << np.uint64(32)) | t.astype(np.uint64)


def kept_positions(seed, hop, g, deg, k):
    """Ascending positions t in [0, deg) that row g keeps under fan-out k."""
    t = np.arange(deg, dtype=np.int64)
    if k < 0 or k >= deg:
        return t
    return np.sort(np.argsort(keys(seed, hop, g, t), kind="stable")[:k])


def csr_of(edge_index, n):
    """A target-grouped CSR (rowptr, col, perm) of an int64 [2, E] edge list; slots of a row in input order."""
    src, dst = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    perm = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[perm], perm


def sample_hop(rowptr, col, rows, k, seed, hop):
    """(out_rowptr [n_rows + 1], col [n_e], slot [n_e]) of one hop, as ops.sample_neighbors returns them."""
    out_ptr, cols, slots = [0], [], []
    for g in np.asarray(rows).tolist():
        b, deg = int(rowptr[g]), int(rowptr[g + 1] - rowptr[g])
        s = b + kept_positions(seed, hop, g, deg, k)
        slots.append(s)
        cols.append(np.asarray(col)[s])
        out_ptr.append(out_ptr[-1] + len(s))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
    return np.asarray(out_ptr, dtype=np.int64), cat(cols), cat(slots)


def sample_batch(rowptr, col, perm, seeds, fanouts, seed):
    """The whole batch: {'n_id', 'edge_index' [2, E_b] local ids, 'e_id', 'hop_of_edge', 'segments'} — hop h samples the
    in-edges of the nodes that entered at hop h - 1; a hop's new nodes are appended in ascending global id."""
    seeds = np.asarray(seeds, dtype=np.int64)
    n_id = list(seeds.tolist())
    local = {g: i for i, g in enumerate(n_id)}
    rows, first_row = seeds, 0
    src, dst, e_id, hops, segments = [], [], [], [], [len(n_id)]
    for hop, k in enumerate(fanouts):
        if len(rows) == 0:
            break
        ptr, c, s = sample_hop(rowptr, col, rows, k, seed, hop)
        new = sorted(set(c.tolist()) - set(local))
        n0 = len(n_id)
        for g in new:
            local[g] = len(n_id)
            n_id.append(g)
        src.append(np.asarray([local[g] for g in c.tolist()], dtype=np.int64))
        dst.append(first_row + np.repeat(np.arange(len(rows), dtype=np.int64), np.diff(ptr)))
        e_id.append(np.asarray(perm)[s].astype(np.int64))
        hops.append(np.full(len(c), hop, dtype=np.int64))
        segments.append(len(n_id))
        rows, first_row = np.asarray(new, dtype=np.int64), n0
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return {"n_id": np.asarray(n_id, dtype=np.int64), "edge_index": np.stack([cat(src), cat(dst)]), "e_id": cat(e_id),
            "hop_of_edge": cat(hops), "segments": segments}


# ---- graphs ---------------------------------------------------------------------------------------------------------------

def degree_list():
    """In-degrees the one-hop cases need: 0, 1, k - 1, k, k + 1 for every fan-out k, 63 / 64 / 65, each row-length boundary
    of the selection scheme just below, at and just above (64 and 1024 = LONG_ROW_SLOTS), and one hub row."""
    degs = {0, 1, 63, 64, 65, HUB_SLOTS}
    for k in FANOUTS:
        if k > 0:
            degs.update((k - 1, k, k + 1))
    for b in (SHORT_ROW_SLOTS, WAVE_ROW_SLOTS):
        degs.update((b - 1, b, b + 1))
    return sorted(degs)


def degree_graph(n=3000, seed=11):
    """(edge_index int64 [2, E], n, {degree: node id}): one node per degree of degree_list() at scattered ids, the other
    nodes with 0..8 in-edges; every listed row of two or more slots starts with a duplicate edge and, from three slots
    on, holds a self-loop. The edge list is shuffled."""
    rng = np.random.default_rng(seed)
    degs = degree_list()
    ids = rng.permutation(n)[:len(degs)]
    node_of = {d: int(i) for d, i in zip(degs, ids)}
    deg = rng.integers(0, 9, size=n)
    for d, i in node_of.items():
        deg[i] = d
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, size=dst.size)
    start = np.concatenate([[0], np.cumsum(deg)])
    for d, i in node_of.items():
        if d >= 2:
            src[start[i] + 1] = src[start[i]]      # a duplicate edge
        if d >= 3:
            src[start[i] + 2] = i                  # a self-loop
    order = rng.permutation(dst.size)
    return np.stack([src[order], dst[order]]).astype(np.int64), n, node_of


def random_graph(n=2000, e=16000, seed=12):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, size=(2, e)).astype(np.int64), n


def powerlaw_graph(n=3000, e=30000, seed=13):
    """Targets drawn with weight 1 / (rank + 1): a few hub rows beyond 1024 slots, a tail of short rows."""
    rng = np.random.default_rng(seed)
    w = 1.0 / (np.arange(n) + 1.0)
    dst = rng.choice(n, size=e, p=w / w.sum())
    relabel = rng.permutation(n)
    src = rng.integers(0, n, size=e)
    return np.stack([src, relabel[dst]]).astype(np.int64), n


def uniformity_graph(rows=4000, deg=20):
    """4000 rows of degree 20 with ids 17 + 3 r (section 1 of the design): (edge_index, n, row ids)."""
    ids = 17 + 3 * np.arange(rows)
    n = int(ids[-1]) + 3
    dst = np.repeat(ids, deg)
    src = (dst * 7 + np.tile(np.arange(deg), rows) * 13) % n
    return np.stack([src, dst]).astype(np.int64), n, ids


UNIFORMITY_SEEDS = ((123, 456), (1, 2), (2 ** 31 - 2, 7))


def pick_counts(seed, hop, ids, deg, k):
    """How often each position t is kept over the rows `ids` of degree `deg` (vectorised), and whether any two keys of a
    row share their upper word."""
    t = np.tile(np.arange(deg, dtype=np.int64), len(ids))
    g = np.repeat(np.asarray(ids, dtype=np.int64), deg)
    d = draw32(seed[0], seed[1], (STREAM + hop) & 0xFFFFFFFF, g, t).reshape(len(ids), deg)
    key = (d << np.uint64(32)) | np.arange(deg, dtype=np.uint64)[None, :]
    kept = np.argsort(key, axis=1, kind="stable")[:, :k]
    counts = np.bincount(kept.reshape(-1), minlength=deg)
    shared = any(len(np.unique(row)) != deg for row in d)
    return counts, shared


def planted_partition(n=600, classes=4, f=16, p_in=0.03, p_out=0.002, seed=14):
    """(x float32 [n, f], y int64 [n], edge_index int64 [2, E]): dense blocks on the diagonal, class means in the features."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, size=n)
    same = y[:, None] == y[None, :]
    adj = rng.random((n, n)) < np.where(same, p_in, p_out)
    np.fill_diagonal(adj, False)
    adj |= adj.T
    src, dst = np.nonzero(adj)
    means = rng.normal(size=(classes, f))
    x = (0.5 * means[y] + rng.normal(size=(n, f))).astype(np.float32)
    return x, y.astype(np.int64), np.stack([src, dst]).astype(np.int64)
