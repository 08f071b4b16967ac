"""Neighbour sampling, the host side: the numpy restatement of the draw (tests/_neighbor_sample_ref.py) checked against its
own definition, the graphs the GPU file (test_gpu_neighbor_sample.py) runs on, the argument errors of the new C entry
points and the refusals of experiment(num_neighbors=...). No GPU needed."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _neighbor_sample_ref as R


def test_mix32_and_draw32_restate_the_header():
    """Against the C arithmetic written out for single values with Python ints."""
    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16

    def draw(s0, s1, stream, a, b):
        return mix(mix((mix(a ^ s0) + b * 0x9E3779B9 + stream) & 0xFFFFFFFF) ^ s1)

    rng = np.random.default_rng(0)
    vals = rng.integers(0, 2 ** 32, size=(50, 5)).tolist() + [[0] * 5, [2 ** 32 - 1] * 5]
    for s0, s1, stream, a, b in vals:
        assert int(R.mix32(np.array([a]))[0]) == mix(a)
        assert int(R.draw32(s0, s1, stream, np.array([a]), np.array([b]))[0]) == draw(s0, s1, stream, a, b)
    assert mix(0) == 0 and mix(1) != 1
    # a seed word given as a negative int32 is the same 32 bits
    assert int(R.draw32(-5, 7, 3, np.array([9]), np.array([4]))[0]) == draw(2 ** 32 - 5, 7, 3, 9, 4)
    assert R.STREAM == 0x082EFA98


def test_the_graphs_have_what_the_gpu_cases_rely_on():
    ei, n, node_of = R.degree_graph()
    rowptr, col, perm = R.csr_of(ei, n)
    deg = np.diff(rowptr)
    want = {0, 1, 2, 3, 4, 5, 6, 63, 64, 65, 99, 100, 101, 1023, 1024, 1025, R.HUB_SLOTS}
    assert set(R.degree_list()) == want and set(node_of) == want
    assert R.SHORT_ROW_SLOTS == 64 and R.WAVE_ROW_SLOTS == 1024
    assert len(set(node_of.values())) == len(node_of)
    for d, i in node_of.items():
        assert deg[i] == d
        row = col[rowptr[i]:rowptr[i + 1]]
        if d >= 2:
            assert len(set(row.tolist())) < d          # a duplicate edge: separate slots
        if d >= 3:
            assert i in row                             # a self-loop
    assert (ei[:, perm][1] == np.repeat(np.arange(n), deg)).all() and (ei[0, perm] == col).all()
    assert n % 16 != 0 and len(node_of) % 16 != 0       # n_rows that are no multiple of the group count

    ei, n = R.random_graph()
    deg = np.bincount(ei[1], minlength=n)
    assert 5 < deg.max() <= 64                          # every row in the short-row kernel

    ei, n = R.powerlaw_graph()
    deg = np.bincount(ei[1], minlength=n)
    assert deg.max() > R.WAVE_ROW_SLOTS and ((deg > 64) & (deg <= 1024)).sum() >= 3 and (deg == 0).sum() > 0

    ei, n, ids = R.uniformity_graph()
    deg = np.bincount(ei[1], minlength=n)
    assert len(ids) == 4000 and (deg[ids] == 20).all() and deg.sum() == 80000 and ids[0] == 17 and ids[1] == 20

    x, y, ei = R.planted_partition()
    assert x.shape == (600, 16) and len(set(y.tolist())) == 4 and 3000 < ei.shape[1] < 12000
    same = (y[ei[0]] == y[ei[1]]).mean()
    assert same > 0.7


def test_the_draws_of_a_row_are_distinct():
    """mix32 is a bijection and the row position enters draw32 as an odd multiple, so two slots of a row never share
    their draw: the kernels select on the upper word of the key alone. Checked on rows of every length class."""
    for deg in (64, 1024, R.HUB_SLOTS, 70000):
        t = np.arange(deg, dtype=np.int64)
        for seed in R.UNIFORMITY_SEEDS:
            for hop, g in ((0, 17), (2, 2999), (2 ** 31 - 1, 0)):
                d = R.draw32(seed[0], seed[1], (R.STREAM + hop) & 0xFFFFFFFF, np.full(deg, g, dtype=np.int64), t)
                assert len(np.unique(d)) == deg
    x = np.arange(1 << 16, dtype=np.int64) * 65537 % (1 << 32)
    assert len(np.unique(R.mix32(x))) == len(x)


def test_uniformity_of_the_draw():
    """Section 1's check: 4000 rows of degree 20, k = 5, three seeds, hops 0..2 — every position's pick count within
    5 sigma of 1000 (sigma = sqrt(4000 * 0.25 * 0.75) = 27.4), and no two keys of a row share their upper word."""
    _, _, ids = R.uniformity_graph()
    sigma = np.sqrt(4000 * 0.25 * 0.75)
    for seed in R.UNIFORMITY_SEEDS:
        for hop in range(3):
            counts, shared = R.pick_counts(seed, hop, ids, 20, 5)
            assert counts.sum() == 4000 * 5
            assert np.abs(counts - 1000).max() <= 5 * sigma, (seed, hop, counts)
            assert not shared


@pytest.mark.parametrize("k", R.FANOUTS)
def test_kept_sets_are_the_smallest_keys_in_slot_order(k):
    ei, n, node_of = R.degree_graph()
    rowptr, col, _ = R.csr_of(ei, n)
    rows = np.array(sorted(node_of.values()) + [0, 1, 2])
    rows = rows[np.sort(np.unique(rows, return_index=True)[1])]
    seed = (123, 456)
    ptr, c, s = R.sample_hop(rowptr, col, rows, k, seed, hop=1)
    deg = rowptr[rows + 1] - rowptr[rows]
    assert (np.diff(ptr) == (deg if k < 0 else np.minimum(deg, k))).all()
    for r, g in enumerate(rows.tolist()):
        kept = s[ptr[r]:ptr[r + 1]] - rowptr[g]
        assert (np.diff(kept) > 0).all()                                     # ascending slots, no repeats
        assert (c[ptr[r]:ptr[r + 1]] == col[rowptr[g] + kept]).all()
        key = R.keys(seed, 1, g, np.arange(deg[r]))
        assert len(np.unique(key)) == deg[r]
        if k < 0 or k >= deg[r]:
            assert (kept == np.arange(deg[r])).all()                         # the CSR row as it stands
        else:
            rest = np.setdiff1d(np.arange(deg[r]), kept)
            assert key[kept].max() < key[rest].min()                          # exactly the k smallest keys


def test_hops_differ_and_batches_are_consistent():
    ei, n = R.powerlaw_graph()
    rowptr, col, perm = R.csr_of(ei, n)
    rows = np.arange(0, n, 7)
    a = R.sample_hop(rowptr, col, rows, 3, (5, 6), 0)
    b = R.sample_hop(rowptr, col, rows, 3, (5, 6), 1)
    assert (a[0] == b[0]).all() and not (a[2] == b[2]).all()
    seeds = np.array([5, 900, 17, 2048, 3])
    for fanouts in ([3, 2], [5, 5, 5], [-1, -1]):
        batch = R.sample_batch(rowptr, col, perm, seeds, fanouts, (9, 10))
        n_id, eb, e_id = batch["n_id"], batch["edge_index"], batch["e_id"]
        assert (n_id[:5] == seeds).all() and len(set(n_id.tolist())) == len(n_id)
        seg = batch["segments"]
        for lo, hi in zip(seg[:-1], seg[1:]):
            assert (np.diff(n_id[lo:hi]) > 0).all()
        assert eb.max() < len(n_id)
        assert (n_id[eb[0]] == ei[0, e_id]).all() and (n_id[eb[1]] == ei[1, e_id]).all()
        hops_of_target = {}
        for t, h in zip(eb[1].tolist(), batch["hop_of_edge"].tolist()):
            assert hops_of_target.setdefault(t, h) == h                       # in-edges from one hop only
    full = R.sample_batch(rowptr, col, perm, seeds, [-1, -1], (9, 10))
    deg = np.diff(rowptr)
    first = full["n_id"][:full["segments"][1]]
    assert len(full["e_id"]) == deg[first].sum()


def test_argument_errors_of_the_sampling_entry_points():
    """Host-side validation only: every rejected call returns before a launch (fake, never dereferenced pointers)."""
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    p = 0x10000
    big = 2 ** 31
    n = ctypes.c_size_t(0)
    assert lib.rgbx_sample_workspace_bytes(-1, 4, 10, ctypes.byref(n)) == -1
    assert lib.rgbx_sample_workspace_bytes(4, 4, 10, None) == -1
    assert lib.rgbx_sample_workspace_bytes(big, 4, 10, ctypes.byref(n)) == -2
    assert lib.rgbx_sample_workspace_bytes(4, big, 10, ctypes.byref(n)) == -2
    count = lambda rowptr=p, rows=p, n_rows=5, k=5, out=p, ws=p: lib.rgbx_sample_count(
        rowptr, 10, rows, n_rows, k, out, None, ws, 1 << 20, None)
    assert count(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert count(rows=None) == -1 and count(out=None) == -1 and count(ws=None) == -1
    assert count(k=0) == -1 and b"fan-out" in lib.rgbx_last_error_string()
    assert count(k=-2) == -1 and count(k=-100) == -1
    assert count(n_rows=big) == -2 and count(n_rows=-1) == -1
    pick = lambda rowptr=p, col=p, rows=p, n_rows=5, k=5, seed=p, hop=0, out=p: lib.rgbx_sample_pick(
        rowptr, col, 10, rows, n_rows, k, seed, hop, p, out, out, 7, None)
    assert pick(rowptr=None) == -1 and pick(col=None) == -1 and pick(rows=None) == -1 and pick(seed=None) == -1
    assert pick(out=None) == -1 and pick(k=0) == -1 and pick(k=-2) == -1 and pick(hop=-1) == -1
    assert pick(n_rows=big) == -2
    assert pick(n_rows=0, rowptr=None) == 0                                    # nothing to do
    frontier = lambda cand=p, n_cand=5, local=p, first=0, new=p, cnt=p, ws=p: lib.rgbx_sample_frontier(
        cand, n_cand, local, 10, first, new, cnt, ws, 1 << 20, None)
    assert frontier(cand=None) == -1 and frontier(local=None) == -1 and frontier(new=None) == -1
    assert frontier(cnt=None) == -1 and frontier(ws=None) == -1 and frontier(first=-1) == -1
    assert frontier(n_cand=big) == -2
    assert lib.rgbx_sample_set_local(None, 5, 0, p, 10, None) == -1
    assert lib.rgbx_sample_set_local(p, 5, 0, None, 10, None) == -1
    assert lib.rgbx_sample_set_local(p, big, 0, p, 10, None) == -2
    assert lib.rgbx_sample_set_local(None, 0, 0, None, 10, None) == 0
    relabel = lambda ptr=p, n_rows=5, col=p, n_e=5, local=p, src=p: lib.rgbx_sample_relabel(
        ptr, n_rows, col, p, n_e, local, 10, p, 0, src, p, p, None)
    assert relabel(ptr=None) == -1 and relabel(col=None) == -1 and relabel(local=None) == -1 and relabel(src=None) == -1
    assert relabel(n_rows=0) == -1 and relabel(n_e=big) == -2 and relabel(n_e=0, ptr=None) == 0


def test_fanout_lists_and_the_python_surface():
    import rgb_experiment_amd as pkg
    from rgb_experiment_amd import ops, sampler
    assert pkg.NeighborSampler is sampler.NeighborSampler
    assert list(inspect.signature(ops.sample_neighbors).parameters) == ["graph", "rows", "fanout", "seed", "hop"]
    assert list(inspect.signature(sampler.NeighborSampler.__init__).parameters)[1:] == ["edge_index", "num_nodes",
                                                                                       "num_neighbors"]
    assert list(inspect.signature(sampler.NeighborSampler.sample).parameters)[1:] == ["seeds", "seed"]
    assert list(inspect.signature(sampler.NeighborSampler.sample_unchecked).parameters)[1:] == ["seeds", "seed"]
    assert sampler.check_num_neighbors([25, 10]) == [25, 10] and sampler.check_num_neighbors((-1,)) == [-1]
    for bad in ([], [0], [5, -2], [2.0], [True], "5", 5, None, [[5]]):
        with pytest.raises(ValueError):
            sampler.check_num_neighbors(bad)
    assert (ops.SAMPLE_STREAM, ops.SAMPLE_SHORT_ROW_SLOTS, ops.SAMPLE_WAVE_ROW_SLOTS) == (
        R.STREAM, R.SHORT_ROW_SLOTS, R.WAVE_ROW_SLOTS)
    from rgb_experiment_amd.graph import LONG_ROW_SLOTS
    assert ops.SAMPLE_WAVE_ROW_SLOTS == LONG_ROW_SLOTS
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback"):     # CPU tensors are refused
        sampler.NeighborSampler(ei, 3, [2])
    with pytest.raises(ValueError):
        sampler.NeighborSampler(ei, 3, [0])
    doc = sampler.__doc__ + inspect.getdoc(pkg.experiment)
    assert "gcn_norm" in doc and "outer ring" in doc and "as many hops as layers" in doc


def _data():
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    data = Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g), edge_weight=torch.rand(300, generator=g),
                edge_attr=torch.rand(300, 2, generator=g), edge_type=torch.randint(0, 2, (300,), generator=g))
    return data


def _run(model_name, init=None, **kw):
    from rgb_experiment_amd import experiment
    args = dict(specify_data=True, data=_data(), remake_data_mask=True, model_name=model_name, epoch=2, print_print=False)
    args.update(kw)
    return experiment(init or dict(num_layers=2, hidden_unit=8, dropout_rate=0.5), **args)


def test_experiment_refusals_and_defaults():
    sig = inspect.signature(__import__("rgb_experiment_amd").experiment).parameters
    assert sig["num_neighbors"].default is None and sig["batch_size"].default == 1024
    for bad in ([], [0], [3, -2], [1.5], "3", 3):
        with pytest.raises(ValueError, match="num_neighbors|fan-out"):
            _run("graphsage2", num_neighbors=bad)
    for bad in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="batch_size"):
            _run("graphsage2", num_neighbors=[3, 3], batch_size=bad)
    with pytest.raises(ValueError, match="PTA"):
        _run("pta", init=dict(K=2, alpha=0.1, hidden=8, dropout=0.5), num_neighbors=[3])
    with pytest.raises(ValueError, match="num_neighbors cannot be combined"):
        _run("gcn", num_neighbors=[3], use_edge_weight=True)
    with pytest.raises(ValueError, match="num_neighbors cannot be combined"):
        _run("gine", num_neighbors=[3], use_edge_attr=True)
    with pytest.raises(ValueError, match="num_neighbors cannot be combined"):
        _run("rgcn", num_neighbors=[3], use_edge_type=True)
    # a layer that keeps its first call's propagated features: SGC's default, and the same layer inside a caller's module
    with pytest.raises(ValueError, match="cached=True"):
        _run("sgc", init=dict(K=2), num_neighbors=[3])
    with pytest.raises(ValueError, match="cached=True"):
        _run("sgc", init=dict(K=2, cached=True), num_neighbors=[3])
    from rgb_experiment_amd.models import SGC
    with pytest.raises(ValueError, match="SGConv\\(cached=True\\)"):
        _run("gcn", model=SGC(8, 3, K=2), num_neighbors=[3])
    if not torch.cuda.is_available():  # cached=False passes the refusals (and then needs the device)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _run("sgc", init=dict(K=2, cached=False), num_neighbors=[3])
    with pytest.raises(NotImplementedError, match="partitioned"):
        _run("graphsage", num_neighbors=[3], distributed=True)
    # a bad batch_size without the keyword is not looked at: nothing changes on the full-batch route
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _run("graphsage2", batch_size=0)
