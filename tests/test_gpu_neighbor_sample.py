"""Neighbour sampling on the device (csrc/sample.hip, ops.sample_neighbors, NeighborSampler, experiment(num_neighbors=...))
against the numpy restatement of tests/_neighbor_sample_ref.py, element by element.

Row-length boundaries of the selection scheme, each met just below, at and just above by a row of the degree graph:
  64   (ops.SAMPLE_SHORT_ROW_SLOTS)  up to here a group of 16 lanes selects a row from keys held in registers;
  1024 (ops.SAMPLE_WAVE_ROW_SLOTS = graph.LONG_ROW_SLOTS)  up to here one wave per row, one draw bit per round; beyond it a
       workgroup per row with an LDS histogram, eight draw bits per round (the hub row of 5000 slots goes there too).
The select runs over the draw's 32 bits only: a row's draws are distinct by construction (test_neighbor_sample_host.py:
test_the_draws_of_a_row_are_distinct), so there is no tie-breaking path to reach.
Rows with deg <= k are copies in each of the three kernels (fan-outs 64, 100 and -1 reach those paths)."""
import numpy as np
import pytest
import torch

import _neighbor_sample_ref as R
from _guarded_alloc import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class OnDevice:
    """A graph of the restatement on the device, with the CSR the kernels read copied back for the restatement."""

    def __init__(self, ei, n):
        from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
        self.ei_np, self.n = ei, n
        self.ei = torch.from_numpy(ei).to(DEV)
        self.graph = get_graph(self.ei, n, LOOPS_KEEP)
        csr = self.graph.fwd
        self.rowptr = csr.rowptr.cpu().numpy().astype(np.int64)
        self.col = csr.col[:csr.nnz].cpu().numpy().astype(np.int64)
        self.perm = csr.perm[:csr.nnz].cpu().numpy().astype(np.int64)
        assert (ei[0, self.perm] == self.col).all() and (np.diff(self.rowptr) == np.bincount(ei[1], minlength=n)).all()


@pytest.fixture(scope="module")
def degree_graph():
    ei, n, node_of = R.degree_graph()
    g = OnDevice(ei, n)
    g.node_of = node_of
    return g


@pytest.fixture(scope="module")
def structure_graphs():
    return {"random": OnDevice(*R.random_graph()), "powerlaw": OnDevice(*R.powerlaw_graph())}


def seed_words(a, b):
    return torch.tensor([a, b], dtype=torch.int32, device=DEV)


def one_hop(g, rows, k, seed, hop, monkeypatch):
    from rgb_experiment_amd import ops
    with guarded(monkeypatch) as guard:
        out = ops.sample_neighbors(g.graph, torch.as_tensor(rows, device=DEV), k, seed_words(*seed), hop)
        torch.cuda.synchronize()
        guard.check()
        assert guard.allocations >= 3
    return [t.cpu().numpy().astype(np.int64) for t in out]


def assert_hop_equal(got, want):
    for name, a, b in zip(("rowptr", "col", "slot"), got, want):
        assert a.shape == b.shape and (a == b).all(), (name, np.nonzero(a != b)[0][:8] if a.shape == b.shape else (a.shape, b.shape))


@pytest.mark.parametrize("k", R.FANOUTS)
def test_one_hop_equals_the_restatement(degree_graph, k, monkeypatch):
    g = degree_graph
    listed = np.array(sorted(g.node_of.values()))
    all_rows = np.random.default_rng(3).permutation(g.n)           # every row, shuffled: 3000 = 187 * 16 + 8
    for rows in (listed, all_rows, listed[:1], np.array([g.node_of[R.HUB_SLOTS]])):
        for hop in (0, 2):
            got = one_hop(g, rows, k, (123, 456), hop, monkeypatch)
            assert_hop_equal(got, R.sample_hop(g.rowptr, g.col, rows, k, (123, 456), hop))


def test_hops_differ_and_a_call_repeats_bit_for_bit(degree_graph, monkeypatch):
    g = degree_graph
    rows = np.array(sorted(g.node_of.values()))
    a = one_hop(g, rows, 5, (77, 88), 0, monkeypatch)
    b = one_hop(g, rows, 5, (77, 88), 1, monkeypatch)
    c = one_hop(g, rows, 5, (77, 88), 0, monkeypatch)
    d = one_hop(g, rows, 5, (78, 88), 0, monkeypatch)
    assert (a[0] == b[0]).all() and not (a[2] == b[2]).all() and not (a[2] == d[2]).all()
    for x, y in zip(a, c):
        assert (x == y).all()
    # the largest hop word still wraps into 32 bits
    e = one_hop(g, rows, 5, (77, 88), 2 ** 31 - 1, monkeypatch)
    assert_hop_equal(e, R.sample_hop(g.rowptr, g.col, rows, 5, (77, 88), 2 ** 31 - 1))


def test_a_graph_without_edges_and_refused_arguments(monkeypatch):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    g = OnDevice(np.zeros((2, 0), dtype=np.int64), 10)
    for k in (1, 5, -1):
        rowptr, col, slot = one_hop(g, np.arange(10), k, (1, 2), 0, monkeypatch)
        assert (rowptr == 0).all() and rowptr.shape == (11,) and col.size == 0 and slot.size == 0
    rowptr, col, slot = one_hop(g, np.zeros(0, dtype=np.int64), 3, (1, 2), 0, monkeypatch)
    assert rowptr.tolist() == [0] and col.size == 0
    rows = torch.arange(10, device=DEV)
    for bad in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="fan-out"):
            ops.sample_neighbors(g.graph, rows, bad, seed_words(1, 2), 0)
    with pytest.raises(ValueError, match="hop"):
        ops.sample_neighbors(g.graph, rows, 2, seed_words(1, 2), -1)
    with pytest.raises(ValueError, match="outside"):
        ops.sample_neighbors(g.graph, rows + 1, 2, seed_words(1, 2), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_neighbors(g.graph, rows.cpu(), 2, seed_words(1, 2), 0)
    with pytest.raises(ValueError, match="LOOPS_KEEP"):
        ops.sample_neighbors(get_graph(g.ei, 10, LOOPS_ADD_REMAINING), rows, 2, seed_words(1, 2), 0)


def test_uniformity_case_equals_the_restatement(monkeypatch):
    """Section 1's 4000 rows of degree 20, k = 5, three seeds, hops 0..2: the device's picks ARE the restatement's (whose
    uniformity tests/test_neighbor_sample_host.py asserts), so the pick counts are within 5 sigma too."""
    ei, n, ids = R.uniformity_graph()
    g = OnDevice(ei, n)
    sigma = np.sqrt(4000 * 0.25 * 0.75)
    for seed in R.UNIFORMITY_SEEDS:
        for hop in range(3):
            rowptr, col, slot = one_hop(g, ids, 5, seed, hop, monkeypatch)
            t = np.tile(np.arange(20, dtype=np.int64), len(ids))
            d = R.draw32(seed[0], seed[1], (R.STREAM + hop) & 0xFFFFFFFF, np.repeat(ids, 20), t).reshape(len(ids), 20)
            key = (d << np.uint64(32)) | np.arange(20, dtype=np.uint64)[None, :]
            kept = np.sort(np.argsort(key, axis=1, kind="stable")[:, :5], axis=1)
            want_slot = (g.rowptr[ids][:, None] + kept).reshape(-1)
            assert (rowptr == 5 * np.arange(len(ids) + 1)).all()
            assert (slot == want_slot).all() and (col == g.col[want_slot]).all()
            counts = np.bincount(slot - np.repeat(g.rowptr[ids], 5), minlength=20)
            assert np.abs(counts - 1000).max() <= 5 * sigma


@pytest.mark.parametrize("which", ["random", "powerlaw"])
@pytest.mark.parametrize("fanouts", [[3, 2], [5, 5, 5], [-1, -1]], ids=str)
def test_batch_structure(structure_graphs, which, fanouts, monkeypatch):
    from rgb_experiment_amd import NeighborSampler
    g = structure_graphs[which]
    seeds = np.random.default_rng(21).permutation(g.n)[:50]
    hub = int(np.argmax(np.diff(g.rowptr)))
    if hub not in seeds:
        seeds[7] = hub
    with guarded(monkeypatch) as guard:
        sampler = NeighborSampler(g.ei, g.n, fanouts)
        batch = sampler.sample(torch.from_numpy(seeds).to(DEV), seed=(9, 10))
        again = sampler.sample(torch.from_numpy(seeds).to(DEV), seed=seed_words(9, 10))
        torch.cuda.synchronize()
        guard.check()
    assert bool((sampler.local_of == -1).all()) and sampler.local_of.numel() == g.n
    n_id, eb, e_id = (t.cpu().numpy() for t in (batch.n_id, batch.edge_index, batch.e_id))
    assert batch.n_id.dtype == batch.edge_index.dtype == batch.e_id.dtype == torch.int64 and batch.num_seeds == 50
    for a, b in ((batch.n_id, again.n_id), (batch.edge_index, again.edge_index), (batch.e_id, again.e_id)):
        assert torch.equal(a, b)
    want = R.sample_batch(g.rowptr, g.col, g.perm, seeds, fanouts, (9, 10))
    assert (n_id[:50] == seeds).all() and len(np.unique(n_id)) == len(n_id)
    assert n_id.shape == want["n_id"].shape and (n_id == want["n_id"]).all()
    for lo, hi in zip(want["segments"][:-1], want["segments"][1:]):
        assert (np.diff(n_id[lo:hi]) > 0).all()                                # a hop's new nodes ascend
    assert eb.shape == want["edge_index"].shape and eb.shape[1] > 0 and eb.min() >= 0 and eb.max() < len(n_id)
    assert (n_id[eb[0]] == g.ei_np[0, e_id]).all() and (n_id[eb[1]] == g.ei_np[1, e_id]).all()
    assert (eb == want["edge_index"]).all() and (e_id == want["e_id"]).all()
    hop_of = {}
    for t, h in zip(eb[1].tolist(), want["hop_of_edge"].tolist()):
        assert hop_of.setdefault(t, h) == h                                     # a target's in-edges come from one hop


def test_seed_checks_and_the_generator_seed():
    from rgb_experiment_amd import NeighborSampler
    ei, n = R.random_graph()
    ei_d = torch.from_numpy(ei).to(DEV)
    sampler = NeighborSampler(ei_d, n, [4, 4])
    ok = torch.tensor([5, 9, 2], device=DEV)
    with pytest.raises(ValueError, match="distinct"):
        sampler.sample(torch.tensor([5, 9, 5], device=DEV))
    with pytest.raises(ValueError, match="outside"):
        sampler.sample(torch.tensor([5, n], device=DEV))
    with pytest.raises(ValueError, match="outside"):
        sampler.sample(torch.tensor([-1, 3], device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sampler.sample(ok.cpu())
    with pytest.raises(ValueError, match="seed"):
        sampler.sample(ok, seed=(1, 2, 3))
    assert bool((sampler.local_of == -1).all())
    torch.cuda.manual_seed(5)
    a = sampler.sample(ok)
    b = sampler.sample(ok)
    torch.cuda.manual_seed(5)
    c = sampler.sample(ok)
    assert torch.equal(a.edge_index, c.edge_index) and torch.equal(a.n_id, c.n_id) and torch.equal(a.e_id, c.e_id)
    assert a.e_id.shape != b.e_id.shape or not torch.equal(a.e_id, b.e_id)     # the generator moved on
    u = sampler.sample_unchecked(ok, seed=(4, 5))
    v = sampler.sample(ok, seed=(4, 5))
    assert torch.equal(u.edge_index, v.edge_index) and torch.equal(u.n_id, v.n_id) and torch.equal(u.e_id, v.e_id)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sampler.sample_unchecked(ok.cpu())
    empty = sampler.sample(torch.zeros(0, dtype=torch.int64, device=DEV))
    assert empty.n_id.numel() == 0 and tuple(empty.edge_index.shape) == (2, 0) and empty.num_seeds == 0


# ---- exactness on the seeds ---------------------------------------------------------------------------------------------

class TwoLayer(torch.nn.Module):
    def __init__(self, a, b):
        super().__init__()
        self.a, self.b = a, b

    def forward(self, x, edge_index):
        return self.b(torch.relu(self.a(x, edge_index)), edge_index)


def make_stack(kind):
    from rgb_experiment_amd.nn import GATConv, GINConv, Linear, SAGEConv
    torch.manual_seed(31)
    if kind == "sage":
        return TwoLayer(SAGEConv(12, 16), SAGEConv(16, 5, aggr="max"))
    if kind == "gat":
        return TwoLayer(GATConv(12, 8, heads=2), GATConv(16, 5, heads=1))
    mlp = lambda i, o: torch.nn.Sequential(Linear(i, o), torch.nn.ReLU(), Linear(o, o))
    return TwoLayer(GINConv(mlp(12, 16), train_eps=True), GINConv(mlp(16, 5), train_eps=True))


@pytest.fixture(scope="module")
def full_batch():
    from rgb_experiment_amd import NeighborSampler
    g = OnDevice(*R.powerlaw_graph(n=1500, e=12000, seed=41))
    seeds = torch.from_numpy(np.random.default_rng(42).permutation(g.n)[:40]).to(DEV)
    batch = NeighborSampler(g.ei, g.n, [-1, -1]).sample(seeds, seed=(3, 4))
    x = torch.randn(g.n, 12, generator=torch.Generator().manual_seed(43)).to(DEV)
    y = torch.randint(0, 5, (g.n,), generator=torch.Generator().manual_seed(44)).to(DEV)
    return g, seeds, batch, x, y


@pytest.mark.parametrize("kind", ["sage", "gat", "gin"])
def test_full_fanout_batches_are_exact_on_the_seeds(full_batch, kind):
    """[-1, -1] under a two-layer stack: every seed sees its whole two-hop neighbourhood, and these layers normalise by the
    target only. Forward tolerance 1e-4 * max(1, |ref|max); SAGE parameter gradients 2e-4 * max(1, |ref|max)."""
    g, seeds, batch, x, y = full_batch
    net = make_stack(kind).to(DEV).eval()
    ref = net(x, g.ei)[seeds]
    ref_loss = torch.nn.functional.cross_entropy(ref, y[seeds])
    ref_grads = torch.autograd.grad(ref_loss, list(net.parameters())) if kind == "sage" else None
    ref = ref.detach()
    out = net(x[batch.n_id].contiguous(), batch.edge_index)[:batch.num_seeds]
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    err = float((out.detach() - ref).abs().max())
    print(f"{kind}: seed logits max|diff| = {err:.3e} (tolerance {tol:.3e})")
    assert torch.isfinite(ref).all() and err <= tol
    if kind == "sage":
        loss = torch.nn.functional.cross_entropy(out, y[batch.n_id[:batch.num_seeds]])
        grads = torch.autograd.grad(loss, list(net.parameters()))
        for (name, _), a, b in zip(net.named_parameters(), grads, ref_grads):
            gtol = 2e-4 * max(1.0, float(b.abs().max()))
            gerr = float((a - b).abs().max())
            print(f"sage: d{name} max|diff| = {gerr:.3e} (tolerance {gtol:.3e})")
            assert gerr <= gtol, name


# ---- experiment() ---------------------------------------------------------------------------------------------------------

def _experiment(**kw):
    from rgb_experiment_amd import experiment
    from rgb_experiment_amd.data import Data
    x, y, ei = R.planted_partition()
    data = Data(x=torch.from_numpy(x), y=torch.from_numpy(y), edge_index=torch.from_numpy(ei))
    args = dict(specify_data=True, data=data, remake_data_mask=True, model_name="graphsage2", epoch=6, learning_rate=0.01,
                implement_early_stopping=False, need_to_reappear=True, return_model=True, print_print=False)
    args.update(kw)
    return experiment(dict(num_layers=2, hidden_unit=32, dropout_rate=0.5), **args)


METRICS = ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro")


def test_experiment_trains_on_sampled_batches_reproducibly():
    from rgb_experiment_amd import graph
    graph.clear_cache()
    a = _experiment(num_neighbors=[5, 5], batch_size=64)
    assert len(graph._CACHE) <= 4            # the batches' graphs (6 epochs x 6 batches) did not stay behind
    b = _experiment(num_neighbors=[5, 5], batch_size=64)
    hist = a["history"]
    print("train_loss per epoch:", hist["train_loss"], "ACC", a["ACC"])
    assert all(np.isfinite(a[k]) for k in METRICS)
    assert all(len(v) == 6 and np.isfinite(v).all() for v in hist.values())
    assert hist["train_loss"][-1] < hist["train_loss"][0]
    assert a["used_hip_graph"] is False
    assert {k: a[k] for k in METRICS} == {k: b[k] for k in METRICS} and hist == b["history"]
    assert not getattr(a["model"], "cache_input_aggregate", False)


def test_sgc_runs_on_batches_only_without_its_cache():
    """SGConv(cached=True) keeps the first call's propagated rows: refused on this route. With cached=False every batch
    and the full-graph evaluation propagate their own rows, and the run equals its repetition."""
    from rgb_experiment_amd import experiment
    from rgb_experiment_amd.data import Data
    x, y, ei = R.planted_partition()

    def run(init):
        data = Data(x=torch.from_numpy(x), y=torch.from_numpy(y), edge_index=torch.from_numpy(ei))
        return experiment(init, specify_data=True, data=data, remake_data_mask=True, model_name="sgc", epoch=6,
                          learning_rate=0.01, implement_early_stopping=False, need_to_reappear=True, return_model=True,
                          print_print=False, num_neighbors=[5, 5], batch_size=64)

    with pytest.raises(ValueError, match="cached=True"):
        run(dict(K=2))
    a, b = run(dict(K=2, cached=False)), run(dict(K=2, cached=False))
    assert a["model"].conv1._cached_x is None and tuple(a["emb"].shape) == (600, 4)
    assert all(np.isfinite(v).all() for v in a["history"].values()) and a["history"] == b["history"]
    assert a["history"]["train_loss"][-1] < a["history"]["train_loss"][0]

def test_experiment_without_the_keyword_is_the_full_batch_route():
    a = _experiment()
    b = _experiment(num_neighbors=None)
    assert {k: a[k] for k in METRICS} == {k: b[k] for k in METRICS} and a["history"] == b["history"]
    assert torch.equal(a["emb"], b["emb"])
    c = _experiment(num_neighbors=[5, 5], batch_size=64)
    assert c["history"]["train_loss"] != a["history"]["train_loss"]
