#!/usr/bin/env python3
"""A/B of two builds of librgbx_hip.so on the benchmark graph: the same op closures run interleaved through build A
(the in-tree library) and build B (a variant built elsewhere, e.g. scratch/<name>/librgbx_hip.so), HIP events.
After the warm-up every case runs once through each build under the same torch seed and its output and gradients are
compared with torch.equal (value equality: -0 equals +0, a NaN equals nothing); a tensor that differs, or that only
one build returns, makes the exit status non-zero.
The layer cases set train() / eval() and drop the old gradients inside the timed closure (the comparison needs fresh
gradients). The gat / gcn / sage cases did neither before the comparison was added, so their times are not those of
A/B outputs recorded earlier.
Usage: python tools/ab_lib.py <path to build B> [S|L] [rounds] [ops: gat,gcn,sage,spmm,gatv2,transformer,supergat,
fagcn,resgated,gine,cgconv,film,rgcn,gmm,genconv,...] [--a=<path to build A>] [--split=<slots>]
(--a binds another build than the in-tree one as A, e.g. B again for the A/A spread; --split cuts rows longer than
<slots> into hub-row chunks (graph.LONG_ROW_SLOTS), so that the chunk and combine kernels run on a graph whose longest
row is below the default 1024)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import WORKLOADS, synth
from rgb_experiment_amd import _lib, graph as rgraph, nn as RN, ops
from rgb_experiment_amd.graph import get_graph


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    path_a = next((a[4:] for a in sys.argv[1:] if a.startswith("--a=")), None)
    split = next((int(a[8:]) for a in sys.argv[1:] if a.startswith("--split=")), None)
    if split is not None:  # before any graph is built: the plan is made with the graph
        rgraph.LONG_ROW_SLOTS = split
    path_b = argv[0]
    wl = WORKLOADS[argv[1] if len(argv) > 1 else "L"]
    rounds = int(argv[2]) if len(argv) > 2 else 4
    which = (argv[3] if len(argv) > 3 else "gat,gcn").split(",")
    N, E, d = wl["N"], wl["E"], wl["d"]
    dev = torch.device("cuda:0")
    ei, x, _ = synth(N, E, d)
    ei, x = ei.to(dev), x.to(dev)
    gy = torch.randn_like(x)
    if split is not None:  # how many rows of the forward and of the transposed CSR the plan cuts (0: no chunk kernel runs)
        deg_in, deg_out = torch.bincount(ei[1], minlength=N), torch.bincount(ei[0], minlength=N)
        print(f"--split={split}: longest row {int(deg_in.max())} in / {int(deg_out.max())} out; rows cut into chunks "
              f"{int((deg_in > split).sum())} in / {int((deg_out > split).sum())} out", flush=True)
    lib_a = _lib.bind(path_a, strict=False) if path_a else _lib.load()
    lib_b = _lib.bind(path_b, strict=False)
    cases = {}

    def add_layer(label, conv, call, aux_loss=None, inp=None):
        """An inference forward and a train forward + backward of a layer on `inp` (x where None); each returns what
        the bit comparison checks: the output, and after the backward the gradient of the input and of every
        parameter."""
        inp = x if inp is None else inp
        h = inp.clone().requires_grad_(True)
        leaves = [h] + list(conv.parameters())

        def infer():
            conv.eval()
            with torch.no_grad():
                return (call(conv, inp),)

        def train():
            conv.train()
            for t in leaves:
                t.grad = None
            out = call(conv, h)
            heads, grads = [out], [gy[:, :out.size(1)]]
            if aux_loss is not None:
                heads.append(aux_loss(conv))
                grads.append(None)
            torch.autograd.backward(heads, grads)
            return (out.detach(), *[t.grad for t in leaves if t.grad is not None])
        cases[f"{label} inference forward"] = infer
        cases[f"{label} train forward+backward"] = train

    for H, C in ((8, 16), (1, 128)):
        torch.manual_seed(0)
        kw = dict(heads=H, concat=H > 1)
        if "gat" in which:
            add_layer(f"gat H={H} C={C}", RN.GATConv(d, C, H, concat=H > 1).to(dev), lambda conv, h: conv(h, ei))
        if "gatv2" in which:
            add_layer(f"gatv2 H={H} C={C}", RN.GATv2Conv(d, C, dropout=0.6, **kw).to(dev), lambda conv, h: conv(h, ei))
        if "transformer" in which:
            add_layer(f"transformer H={H} C={C}", RN.TransformerConv(d, C, dropout=0.6, **kw).to(dev),
                      lambda conv, h: conv(h, ei))
        if "supergat" in which:
            # neg_sample_ratio=0: the negative pairs' row gradients are added with float atomics, the one sum of the
            # layer whose order no build fixes; the positive half of the attention loss stays in
            add_layer(f"supergat H={H} C={C}",
                      RN.SuperGATConv(d, C, dropout=0.6, edge_sample_ratio=0.8, neg_sample_ratio=0.0, **kw).to(dev),
                      lambda conv, h: conv(h, ei), aux_loss=lambda conv: conv.get_attention_loss())
    torch.manual_seed(0)
    if "fagcn" in which:
        add_layer(f"fagcn C={d}", RN.FAConv(d, eps=0.1, dropout=0.5).to(dev), lambda conv, h: conv(h, x, ei))
    if "gcn" in which:
        add_layer("gcn", RN.GCNConv(d, d).to(dev), lambda conv, h: conv(h, ei))
    if "sage" in which:
        add_layer("sage", RN.SAGEConv(d, d).to(dev), lambda conv, h: conv(h, ei))
    # the edge-message families (csrc/edge_common.h). Those with a feature row per edge run 32 channels wide: at L a
    # 128-wide row per edge is 31 GB, and as much again for its gradient.
    gen = torch.Generator().manual_seed(7)
    xn = x[:, :32].contiguous()
    if "resgated" in which:
        add_layer(f"resgated C={d}", RN.ResGatedGraphConv(d, d).to(dev), lambda conv, h: conv(h, ei))
    if "gine" in which:
        ea = torch.randn(E, 4, generator=gen).to(dev)
        add_layer("gine C=32 D=4", RN.GINEConv(torch.nn.Linear(32, 32), train_eps=True, edge_dim=4).to(dev),
                  lambda conv, h: conv(h, ei, ea), inp=xn)
    if "cgconv" in which:
        ec = torch.randn(E, 4, generator=gen).to(dev)
        add_layer("cgconv C=32 D=4", RN.CGConv(32, dim=4, aggr="mean").to(dev), lambda conv, h: conv(h, ei, ec), inp=xn)
    if "film" in which or "rgcn" in which:
        et = torch.randint(0, 4, (E,), generator=gen).to(dev)
    if "film" in which:
        add_layer(f"film R=4 C={d}", RN.FiLMConv(d, d, num_relations=4).to(dev), lambda conv, h: conv(h, ei, et))
    if "rgcn" in which:
        add_layer(f"rgcn R=4 B=2 C={d}", RN.RGCNConv(d, d, 4, num_bases=2).to(dev), lambda conv, h: conv(h, ei, et))
    if "gmm" in which:
        eu = torch.rand(E, 2, generator=gen).to(dev)
        add_layer("gmm K=4 D=2 C=32", RN.GMMConv(d, 32, dim=2, kernel_size=4).to(dev), lambda conv, h: conv(h, ei, eu))
    if "genconv" in which:
        add_layer(f"genconv C={d}", RN.GENConv(d, d, learn_t=True).to(dev), lambda conv, h: conv(h, ei))
    if "spmm" in which:
        g = get_graph(ei, N, 1)
        out = torch.empty_like(x)

        def spmm():
            ops.spmm_raw(g.fwd, g.w, None, x, out=out)
            return (out,)
        cases["gcn spmm"] = spmm
    if "appnp" in which:  # the K-loop: every step gathers the table the previous step wrote
        g = get_graph(ei, N, 1)
        cases["appnp K=10 forward"] = lambda: ops.appnp_raw(g.fwd, g.w, x, 10, 0.1)
    res = {k: {"A": [], "B": []} for k in cases}
    for tag, lib in (("A", lib_a), ("B", lib_b)):  # warm-up both (graph build, allocator)
        _lib.use(lib)
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    mismatches = 0
    for k, fn in cases.items():  # bit comparison: the same seed in front of each run, so the dropout seeds agree
        got = {}
        for tag, lib in (("A", lib_a), ("B", lib_b)):
            _lib.use(lib)
            torch.manual_seed(1234)
            r = fn()
            got[tag] = [t.clone() for t in ((r,) if torch.is_tensor(r) else r or ()) if torch.is_tensor(t)]
        eq = [torch.equal(a, b) for a, b in zip(got["A"], got["B"])]
        eq += [False] * abs(len(got["A"]) - len(got["B"]))  # a tensor only one build returned
        ok = bool(eq) and all(eq)  # a case that returns nothing was not compared
        mismatches += eq.count(False) + (not eq)
        print(f"{k:42s} torch.equal A/B: {'yes' if ok else 'NO'}  ({len(eq)} tensors: "
              f"{' '.join('=' if e else 'X' for e in eq)})", flush=True)
        del got
    pairs = (("A", lib_a), ("B", lib_b))
    for r in range(rounds):  # swap the order every round, so that neither build is always the one that runs second
        for k, fn in cases.items():
            for tag, lib in (pairs if r % 2 == 0 else pairs[::-1]):
                _lib.use(lib)
                res[k][tag].append(timed(fn, 5))
    _lib.use(lib_a)
    for k, r in res.items():
        a, b = sorted(r["A"])[len(r["A"]) // 2], sorted(r["B"])[len(r["B"]) // 2]
        print(f"{k:42s} A {a:8.3f} ms   B {b:8.3f} ms   B/A {b / a:6.3f}", flush=True)
    if mismatches:
        sys.exit(f"{mismatches} tensors differ between build A and build B")


if __name__ == "__main__":
    main()
