"""FAGCN on the host: a float64 restatement of FAConv / FAGCN checked against a brute-force dense evaluation, module
layout (PyG's parameter names, strict state_dict loading), defaults, refusals, the C ABI of the new entry points, and
experiment(model=<nn.Module>) on the CPU loop. No GPU needed."""
import copy
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rewritten_edges(ei, n):
    """Self-loops removed, one self-loop per node appended (add_remaining_self_loops with fill 1): (src, dst)."""
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


class RefFAConv(nn.Module):
    """float64 restatement of FAConv (normalize=True, add_self_loops=True), written from the layer's formulas; PyG's
    parameter names. The dropout decisions are an INPUT: `choices` = {'src', 'dst' (the edges after the self-loop
    rewrite, in the order the mask refers to), 'keep' bool [E']}; without it the edges are rewritten here and nothing
    is dropped. `deg` ([n], optional): in-degrees (self-loop included) to normalise with instead of those of the
    edges given — for a subgraph cut out of a larger graph."""

    def __init__(self, channels, eps=0.1, dropout=0.0):
        super().__init__()
        self.eps, self.p = eps, dropout
        self.att_l = nn.Linear(channels, 1, bias=False).double()
        self.att_r = nn.Linear(channels, 1, bias=False).double()

    def forward(self, x, x_0, ei, choices=None, deg=None):
        n = x.size(0)
        if choices is None:
            src, dst = rewritten_edges(ei, n)
            keep = torch.ones(src.numel(), dtype=torch.bool)
        else:
            src, dst, keep = choices["src"], choices["dst"], choices["keep"]
        if deg is None:
            deg = torch.zeros(n, dtype=torch.float64).index_add(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
        dis = deg.double().pow(-0.5)
        w = dis[src] * dis[dst]
        al, ar = self.att_l(x).view(-1), self.att_r(x).view(-1)
        a = torch.tanh(al[src] + ar[dst])
        k = keep.double() / (1.0 - self.p) if self.training and self.p > 0 else torch.ones_like(a)
        self.a = a
        out = torch.zeros_like(x).index_add(0, dst, (k * a * w).unsqueeze(-1) * x[src])
        return out + self.eps * x_0 if self.eps != 0.0 else out


class RefFAGCN(nn.Module):
    """reference models/fagcn.py in float64. The two feature dropouts are inputs: `masks` = (mask0 [N, F], mask1
    [N, hidden]) of 0 / 1 (None = no dropout), scaled by 1 / (1 - p) here; `choices` = one dict per layer."""

    def __init__(self, num_layers, input_dim, hidden_unit, output_dim, dropout_rate, epsilon):
        super().__init__()
        self.p = dropout_rate
        self.layers = nn.ModuleList(RefFAConv(hidden_unit, epsilon, dropout_rate) for _ in range(num_layers))
        self.t1 = nn.Linear(input_dim, hidden_unit).double()
        self.t2 = nn.Linear(hidden_unit, output_dim).double()

    def forward(self, x, ei, choices=None, masks=(None, None)):
        drop = lambda t, m: t if (m is None or not self.training) else t * m.double() / (1.0 - self.p)
        h = torch.relu(self.t1(drop(x, masks[0])))
        h = drop(h, masks[1])
        raw = h
        for i, layer in enumerate(self.layers):
            h = layer(h, raw, ei, None if choices is None else choices[i])
        h = self.t2(h)
        return {"out": F.log_softmax(h, dim=1), "emb": h}


def test_restatement_equals_a_dense_evaluation():
    """12 nodes; the edge list holds a duplicate edge (3 -> 5 twice), an existing self-loop (7 -> 7) and leaves node 11
    isolated. The dense form: M[i, j] = (number of edges j -> i after the rewrite) * tanh(al_j + ar_i) / sqrt(d_i d_j),
    out = M x + eps x0."""
    n, C = 12, 5
    g = torch.Generator().manual_seed(3)
    ei = torch.tensor([[0, 1, 2, 3, 3, 4, 5, 6, 7, 7, 8, 9, 10, 2, 6], [1, 2, 0, 5, 5, 3, 4, 0, 7, 8, 9, 10, 8, 9, 1]])
    assert int((ei[0] == ei[1]).sum()) == 1 and 11 not in ei.tolist()[0] + ei.tolist()[1]
    x = torch.randn(n, C, generator=g, dtype=torch.float64)
    x0 = torch.randn(n, C, generator=g, dtype=torch.float64)
    conv = RefFAConv(C, eps=0.3).eval()
    with torch.no_grad():
        conv.att_l.weight.copy_(torch.randn(1, C, generator=g, dtype=torch.float64))
        conv.att_r.weight.copy_(torch.randn(1, C, generator=g, dtype=torch.float64))
    got = conv(x, x0, ei)
    count = torch.zeros(n, n, dtype=torch.float64)  # count[i, j]: edges j -> i, self-loops dropped, then I added
    for s, d in ei.t().tolist():
        if s != d:
            count[d, s] += 1
    count += torch.eye(n, dtype=torch.float64)
    deg = count.sum(1)
    assert deg[11].item() == 1.0 and count[5, 3].item() == 2.0 and count[7, 7].item() == 1.0
    al = x @ conv.att_l.weight.view(-1)
    ar = x @ conv.att_r.weight.view(-1)
    M = count * torch.tanh(al.view(1, n) + ar.view(n, 1)) / torch.sqrt(deg.view(n, 1) * deg.view(1, n))
    want = M @ x + 0.3 * x0
    assert torch.allclose(got, want, atol=1e-13)
    # dropout: the mask enters as keep / (1 - p); dropping every slot leaves eps * x0
    conv.train()
    conv.p = 0.5
    src, dst = rewritten_edges(ei, n)
    none = conv(x, x0, ei, {"src": src, "dst": dst, "keep": torch.zeros(src.numel(), dtype=torch.bool)})
    assert torch.allclose(none, 0.3 * x0, atol=1e-15)
    every = conv(x, x0, ei, {"src": src, "dst": dst, "keep": torch.ones(src.numel(), dtype=torch.bool)})
    assert torch.allclose(every, 2 * (M @ x) + 0.3 * x0, atol=1e-13)
    conv.eps = 0.0
    assert torch.allclose(conv(x, x0, ei, {"src": src, "dst": dst, "keep": torch.ones(src.numel(), dtype=torch.bool)}),
                          2 * (M @ x), atol=1e-13)


def test_module_layout_init_and_strict_loading():
    from rgb_experiment_amd.models import FAGCN
    from rgb_experiment_amd.nn import FAConv
    model = FAGCN(2, 24, 8, 5, 0.5, 0.3)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == {"layers.0.att_l.weight": (1, 8), "layers.0.att_r.weight": (1, 8), "layers.1.att_l.weight": (1, 8),
                      "layers.1.att_r.weight": (1, 8), "t1.weight": (8, 24), "t1.bias": (8,), "t2.weight": (5, 8),
                      "t2.bias": (5,)}
    assert all(isinstance(layer, FAConv) and layer.eps == 0.3 and layer.dropout == 0.5 for layer in model.layers)
    ref = RefFAGCN(2, 24, 8, 5, 0.5, 0.3)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    for C in (4, 64):
        conv = FAConv(C)
        bound = 1.0 / C ** 0.5
        assert conv.att_l.weight.abs().max().item() <= bound and conv.att_r.weight.abs().max().item() <= bound
        assert conv.att_l.weight.abs().max().item() > 0 and conv.att_l.bias is None and conv.att_r.bias is None
    # xavier_normal_(gain=1.414): std = 1.414 * sqrt(2 / (fan_in + fan_out)); a 256 x 256 weight pins it within 3 %
    big = FAGCN(1, 256, 256, 256, 0.0, 0.1)
    for w in (big.t1.weight, big.t2.weight):
        assert abs(w.std().item() / (1.414 * (2.0 / 512) ** 0.5) - 1.0) < 0.03


def test_defaults_and_registry():
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.itexperiments import _OUT_OF_SCOPE
    from rgb_experiment_amd import models
    assert InitialParameters.defaults_for("FAGCN") == {"num_layers": 2, "hidden_unit": 64, "dropout_rate": 0.5,
                                                       "epsilon": 0.3}
    assert InitialParameters.model_names[12] == "FAGCN" and len(InitialParameters.model_names) == 13
    assert len(InitialParameters.default_init_params) == 13
    assert "fagcn" not in models.MODELS and "fagcn" not in models.REGISTRY and "fagcn" in _OUT_OF_SCOPE
    assert models.FAGCN.__name__ == "FAGCN"


def test_refusals():
    from rgb_experiment_amd.nn import FAConv
    with pytest.raises(NotImplementedError, match="normalize"):
        FAConv(4, normalize=False)
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        FAConv(4, add_self_loops=False)
    conv = FAConv(4)
    x = torch.randn(5, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback"):
        conv(x, x, torch.tensor([[0, 1], [1, 2]]))


NEW_ENTRIES = ("rgbx_faconv_supported", "rgbx_faconv_scores_f32", "rgbx_faconv_fwd_f32", "rgbx_faconv_bwd_dst_f32",
               "rgbx_faconv_bwd_src_f32", "rgbx_faconv_edge_coef_f32", "rgbx_faconv_edge_dot_f32", "rgbx_faconv_draws_u8")


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbx_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert text.rstrip().endswith("#endif") and text.index("rgbx_faconv_supported") > text.index("rgbx_paced_copy_f32")
    assert lib.rgbx_version() == 501  # unchanged


def test_faconv_entry_points_validate_on_the_host():
    """Every rejected call returns before a launch (fake, never dereferenced pointers)."""
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    p = 0x10000  # 16-byte aligned, non-null
    ok = lib.rgbx_faconv_supported
    assert all(ok(C) for C in (1, 4, 7, 8, 16, 40, 63, 64, 66, 128, 132, 256))
    assert not any(ok(C) for C in (0, -4, 65, 67, 127, 130, 258, 260, 512))
    E_ARG, E_ALIGN, E_SHAPE = -1, -3, -5

    def scores(x=p, ldx=64, N=10, C=64, alr=p):
        return lib.rgbx_faconv_scores_f32(x, ldx, p, p, alr, N, C, None)
    assert scores(x=None) == E_ARG and b"null" in lib.rgbx_last_error_string()
    assert scores(N=-1) == E_ARG and scores(C=0) == E_ARG
    assert scores(ldx=66) == E_ALIGN and scores(x=p + 4) == E_ALIGN and scores(alr=p + 4) == E_ALIGN
    assert scores(ldx=32) == E_ARG                                    # leading dimension < C
    assert scores(N=0) == 0                                           # nothing to do: no launch

    def fwd(rowptr=p, x=p, ldx=64, N=10, C=64, out=p + 4096, ldo=64, x0=None, ld0=0, seed=None, p_drop=0.0):
        return lib.rgbx_faconv_fwd_f32(rowptr, p, p, x, ldx, p, x0, ld0, 0.3, out, ldo, N, C, seed, p_drop, None, None)
    assert fwd(rowptr=None) == E_ARG and fwd(out=None) == E_ARG
    assert fwd(N=-1) == E_ARG
    assert fwd(C=67) == E_SHAPE and fwd(C=130, ldx=130, ldo=130) == E_SHAPE and fwd(C=260, ldx=260, ldo=260) == E_SHAPE
    assert fwd(ldx=66) == E_ALIGN and fwd(ldo=65) == E_ALIGN and fwd(x=p + 8) == E_ALIGN
    assert fwd(x0=p, ld0=62) == E_ARG and fwd(x0=p, ld0=66) == E_ALIGN
    assert fwd(out=p) == E_ARG                                        # out aliases x
    assert fwd(seed=p, p_drop=1.0) == E_ARG
    assert fwd(N=0) == 0

    def dst(rowptr=p, ldx=64, ldg=64, N=10, C=64, g_alr=p):
        return lib.rgbx_faconv_bwd_dst_f32(rowptr, p, p, p, ldx, p, p + 4096, ldg, g_alr, N, C, None, 0.0, None, None)
    assert dst(rowptr=None) == E_ARG and dst(g_alr=None) == E_ARG and dst(N=-1) == E_ARG
    assert dst(C=67) == E_SHAPE and dst(ldg=66) == E_ALIGN and dst(ldx=8) == E_ARG and dst(N=0) == 0

    def src(t2f=None, seed=None, ldgx=64, N=10, C=64, g_x=p + 8192, att=p):
        return lib.rgbx_faconv_bwd_src_f32(p, p, p, t2f, p, 64, p, p + 4096, 64, att, att, p, g_x, ldgx, N, C, seed, 0.5,
                                           None, None)
    assert src(g_x=None) == E_ARG and src(N=-1) == E_ARG and src(att=None) == E_ARG
    assert src(seed=p) == E_ARG and b"slot map" in lib.rgbx_last_error_string()   # training mode without t2f
    assert src(C=65) == E_SHAPE and src(ldgx=66) == E_ALIGN and src(g_x=p + 4096) == E_ARG and src(N=0) == 0

    coef = lambda **kw: lib.rgbx_faconv_edge_coef_f32(kw.get("rowptr", p), p, p, None, kw.get("alr", p), 0, kw.get("N", 10),
                                                      kw.get("seed"), kw.get("p_drop", 0.0), kw.get("coef", p), None, None)
    assert coef(rowptr=None) == E_ARG and coef(coef=None) == E_ARG and coef(N=-1) == E_ARG
    assert coef(alr=p + 4) == E_ALIGN and coef(seed=p, p_drop=-0.1) == E_ARG and coef(N=0) == 0

    dot = lambda **kw: lib.rgbx_faconv_edge_dot_f32(p, p, kw.get("q", p), p, kw.get("lda", 67), p, 67, p, kw.get("stride", 2),
                                                    kw.get("N", 10), kw.get("C", 67), None)
    assert dot(q=None) == E_ARG and dot(N=-1) == E_ARG and dot(C=0) == E_ARG and dot(stride=0) == E_ARG
    assert dot(lda=66) == E_ARG and dot(C=64, lda=70) == E_ALIGN and dot(N=0) == 0

    draws = lib.rgbx_faconv_draws_u8
    assert draws(None, 5, 0.5, p, None) == E_ARG and draws(p, -1, 0.5, p, None) == E_ARG
    assert draws(p, 5, 1.5, p, None) == E_ARG and draws(p, 2 ** 31, 0.5, p, None) == -2 and draws(p, 0, 0.5, p, None) == 0


class TinyMLP(nn.Module):
    """A module of the caller's own: no edge_index in its forward, the package's forward contract."""

    def __init__(self, f, hid, c):
        super().__init__()
        self.a, self.b = nn.Linear(f, hid), nn.Linear(hid, c)

    def forward(self, x):
        h = self.b(F.dropout(torch.relu(self.a(x)), p=0.3, training=self.training))
        return {"out": F.log_softmax(h, dim=1), "emb": h}


def toy_data(n=120, f=6, c=3, seed=0):
    import rgb_experiment_amd as R
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, c, (n,), generator=g)
    x = torch.randn(n, f, generator=g) + 1.5 * F.one_hot(y, f).float()
    return R.Data(x=x, y=y, edge_index=torch.randint(0, n, (2, 4 * n), generator=g))


def test_experiment_trains_the_passed_module_on_the_cpu_loop():
    import rgb_experiment_amd as R
    from rgb_experiment_amd.itexperiments import _as_bool_mask, _make_masks, compare_pred_label
    data = toy_data()
    torch.manual_seed(7)
    mine = TinyMLP(6, 16, 3)
    twin = copy.deepcopy(mine)
    before = copy.deepcopy(mine.state_dict())
    epochs = 12
    res = R.experiment({"ignored": True}, specify_data=True, data=data, model=mine, model_name="GCN", use_cpu=True,
                       learning_rate=0.05, epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                       implement_early_stopping=False)
    assert res["model"] is mine and not res["used_hip_graph"]
    assert any(not torch.equal(v, before[k]) for k, v in mine.state_dict().items())
    # the same loop by hand, same seeds (reference :417-504 with the 'acc' criterion, no early stopping)
    n = data.x.size(0)
    tm, vm, sm = (_as_bool_mask(m, n, torch.device("cpu"))
                  for m in _make_masks(data.y, "ratio", "6-2-2", 20, 500, 1000, 123456789))
    random.seed(14530529)
    np.random.seed(14530529)
    torch.manual_seed(14530529)
    opt = torch.optim.Adam(twin.parameters(), lr=0.05, weight_decay=0)
    losses, best, best_acc = [], None, None
    for _ in range(epochs):
        twin.train()
        opt.zero_grad()
        out = twin(data.x)["out"]
        loss = F.nll_loss(out[tm], data.y[tm])
        losses.append(loss.item())
        loss.backward()
        opt.step()
        twin.eval()
        with torch.no_grad():
            out = twin(data.x)["out"]
        acc = (out[vm].max(1)[1] == data.y[vm]).float().mean().item()
        if best_acc is None or acc >= best_acc:
            best_acc, best = acc if best_acc is None else max(acc, best_acc), copy.deepcopy(twin.state_dict())
    twin.load_state_dict(best)
    twin.eval()
    with torch.no_grad():
        pred = twin(data.x)["out"].max(1)[1]
    want = compare_pred_label(pred[sm], data.y[sm], True)
    assert res["history"]["train_loss"] == losses
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert res[key] == want[key], key
    for k, v in mine.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k]), k
    assert losses[-1] < losses[0]


def test_experiment_model_argument_contract():
    import rgb_experiment_amd as R
    from rgb_experiment_amd.models import FAGCN
    data = toy_data()
    kw = dict(specify_data=True, data=data, use_cpu=True, epoch=3, need_to_reappear=True, print_print=False)
    # model=None: number for number the run that does not pass the keyword
    params = R.InitialParameters.defaults_for("MLP")
    a = R.experiment(params, model_name="mlp", return_model=True, **kw)
    b = R.experiment(params, model_name="mlp", return_model=True, model=None, **kw)
    assert a["history"] == b["history"] and all(a[k] == b[k] for k in ("ACC", "f1_macro", "f1_micro"))
    # the label still passes the name checks
    with pytest.raises(NotImplementedError):
        R.experiment({}, model=TinyMLP(6, 4, 3), model_name="FAGCN", **kw)
    with pytest.raises(ValueError, match="unknown model_name"):
        R.experiment({}, model=TinyMLP(6, 4, 3), model_name="nope", **kw)
    with pytest.raises(TypeError):
        R.experiment({}, model=lambda x: x, **kw)

    class NoEmb(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(6, 3)

        def forward(self, x):
            return {"out": F.log_softmax(self.lin(x), dim=1)}

    with pytest.raises(ValueError, match="'emb'"):
        R.experiment({}, model=NoEmb(), **kw)
    # a module that owns a graph layer: the layer itself refuses the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment({}, model=FAGCN(2, 6, 8, 3, 0.5, 0.3), model_name="MLP", **kw)
