"""GGNN on the MI355X: the GRU gate kernels, GatedGraphConv steps in every form (fused, composed, general) and the
whole model against a float64 restatement of PyG GatedGraphConv (tests/test_ggnn_host.py), experiment() eager vs
hipGraph, and one step of workload L's size in eval mode."""
import numpy as np
import pytest
import torch

from test_ggnn_host import RefGatedGraphConv, RefGGNN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def rand_graph(n, e, seed, loops=0, dups=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    if loops:
        k = torch.randint(0, n, (loops,), generator=g)
        ei = torch.cat([ei, torch.stack([k, k])], dim=1)
    if dups and e:
        ei = torch.cat([ei, ei[:, :dups]], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=g)]


def hub_graph(n, seed):
    """Random edges among the first n - 3 nodes (duplicates, self-loops), a star of 2500 in-edges (above
    graph.LONG_ROW_SLOTS = 1024: the row-split path) into node 0, and three isolated nodes at the end."""
    ei = rand_graph(n - 3, 6 * n, seed, loops=7, dups=9)
    g = torch.Generator().manual_seed(seed + 1)
    star = torch.stack([torch.randint(0, n - 3, (2500,), generator=g), torch.zeros(2500, dtype=torch.long)])
    return torch.cat([ei, star], 1)


def close(got, want, tol):
    """max |got - want| within tol * max(1, max |want|) (the scale of the whole tensor, as the parity tests measure)."""
    err = (got.detach().cpu().double() - want.detach()).abs().max().item()
    ok = err < tol * max(1.0, want.detach().abs().max().item())
    if not ok:
        print(f"max |diff| {err:.3e}, max |ref| {want.detach().abs().max().item():.3e}")
    return ok


def ref_cell(pre, x):
    C = x.size(1)
    r, z = torch.sigmoid(pre[:, :C]), torch.sigmoid(pre[:, C:2 * C])
    n = torch.tanh(pre[:, 2 * C:3 * C] + r * pre[:, 3 * C:])
    return (1 - z) * n + z * x


@pytest.mark.parametrize("C", [4, 7, 8, 16, 30, 40, 64, 96, 128])
def test_gru_gate_kernels(dev, C):
    from rgb_experiment_amd import ops
    Cp = (C + 3) // 4 * 4
    N = 1000
    g = torch.Generator().manual_seed(C)
    pre = torch.randn(N, 4 * Cp, generator=g, dtype=torch.float64) * 3
    pre[:40] *= 40  # saturated gates: σ and tanh at 0 / 1 / ±1
    x = torch.randn(N, Cp, generator=g, dtype=torch.float64)
    gout = torch.randn(N, Cp, generator=g, dtype=torch.float64)
    if Cp != C:  # pad columns zero, as GatedGraphConv keeps them
        x[:, C:] = 0
        gout[:, C:] = 0
        pre.view(N, 4, Cp)[:, :, C:] = 0
    out = ops.gru_gate_fwd(pre.float().to(dev), x.float().to(dev))
    pr = pre.clone().requires_grad_()
    xr = x.clone().requires_grad_()
    want = ref_cell(pr, xr)
    assert close(out, want, 1e-5)
    dpre, dxd = ops.gru_gate_bwd(pre.float().to(dev), x.float().to(dev), gout.float().to(dev))
    want.backward(gout)
    # dx_direct is only the part gout ⊙ z; the reference's x gradient is that part alone (pre does not depend on x here)
    assert close(dpre, pr.grad, 1e-5)
    assert close(dxd, xr.grad, 1e-5)
    if Cp != C:
        assert dpre.view(N, 4, Cp)[:, :, C:].abs().max().item() == 0.0


def _conv_pair(C, L, seed):
    from rgb_experiment_amd.nn import GatedGraphConv
    torch.manual_seed(seed)
    ref = RefGatedGraphConv(C, L)
    with torch.no_grad():  # biases large enough that the r / z gates matter
        ref.rnn.bias_ih.normal_(0, 0.5)
        ref.rnn.bias_hh.normal_(0, 0.5)
    conv = GatedGraphConv(C, L)
    conv.load_state_dict(ref.state_dict())
    return ref, conv


FORMS_C = [4, 7, 8, 16, 30, 40, 64, 96, 128]


@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("C", FORMS_C)
def test_gated_graph_conv_steps_all_forms(dev, C, L):
    """Output and the gradients of x and of every parameter against float64, in every form that takes the width;
    the forms agree with each other."""
    from rgb_experiment_amd import ops
    n = 1800
    ei = hub_graph(n, 100 + C)
    g = torch.Generator().manual_seed(C * 10 + L)
    f = C if C % 3 else C - 1  # a narrower input is zero-padded (PyG)
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    ref, conv = _conv_pair(C, L, C + L)
    conv = conv.to(dev)
    xr = x.clone().requires_grad_()
    want = ref(xr, ei)
    gout = torch.randn(n, C, generator=g, dtype=torch.float64)
    want.backward(gout)
    Cp = (C + 3) // 4 * 4
    forms = ["general"] + (["fused", "composed"] if ops.gru_step_supported(Cp) else [])
    outs = {}
    try:
        for form in forms:
            ops.GRU_FORM = form
            conv.zero_grad()
            xd = x.float().to(dev).requires_grad_()
            got = conv(xd, ei.to(dev))
            got.backward(gout.float().to(dev))
            assert close(got, want, 1e-4), form
            assert close(xd.grad, xr.grad, 2e-4), form
            for name, p in conv.named_parameters():
                assert close(p.grad, dict(ref.named_parameters())[name].grad, 2e-4), (form, name)
            outs[form] = got.detach()
    finally:
        ops.GRU_FORM = None
    for form in forms[1:]:
        assert (outs[form] - outs["general"]).abs().max().item() < 1e-4 * max(1.0, outs["general"].abs().max().item())
    if "fused" in forms:  # the default form is the fused kernel where it applies
        assert ops.gru_step_form(Cp) == "fused"


def test_gated_graph_conv_eval_is_the_training_forward(dev):
    """No autograd: nothing saved, the same numbers."""
    ei = hub_graph(900, 3)
    ref, conv = _conv_pair(64, 2, 5)
    conv = conv.to(dev)
    x = torch.randn(900, 64).to(dev)
    train = conv(x.clone().requires_grad_(), ei.to(dev)).detach()
    with torch.no_grad():
        ev = conv(x, ei.to(dev))
    assert torch.equal(train, ev)


def test_ggnn_model_train_mode(dev):
    from rgb_experiment_amd.models import GGNN
    n, f, c, hid, L = 1500, 20, 5, 64, 2
    ei = hub_graph(n, 21)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    y = torch.randint(0, c, (n,), generator=g)
    torch.manual_seed(7)
    ref = RefGGNN(L, hid, f, c)
    model = GGNN(num_layers=L, hidden_unit=hid, input_dim=f, output_dim=c, dropout_rate=0.5)
    model.load_state_dict(ref.state_dict(), strict=True)
    model.to(dev).train()
    ref.train()
    out = model(x.float().to(dev), ei.to(dev))
    want = ref(x, ei)
    assert close(out["out"], want["out"], 1e-4) and close(out["emb"], want["emb"], 1e-4)
    torch.nn.functional.nll_loss(out["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp = dict(ref.named_parameters())
    for name, p in model.named_parameters():
        assert close(p.grad, refp[name].grad, 2e-4), name


def test_ggnn_experiment_hip_graph_equals_eager(dev):
    import rgb_experiment_amd as R
    n, f, c = 1500, 40, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 9000, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = R.InitialParameters.defaults_for("ggnn")
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="ggnn", learning_rate=0.01, epoch=8,
                                 need_to_reappear=True, print_print=False, return_model=True, use_hip_graph=graphed,
                                 need_all_metrics=False))
    a, b = runs
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(b["history"]["train_loss"]) == 8
    for key in ("train_loss", "val_loss", "test_loss", "train_acc", "val_acc", "test_acc"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=2e-6), key
    for (ka, va), (kb, vb) in zip(a["model"].state_dict().items(), b["model"].state_dict().items()):
        assert ka == kb and torch.allclose(va.float(), vb.float(), atol=1e-6), ka
    assert a["history"]["train_loss"][-1] < a["history"]["train_loss"][0]  # it trains


@pytest.mark.slow
def test_ggnn_eval_at_workload_l_on_sampled_rows(dev):
    """|V| = 2 M, |E| = 60 M (bench.py's workload L graph), default GGNN in eval mode: the logits of 64 sampled rows
    against float64 over their 2-hop in-neighbourhood (eval BatchNorm is per row, so that is all a row depends on)."""
    import bench
    from rgb_experiment_amd.models import GGNN
    wl = bench.WORKLOADS["L"]
    ei, x, _ = bench.synth(wl["N"], wl["E"], wl["d"])
    N, f, c = wl["N"], wl["d"], 16
    torch.manual_seed(3)
    model = GGNN(num_layers=2, hidden_unit=64, input_dim=f, output_dim=c, dropout_rate=0.5)
    with torch.no_grad():  # non-trivial running statistics
        for bn in (model.bn1, model.bn2):
            bn.running_mean.normal_(0, 0.3)
            bn.running_var.uniform_(0.5, 2.0)
    model.to(dev).eval()
    eid = ei.to(dev)
    with torch.no_grad():
        logits = model(x.to(dev), eid)["emb"]
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:64].to(dev)
    # 2-hop in-neighbourhood: edges into rows, into their sources
    src, dst = eid[0], eid[1]
    hit1 = torch.zeros(N, dtype=torch.bool, device=dev)
    hit1[rows] = True
    e1 = hit1[dst]
    hop1 = torch.unique(torch.cat([rows, src[e1]]))
    hit2 = torch.zeros(N, dtype=torch.bool, device=dev)
    hit2[hop1] = True
    e2 = hit2[dst]
    nodes = torch.unique(torch.cat([hop1, src[e2]]))
    local = torch.full((N,), -1, dtype=torch.long, device=dev)
    local[nodes] = torch.arange(nodes.numel(), device=dev)
    sub_ei = torch.stack([local[src[e2]], local[dst[e2]]]).cpu()
    ref = RefGGNN(2, 64, f, c)
    ref.load_state_dict({k: (v.double() if v.is_floating_point() else v).cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        want = ref(x[nodes.cpu()].double(), sub_ei)["emb"][local[rows].cpu()]
    assert close(logits[rows], want, 1e-4)
