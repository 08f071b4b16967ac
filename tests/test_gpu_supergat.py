"""SuperGAT on the MI355X: SuperGATConv (eval and training mode, hub rows), the negative sampler, the whole model and
experiment() against the float64 restatement of tests/test_supergat_host.py, which is fed the exact random choices
the device made (ops.supergat_random_choices), and the default model at workload L's size in eval mode.

Tolerances are the project's (tests/test_gpu_parity.py, tests/test_gpu_ggnn.py): forward 1e-4 * max(1, |ref|max),
gradients 2e-4 * max(1, |ref|max). DESIGN.md 3.6: a pre-activation score within ~1e-6 of zero lets float32 and float64
differentiate different LeakyReLU branches, so every seeded input of a gradient test is checked on the CPU with the
restatement (`assert_no_kink`: smallest |s| above 1e-5 * max |s|); a seed that failed was replaced by the next one.
Chosen seeds -> smallest |s| / max |s| of the layer inputs (random graph; hub graph):
  (1, 7, True): seed 100 -> 1.10e+00 / 3.50e+00
  (1, 7, False): seed 100 -> 1.10e+00 / 3.50e+00
  (8, 8, True): seed 100 -> 7.06e-01 / 3.77e+00
  (8, 8, False): seed 100 -> 8.48e-01 / 3.80e+00
  (8, 7, True): seed 100 -> 8.28e-01 / 3.56e+00
  (8, 7, False): seed 100 -> 7.74e-01 / 3.73e+00
  (4, 16, True): seed 100 -> 9.83e-01 / 3.76e+00
  (4, 16, False): seed 100 -> 9.39e-01 / 3.75e+00
  (8, 40, True): seed 100 -> 6.03e-01 / 3.75e+00
  (8, 40, False): seed 100 -> 5.01e-01 / 3.81e+00
  (2, 64, True): seed 100 -> 6.89e-01 / 3.59e+00
  (2, 64, False): seed 100 -> 4.68e-01 / 3.80e+00
  hub graph (8, 8, True) and (8, 40, False): seed 200 -> 6.78e-01 / 3.74e+00 and 2.64e-01 / 3.99e+00
"""
import numpy as np
import pytest
import torch

from test_gpu_ggnn import close, hub_graph, rand_graph
from test_supergat_host import RefSuperGAT, RefSuperGATConv

pytestmark = pytest.mark.gpu

# (H, C, concat) -> seed of the layer tests (see the module docstring)
SEEDS = {(1, 7, True): 100, (1, 7, False): 100, (8, 8, True): 100, (8, 8, False): 100, (8, 7, True): 100, (8, 7, False): 100, (4, 16, True): 100, (4, 16, False): 100, (8, 40, True): 100, (8, 40, False): 100, (2, 64, True): 100, (2, 64, False): 100}
HUB_SEED = 200


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def make_case(H, C, concat, seed, ei, f=12, p=0.0):
    """(x float64 [n, f], reference layer with seeded parameters and a non-zero bias). The score s = t * sigmoid(d),
    t = <h_j, att_l> + <h_i, att_r>, of 6,700 edges x 8 heads of zero-mean random parameters comes within 1e-5 * max |s|
    of zero on practically every seed (500 seeds tried), so the parameters keep t away from zero by construction: feature
    0 is the constant 1, it drives channel 0 of every head (weight 1, the other weights of that row damped), and both
    attention vectors carry +-1.5 on that channel — t is about -3 on even heads (LeakyReLU's slope branch) and +3 on odd
    heads, with every other entry random. The rows of h keep a standard deviation of 0.5 / C^(1/4) per channel, so d stays
    within a few units, sigmoid(d) away from 0, and every term of the backward carries weight."""
    n = int(ei.max()) + 1
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    x[:, 0] = 1.0
    ref = RefSuperGATConv(f, C, heads=H, concat=concat, dropout=p)
    with torch.no_grad():
        for name, prm in ref.named_parameters():
            scale = {"lin.weight": 0.5 / f ** 0.5 / C ** 0.25, "bias": 0.4}.get(name, 0.1)
            prm.copy_(torch.randn(prm.shape, generator=g, dtype=torch.float64) * scale)
        for h in range(H):
            ref.lin.weight[h * C, 0] = 1.0
            ref.lin.weight[h * C, 1:] *= 0.2
            sign = -1.0 if h % 2 == 0 else 1.0
            ref.att_l[0, h, 0] += 1.5 * sign
            ref.att_r[0, h, 0] += 1.5 * sign
    return x, ref


def assert_no_kink(ref):
    s = ref.s.detach().abs()
    assert s.min().item() > 1e-5 * s.max().item(), (s.min().item(), s.max().item())


def device_layer(ref, f, dev, p=0.0, ratios=(1.0, 0.5)):
    from rgb_experiment_amd.nn import SuperGATConv
    conv = SuperGATConv(f, ref.C, heads=ref.H, concat=ref.concat, dropout=p, edge_sample_ratio=ratios[0],
                        neg_sample_ratio=ratios[1])
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv.to(dev)


def choices_of(conv, ei_dev, n):
    """The random choices of conv's last training forward, on the CPU, for the restatement."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    graph = get_graph(ei_dev, n, LOOPS_REMOVE_ADD)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ops.supergat_random_choices(conv.last_draw, graph, conv.heads).items()}


def check_grads(conv, ref, x_dev, x_ref):
    assert close(x_dev.grad, x_ref.grad, 2e-4), "x"
    refp = dict(ref.named_parameters())
    for name, prm in conv.named_parameters():
        assert close(prm.grad, refp[name].grad, 2e-4), name


def run_eval(H, C, concat, seed, ei, dev):
    x, ref = make_case(H, C, concat, seed, ei)
    ref.eval()
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei)
    assert_no_kink(ref)
    conv = device_layer(ref, x.size(1), dev).eval()
    xd = x.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev))
    assert close(out, want, 1e-4)
    assert conv.get_attention_loss().item() == 0.0
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    check_grads(conv, ref, xd, xr)


def run_train(H, C, concat, seed, ei, dev, torch_seed=5):
    x, ref = make_case(H, C, concat, seed, ei, p=0.6)
    n = x.size(0)
    conv = device_layer(ref, x.size(1), dev, p=0.6, ratios=(0.8, 0.5)).train()
    xd = x.float().to(dev).requires_grad_(True)
    eid = ei.to(dev)
    torch.manual_seed(torch_seed)
    out = conv(xd, eid)
    loss = conv.get_attention_loss()
    ch = choices_of(conv, eid, n)
    ref.train()
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei, ch)
    assert_no_kink(ref)
    print(f"train ({H},{C},{concat}): att_loss {loss.item():.6f} vs {ref.att_loss.item():.6f}; kept positives "
          f"{int(ch['pos'].sum())} of {ch['pos'].numel()}, negatives {int(ch['valid'].sum())} of {ch['valid'].numel()}")
    assert close(out, want, 1e-4)
    assert close(loss, ref.att_loss, 1e-4)
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    ((out * cot.float().to(dev)).sum() + 4 * loss).backward()
    ((want * cot).sum() + 4 * ref.att_loss).backward()
    check_grads(conv, ref, xd, xr)
    return conv, xd, eid, out, ch


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,C", [(1, 7), (8, 8), (8, 7), (4, 16), (8, 40), (2, 64)])
def test_supergat_conv_eval_forward_backward(dev, H, C, concat):
    ei = rand_graph(700, 6000, 3, loops=11, dups=40)
    run_eval(H, C, concat, SEEDS[(H, C, concat)], ei, dev)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("H,C", [(1, 7), (8, 8), (8, 7), (4, 16), (8, 40), (2, 64)])
def test_supergat_conv_training_forward_backward(dev, H, C, concat):
    ei = rand_graph(700, 6000, 3, loops=11, dups=40)
    run_train(H, C, concat, SEEDS[(H, C, concat)], ei, dev)


def test_supergat_training_is_repeatable_under_manual_seed(dev):
    ei = rand_graph(700, 6000, 3, loops=11, dups=40)
    seed = SEEDS[(8, 8, True)]
    conv, xd, eid, out_a, ch_a = run_train(8, 8, True, seed, ei, dev, torch_seed=5)
    loss_a = conv.get_attention_loss().item()
    torch.manual_seed(5)
    out_b = conv(xd, eid)
    ch_b = choices_of(conv, eid, xd.size(0))
    assert torch.equal(out_a, out_b) and conv.get_attention_loss().item() == loss_a
    for k in ("pos", "drop", "neg", "valid"):
        assert torch.equal(ch_a[k], ch_b[k]), k
    torch.manual_seed(6)
    conv(xd, eid)
    ch_c = choices_of(conv, eid, xd.size(0))
    assert not torch.equal(ch_a["pos"], ch_c["pos"]) and not torch.equal(ch_a["drop"], ch_c["drop"])
    assert not torch.equal(ch_a["neg"], ch_c["neg"])


@pytest.mark.parametrize("H,C,concat", [(8, 8, True), (8, 40, False)])
def test_supergat_conv_hub_rows(dev, H, C, concat):
    """One target with 2500 in-edges (above LONG_ROW_SLOTS = 1024: chunk + combine kernels in all three passes) and
    isolated nodes, eval and training mode."""
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    ei = hub_graph(1500, 21)
    assert get_graph(ei.to(dev), 1500, LOOPS_REMOVE_ADD).fwd.split is not None
    run_eval(H, C, concat, HUB_SEED, ei, dev)
    run_train(H, C, concat, HUB_SEED, ei, dev)


def test_supergat_sampler_properties(dev):
    from rgb_experiment_amd.nn import SuperGATConv
    n, e = 5000, 40000
    ei = rand_graph(n, e, 17, loops=5, dups=30)
    eid = ei.to(dev)
    torch.manual_seed(1)
    conv = SuperGATConv(16, 8, heads=8, dropout=0.6, edge_sample_ratio=0.8, neg_sample_ratio=0.5).to(dev).train()
    x = torch.randn(n, 16, device=dev)
    conv(x, eid)
    ch = choices_of(conv, eid, n)
    e2 = ch["pos"].numel()  # E' after the self-loop rewrite
    assert e2 == int((ei[0] != ei[1]).sum()) + n
    assert ch["neg"].shape == (2, int(0.5 * 0.8 * e2))
    assert bool(ch["valid"].all())  # non-edge density > 0.996 per draw, 8 re-draws: a failed slot has p < 1e-19
    edges = set(zip(ei[0].tolist(), ei[1].tolist()))
    for u, v in zip(ch["neg"][0].tolist(), ch["neg"][1].tolist()):
        assert u != v and (u, v) not in edges and (v, u) not in edges
    assert 0 <= int(ch["neg"].min()) and int(ch["neg"].max()) < n
    kept = int(ch["pos"].sum())
    assert abs(kept - 0.8 * e2) <= 5 * (e2 * 0.8 * 0.2) ** 0.5, kept
    frac = ch["drop"].float().mean().item()
    assert abs(frac - 0.4) <= 5 * (0.4 * 0.6 / ch["drop"].numel()) ** 0.5, frac
    assert int(conv.last_draw["pos_stats"][1].item()) == kept
    assert int(conv.last_draw["neg_stats"][1].item()) == ch["neg"].size(1)
    # caller-supplied negatives bypass the sampler
    mine = torch.tensor([[0, 1, 2, 7], [3, 4, 5, 7]], device=dev)
    conv(x, eid, neg_edge_index=mine)
    assert torch.equal(conv.last_draw["neg"], mine) and conv.last_draw["valid"] is None
    assert int(conv.last_draw["neg_stats"][1].item()) == 4


def test_supergat_model_against_restatement(dev):
    """SuperGAT at the reference defaults (glorot parameters, which cannot be steered as make_case does, and a second
    layer whose input depends on the device's dropout draws): the kink criterion is evaluated on the CPU for the device
    seeds 8, 9, ... 71 in turn and the first training forward that meets it on both layers is the one compared."""
    from rgb_experiment_amd.models import SuperGAT
    n, f, c = 200, 24, 5
    ei = rand_graph(n, 1200, 31, loops=6, dups=20)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    y = torch.randint(0, c, (n,), generator=g)
    torch.manual_seed(41)
    model = SuperGAT(input_dim=f, hidden_dim=8, output_dim=c, heads=8, dropout_rate=0.6, edge_sample_ratio=0.8,
                     neg_sample_ratio=0.5)
    with torch.no_grad():
        model.conv1.bias.normal_(0, 0.2)
        model.conv2.bias.normal_(0, 0.2)
        # glorot weights x 0.3: at full scale the products d reach -16 and sigmoid(d) carries |s| to 1e-12 * max |s| and
        # below in every forward (32 device seeds tried); at 0.3 |d| stays below 6 and about one forward in five has
        # no score inside the kink band on either layer
        model.conv1.lin.weight.mul_(0.3)
        model.conv2.lin.weight.mul_(0.3)
    ref = RefSuperGAT(f, 8, c, 8, 0.6)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    model.to(dev)
    eid = ei.to(dev)
    # eval mode
    model.eval()
    ref.eval()
    with torch.no_grad():
        out = model(x.float().to(dev), eid)
        want = ref(x, ei)
    assert close(out["emb"], want["emb"], 1e-4) and close(out["out"], want["out"], 1e-4)
    assert out["att_loss"].item() == 0.0 and "att_loss" in out.keys()
    # training mode: the two feature dropouts are recorded too — what each conv was fed shows its mask (a float32
    # normal draw, or elu of a float32 sum, is not exactly 0 unless it was dropped)
    model.train()
    ref.train()
    for device_seed in range(8, 72):
        captured = {}
        hooks = [model.conv1.register_forward_pre_hook(lambda mod, args: captured.__setitem__("x1", args[0].detach())),
                 model.conv2.register_forward_pre_hook(lambda mod, args: captured.__setitem__("x2", args[0].detach()))]
        torch.manual_seed(device_seed)
        res = model(x.float().to(dev), eid)
        for hk in hooks:
            hk.remove()
        mask0, mask1 = (captured["x1"] != 0).cpu(), (captured["x2"] != 0).cpu()
        ch = (choices_of(model.conv1, eid, n), choices_of(model.conv2, eid, n))
        want = ref(x, ei, ch, masks=(mask0, mask1))
        ratios = [cv.s.detach().abs().min().item() / cv.s.detach().abs().max().item() for cv in (ref.conv1, ref.conv2)]
        print(f"device seed {device_seed}: smallest |s| / max |s| = {ratios[0]:.2e}, {ratios[1]:.2e}")
        if min(ratios) > 1e-5:
            break
    for conv in (ref.conv1, ref.conv2):
        assert_no_kink(conv)
    assert abs(mask0.float().mean().item() - 0.4) < 0.03 and abs(mask1.float().mean().item() - 0.4) < 0.03
    assert close(res["emb"], want["emb"], 1e-4) and close(res["att_loss"], want["att_loss"], 1e-4)
    (torch.nn.functional.nll_loss(res["out"], y.to(dev)) + 4 * res["att_loss"]).backward()
    (torch.nn.functional.nll_loss(want["out"], y) + 4 * want["att_loss"]).backward()
    refp = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        assert close(prm.grad, refp[name].grad, 2e-4), name


def test_supergat_experiment(dev):
    import rgb_experiment_amd as R
    from rgb_experiment_amd.models._stack import masked_ce
    n, f, c = 300, 20, 4
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 2000, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = R.InitialParameters.defaults_for("SuperGAT")
    kw = dict(specify_data=True, data=data, model_name="supergat", learning_rate=0.01, epoch=8, need_to_reappear=True,
              print_print=False, return_model=True, need_all_metrics=True)
    a = R.experiment(params, **kw)
    b = R.experiment(params, **kw)
    assert set(a) >= {"ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"}
    assert not a["used_hip_graph"] and len(a["history"]["train_loss"]) == 8
    # the negative pairs' row gradients are added with float atomics (include/rgbx_hip.h: the one order-dependent sum of
    # the layer), so two runs agree to the last bits, not bit for bit: the bound of the eager-vs-graph test of GGNN
    for key in ("train_loss", "val_loss", "test_loss", "train_acc", "val_acc", "test_acc"):
        print(key, a["history"][key], b["history"][key])
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=2e-6), key
    zero = R.experiment(params, supergat_graph_lambda=0, **kw)
    # the first step by hand, under the same seed: experiment() seeds, builds the model, then runs the training forward
    import random
    from rgb_experiment_amd.itexperiments import _as_bool_mask, _make_masks
    tm, _, _ = _make_masks(data.y, "ratio", "6-2-2", 20, 500, 1000, 123456789)
    random.seed(14530529)
    np.random.seed(14530529)
    torch.manual_seed(14530529)
    torch.cuda.manual_seed(14530529)
    from rgb_experiment_amd.models import SuperGAT
    net = SuperGAT(input_dim=f, output_dim=c, **params).to(dev).train()
    ce, _ = masked_ce(net, {"x": data.x.to(dev), "edge_index": ei.to(dev)}, data.y.to(dev), _as_bool_mask(tm, n, dev))
    first = (ce + 4 * net.att_loss).item()
    print(f"first step: CE {ce.item():.6f}, att_loss {net.att_loss.item():.6f}; history {a['history']['train_loss'][0]:.6f}, "
          f"lambda=0 history {zero['history']['train_loss'][0]:.6f}")
    assert net.att_loss.item() > 0
    assert abs(a["history"]["train_loss"][0] - first) <= 1e-6 * max(1.0, abs(first))
    assert abs(zero["history"]["train_loss"][0] - ce.item()) <= 1e-6 * max(1.0, abs(ce.item()))


@pytest.mark.slow
def test_supergat_eval_at_workload_l_on_sampled_rows(dev):
    """|V| = 2 M, |E| = 60 M (bench.py's workload L graph), default SuperGAT in eval mode: the logits of 64 sampled rows
    against float64 over their 2-hop in-neighbourhood, which is all a row depends on."""
    import bench
    from rgb_experiment_amd.models import SuperGAT
    wl = bench.WORKLOADS["L"]
    ei, x, _ = bench.synth(wl["N"], wl["E"], wl["d"])
    N, f, c = wl["N"], wl["d"], 16
    torch.manual_seed(3)
    model = SuperGAT(input_dim=f, output_dim=c, hidden_dim=8, heads=8, dropout_rate=0.6, edge_sample_ratio=0.8,
                     neg_sample_ratio=0.5)
    with torch.no_grad():
        model.conv1.bias.normal_(0, 0.2)
        model.conv2.bias.normal_(0, 0.2)
    model.to(dev).eval()
    eid = ei.to(dev)
    with torch.no_grad():
        logits = model(x.to(dev), eid)["emb"]
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:64].to(dev)
    src, dst = eid[0], eid[1]
    hit1 = torch.zeros(N, dtype=torch.bool, device=dev)
    hit1[rows] = True
    hop1 = torch.unique(torch.cat([rows, src[hit1[dst]]]))
    hit2 = torch.zeros(N, dtype=torch.bool, device=dev)
    hit2[hop1] = True
    e2 = hit2[dst]
    nodes = torch.unique(torch.cat([hop1, src[e2]]))
    local = torch.full((N,), -1, dtype=torch.long, device=dev)
    local[nodes] = torch.arange(nodes.numel(), device=dev)
    sub_ei = torch.stack([local[src[e2]], local[dst[e2]]]).cpu()
    ref = RefSuperGAT(f, 8, c, 8, 0.6)
    ref.load_state_dict({k: v.double().cpu() for k, v in model.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        want = ref(x[nodes.cpu()].double(), sub_ei)["emb"][local[rows].cpu()]
    assert close(logits[rows], want, 1e-4)
