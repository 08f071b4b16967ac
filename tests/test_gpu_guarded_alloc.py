"""The three seeded fuzzes, and a sweep of the kernels no fuzz reaches, over guarded and poisoned buffers.

tests/_guarded_alloc.py puts every allocation the package makes through the module global `torch` between two bands and
pre-fills it: an element a kernel skips reads as NaN in what is compared with the float64 reference (NaN fails every
comparison here), a store next to a buffer changes a band, and Guard.check() names the allocation.

(a) replays every pinned seed of test_gpu_fuzz, test_gpu_fuzz_families and test_gpu_fuzz_edge_families, block by block
as those files run them, with their own assertions and bars; one assertion is added (a compared tensor is finite wherever
its reference is). No case of the three captures a hipGraph, so none is skipped. What the replay does not reach: buffers the
fuzz files allocate themselves (the blocked output `ob` of the fused-layer cases comes from the test module's own
torch.empty and is neither poisoned nor banded), and the fused-layer cases compare with inline asserts, not through check /
_close, so the added assertion is not in front of them (a NaN in a package-allocated output still fails their `<`).

(b) sweeps bn.hip, loss.hip, gemm.hip, rows.hip, graph_prep.hip, rgbx_fold_bn_linear_f32 and rgbx_blocked_to_rows_f32
against plain float64 torch at the sizes where their code branches. Operands are placed by the layouts of
test_gpu_fuzz_families.place with NaN in the slack. The draws are tables (bn_case, loss_case, ...):
tests/test_guarded_alloc_host.py asserts that every listed value occurs in them.

Bars are those of the parity tests of the same operators (tests/test_gpu_parity.py). Where such a fixed bar means nothing
(BatchNorm over one or two rows, a constant column, a column of spread 1e-2 under a mean of 1e3) the rule of
test_gpu_fuzz._close applies, one kind of column at a time: within 16 times what a float32 restatement is off from the float64 one, or
the fixed bar, whichever is larger. profiles/guarded_alloc_suite.txt has what was measured."""
import json
import math
import random

import pytest
import torch

import test_gpu_fuzz as F0
import test_gpu_fuzz_edge_families as FE
import test_gpu_fuzz_families as FF
from _guarded_alloc import guarded
from oracle import ref_cpu as O
from test_gpu_fuzz import run_case, run_fused_layer_case, run_model_case
from test_gpu_fuzz_edge_families import run_edge_family_case
from test_gpu_fuzz_families import PINNED_BLOCKS, SOAK_FOUND, run_family_case
from test_gpu_parity import CSR_CASES, rand_graph

pytestmark = pytest.mark.gpu

NAN = float("nan")
OWN_FACTOR = 16.0  # test_gpu_fuzz._close


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda")


# ---- (a) the replay ---------------------------------------------------------------------------------------------------------

def _finite_where(name, got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.shape == ref.shape and ref.numel():
        bad = torch.isfinite(ref) & ~torch.isfinite(got)
        assert not bool(bad.any()), (name, "not finite where the reference is", int(bad.sum()), "element(s): unwritten?")


def _with_finite_checks(monkeypatch):
    """test_gpu_fuzz.check and ._close (which the family fuzzes' compare ends in) with the added assertion in front."""
    check, close = F0.check, F0._close

    def check_finite(name, got, ref, *a, **k):
        _finite_where(name, got, ref)
        return check(name, got, ref, *a, **k)

    def close_finite(name, got, ref64, ref32, *a, **k):
        _finite_where(name, got, ref64)
        return close(name, got, ref64, ref32, *a, **k)

    monkeypatch.setattr(F0, "check", check_finite)
    monkeypatch.setattr(F0, "_close", close_finite)


def refused(suite, seed):
    """A case whose own draw is a width the entry point refuses: the fuzz asserts the documented error and returns, no
    kernel runs and nothing is allocated. Such a case cannot meet "one guarded float allocation per kind"; every other
    case must."""
    if suite == "families":
        c = FF.draw_case(seed)
        return c["kind"] in FF.SOFTMAX and not FF.head_width_supported(c["C"])
    if suite == "edge_families":
        return bool(FE.draw_case(seed)["refused"])
    return False


def replay(monkeypatch, suite, cases):
    """cases: [(kind, seed, function of the seed)]. Runs them under the guard; at least one guarded float allocation per
    kind, and every band intact."""
    _with_finite_checks(monkeypatch)
    made = {}
    with guarded(monkeypatch) as guard:
        for kind, seed, fn in cases:
            before = guard.float_allocations
            fn(seed)
            if not refused(suite, seed):
                made[kind] = made.get(kind, 0) + guard.float_allocations - before
        torch.cuda.synchronize()
        guard.check()
    idle = sorted(k for k, v in made.items() if v == 0)
    assert not idle, (suite, "kinds that ran without one guarded float allocation", idle,
                      [(k, s) for k, s, _ in cases if k in idle])
    tally(guard)
    return guard


@pytest.mark.parametrize("block", range(8))
def test_conv_layer_fuzz_under_the_guard(dev, monkeypatch, block):
    replay(monkeypatch, "conv", [(F0.KINDS[(9000 + s) % len(F0.KINDS)], 9000 + s, lambda seed: run_case(dev, seed))
                                 for s in range(block * 40, block * 40 + 8)])


@pytest.mark.parametrize("block", range(3))
def test_whole_model_fuzz_under_the_guard(dev, monkeypatch, block):
    replay(monkeypatch, "model", [(F0.MODEL_KINDS[s % len(F0.MODEL_KINDS)], s, lambda seed: run_model_case(dev, seed))
                                  for s in range(block * 25, block * 25 + 10)])


@pytest.mark.parametrize("part", range(3))
def test_whole_model_fuzz_on_sparse_features_under_the_guard(dev, monkeypatch, part):
    """Seeds 6000 .. 6089 by threes (test_whole_models_on_sparse_features), in three parts, and 557 in the first."""
    seeds = list(range(6000, 6090, 3))[part * 10:(part + 1) * 10] + ([557] if part == 0 else [])
    replay(monkeypatch, "model", [(F0.MODEL_KINDS[s % len(F0.MODEL_KINDS)], s, lambda seed: run_model_case(dev, seed))
                                  for s in seeds])


@pytest.mark.parametrize("block", range(4))
def test_fused_layer_fuzz_under_the_guard(dev, monkeypatch, block):
    replay(monkeypatch, "fused", [("fused_layer", s, lambda seed: run_fused_layer_case(dev, seed))
                                  for s in range(block * 100, block * 100 + 15)])


@pytest.mark.parametrize("block", PINNED_BLOCKS)
def test_family_fuzz_under_the_guard(dev, monkeypatch, block):
    replay(monkeypatch, "families", [(FF.KINDS[s % len(FF.KINDS)], s, lambda seed: run_family_case(dev, seed))
                                     for s in range(block * 8, block * 8 + 8)])


@pytest.mark.parametrize("seed", [s for s in SOAK_FOUND if s // 8 not in PINNED_BLOCKS])
def test_family_soak_seeds_under_the_guard(dev, monkeypatch, seed):
    replay(monkeypatch, "families", [(FF.KINDS[seed % len(FF.KINDS)], seed, lambda s: run_family_case(dev, s))])


@pytest.mark.parametrize("block", FE.PINNED_BLOCKS)
def test_edge_family_fuzz_under_the_guard(dev, monkeypatch, block):
    k = len(FE.KINDS)
    replay(monkeypatch, "edge_families", [(FE.KINDS[s % k], s, lambda seed: run_edge_family_case(dev, seed))
                                          for s in range(block * k, (block + 1) * k)])


@pytest.mark.parametrize("seed", [s for s in FE.SOAK_FOUND if s // len(FE.KINDS) not in FE.PINNED_BLOCKS])
def test_edge_family_soak_seeds_under_the_guard(dev, monkeypatch, seed):
    replay(monkeypatch, "edge_families", [(FE.KINDS[seed % len(FE.KINDS)], seed, lambda s: run_edge_family_case(dev, s))])


# ---- (b) the sweep: shared pieces -----------------------------------------------------------------------------------------

LAYOUTS = [("fresh",), ("block", "2F", 0, 1), ("block", "3F", 0, 2), ("block", "pad", 4, 1), ("block", "pad", 1, 1),
           ("block", "pad", 3, 0), ("offset", 1), ("offset", 2), ("offset", 3)]


def place_nan(t, spec, dev, requires_grad=False):
    """test_gpu_fuzz_families.place with NaN in the slack: [n, F] -> (operand view on the device, leaf, function
    leaf.grad -> ([n, F] gradient, gradient of the slack or None))."""
    n, F = t.shape
    total, c0, ld = FF.layout_geometry(spec, n, F)
    if spec[0] == "fresh":
        leaf = t.float().to(dev).requires_grad_(requires_grad)
        return leaf, leaf, lambda g: (g, None)
    base = torch.full((total,), NAN, device=dev)
    if spec[0] == "block":
        base.view(n, ld)[:, c0:c0 + F] = t.float().to(dev)
        base.requires_grad_(requires_grad)

        def split(g):
            g = g.view(n, ld)
            return g[:, c0:c0 + F], torch.cat([g[:, :c0], g[:, c0 + F:]], dim=1)
        return base.view(n, ld)[:, c0:c0 + F], base, split
    base[c0:c0 + n * F] = t.float().to(dev).reshape(-1)
    base.requires_grad_(requires_grad)
    return (base[c0:c0 + n * F].view(n, F), base,
            lambda g: (g[c0:c0 + n * F].view(n, F), torch.cat([g[:c0], g[c0 + n * F:]])))


def slack_is_zero(name, slack):
    if slack is not None and slack.numel():
        assert float(slack.abs().max()) == 0.0, (name, "gradient outside the operand's columns")


def out_view(shape, dev, rng, aligned=False):
    """A contiguous `shape` view a few floats (`aligned`: a multiple of four) into one flat NaN-filled buffer, and the
    function that asserts the rest of the buffer still holds NaN."""
    n = math.prod(shape)
    lead, tail = rng.choice([4, 8] if aligned else [0, 3, 4]), rng.choice([1, 4, 5])
    flat = torch.full((lead + n + tail,), NAN, device=dev)

    def untouched(name):
        rest = torch.cat([flat[:lead], flat[lead + n:]])
        assert bool(torch.isnan(rest).all()), (name, "wrote outside the view it was given")
    return flat[lead:lead + n].view(shape), untouched


def within(name, got, ref64, bar, ref32=None, report=None):
    """|got - ref64| <= bar elementwise (bar: a number or a tensor that broadcasts); with `ref32` (a float32 restatement)
    the bar is raised, where the restatement itself is further off, to OWN_FACTOR times its own largest distance over the
    tensor handed in, as test_gpu_fuzz._close takes it: callers hand in columns of one kind at a time."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, tuple(got.shape), tuple(ref64.shape))
    if not ref64.numel():
        return
    _finite_where(name, got, ref64)
    err = (got - ref64).abs()
    bound = torch.as_tensor(bar, dtype=torch.float64).expand_as(err)
    if ref32 is not None:
        own = (ref32.detach().double() - ref64).abs().max().item()
        if report is not None:
            report.append((name, err.max().item(), own))
        bound = torch.maximum(bound, torch.full_like(err, OWN_FACTOR * own))
    worst = (err - bound).max().item()
    assert worst <= 0.0, (name, "error", err.max().item(), "bar", float(bound.max()), "over by", worst)


def tally(guard):
    """One line per test for `pytest -s` (profiles/guarded_alloc_suite.txt adds them up)."""
    print("GUARDED", json.dumps({"allocations": guard.allocations, "float": guard.float_allocations, "sites": guard.counts()}))


def finish(guard):
    torch.cuda.synchronize()
    guard.check()
    assert guard.float_allocations >= 1, "nothing ran under the guard"
    tally(guard)


# ---- BatchNorm ------------------------------------------------------------------------------------------------------------

BN_D = [1, 3, 4, 7, 64, 132, 257, 1028]
BN_N = [1, 2, 15, 16, 17, 255, 257, 4097]
BN_CASES = 16


def bn_case(k):
    rng = random.Random(7000 + k)
    d, n = BN_D[k % 8], BN_N[(3 * k + k // 8) % 8]
    cols = list(range(d))
    rng.shuffle(cols)
    return {"k": k, "d": d, "n": n, "layout": LAYOUTS[(k * 5 + 1) % len(LAYOUTS)], "colsums": k % 2 == 1,
            "constant": cols[0], "offset": cols[1] if d > 1 else None,
            "cot": rng.choice(["dense", "stride2", "offset3"])}


def bn_restate(x, w, b, rm, rv, eps, mom, dtype, go):
    """One training step of BatchNorm1d over the rows in plain torch at `dtype`: (y, gx, gw, gb, running_mean,
    running_var). nn.BatchNorm1d itself refuses one row; the package follows its rule for the running variance with
    n - 1 clamped at 1. The float64 reference is the centred form. The float32 restatement, the yardstick of the _close
    rule, is the form the module documents as its contract (train_statistics, eval_affine: BN(x) = x * scale + shift with
    scale = w * rstd and shift = b - mean * scale, what lets the next layer fold it into its aggregate): where that form
    costs accuracy (a column whose spread is far below its mean) the yardstick shows it, and nothing else is added."""
    x, w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    n = x.size(0)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    y = affine_form(x, mean, var, w, b, eps, dtype)
    y.backward(go.to(dtype))
    with torch.no_grad():
        rm = (1 - mom) * rm.to(dtype) + mom * mean
        rv = (1 - mom) * rv.to(dtype) + mom * var * (n / max(n - 1, 1))
    return [t.detach() for t in (y, x.grad, w.grad, b.grad, rm, rv)]


def affine_form(x, mean, var, w, b, eps, dtype):
    if dtype == torch.float64:
        return (x - mean) * torch.rsqrt(var + eps) * w + b
    scale = w * torch.rsqrt(var + eps)
    return x * scale + (b - mean * scale)


def run_bn_case(dev, c, report):
    from rgb_experiment_amd.nn import BatchNorm1d
    from rgb_experiment_amd.nn.batchnorm import _AffineCols
    n, d = c["n"], c["d"]
    gen = torch.Generator().manual_seed(100 + c["k"])
    x = torch.randn(n, d, generator=gen) * 3 + 5      # test_batchnorm_matches_torch's inputs
    x[:, c["constant"]] = 2.5
    if c["offset"] is not None:
        x[:, c["offset"]] = 1e3 + 1e-2 * torch.randn(n, generator=gen)
    go = torch.randn(n, d, generator=gen)
    w0, b0 = torch.rand(d, generator=gen) * 1.5 + 0.5, torch.rand(d, generator=gen) * 2 - 1
    mine = BatchNorm1d(d)
    with torch.no_grad():
        mine.weight.copy_(w0)
        mine.bias.copy_(b0)
    mine.to(dev)
    eps, mom = mine.eps, mine.momentum
    hard = torch.zeros(d, dtype=torch.bool)      # columns (all of them at n <= 2) where the fixed bars mean nothing
    hard[c["constant"]] = True
    if c["offset"] is not None:
        hard[c["offset"]] = True
    if n <= 2:
        hard[:] = True
    rm64 = rm32 = torch.zeros(d)
    rv64 = rv32 = torch.ones(d)

    # The hard columns are compared one kind at a time, so that the constant column (whose exact answer is the bias) does
    # not inherit the bar of the 1e3-mean column. Over one or two rows every column is hard and the case is one kind, as
    # the issue lists it and as _close takes a whole tensor: what the affine form costs a column there is ONE rounding of
    # its shift, a single draw per column, and the restatement's own draw for the same column can be 30 times smaller
    # (seen: 8.1e-3 against < 5e-4 at an ulp of 0.03), so a column-by-column yardstick would be a coin toss.
    if n <= 2:
        kinds = [("", hard)]
    else:
        kinds = [(" constant", torch.zeros(d, dtype=torch.bool).index_fill_(0, torch.tensor([c["constant"]]), True))]
        if c["offset"] is not None:
            kinds.append((" 1e3-mean", torch.zeros(d, dtype=torch.bool).index_fill_(0, torch.tensor([c["offset"]]), True)))

    def both(name, got, r64, r32, bar64):
        """Fixed bar on the well-conditioned columns, the _close rule on the others, one kind of column at a time."""
        easy = ~hard
        if bool(easy.any()):
            within(name, got[..., easy.to(got.device)], r64[..., easy], bar64[..., easy] if torch.is_tensor(bar64) else bar64)
        for label, cols in kinds:
            bar = bar64[..., cols] if torch.is_tensor(bar64) else bar64
            within(name + " (hard columns%s)" % label, got[..., cols.to(got.device)], r64[..., cols], bar, r32[..., cols], report)

    for step in range(2):
        y64, gx64, gw64, gb64, rm64, rv64 = bn_restate(x, w0, b0, rm64, rv64, eps, mom, torch.float64, go)
        y32, gx32, gw32, gb32, rm32, rv32 = bn_restate(x, w0, b0, rm32, rv32, eps, mom, torch.float32, go)
        view, leaf, split = place_nan(x, c["layout"], dev, True)
        cs = None
        if c["colsums"] and step == 1:
            xd = x.double()
            cs = torch.stack([xd.sum(0), (xd * xd).sum(0)]).to(dev)
        yb = mine(view, colsums=cs)
        yb.backward(FF.place_cotangent(go, c["cot"], dev))
        both("y", yb, y64, y32, 2e-5)
        g, slack = split(leaf.grad)
        slack_is_zero("x", slack)
        both("x.grad", g, gx64, gx32, 2e-5 * max(1.0, gx64[:, ~hard].abs().max().item() if bool((~hard).any()) else 1.0))
        both("weight.grad", mine.weight.grad, gw64, gw32, 1e-4 * max(1.0, gw64.abs().max().item()))
        both("bias.grad", mine.bias.grad, gb64, gb32, 1e-4 * max(1.0, gb64.abs().max().item()))
        mine.weight.grad = mine.bias.grad = None
    both("running_mean", mine.running_mean, rm64, rm32, 1e-5)
    both("running_var", mine.running_var, rv64, rv32, 1e-6 + 1e-5 * rv64.abs())
    assert int(mine.num_batches_tracked) == 2
    # the eval form: the raw kernel without autograd, _AffineCols with it
    mine.eval()

    def eval_restate(dtype):
        xx, w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w0, b0))
        rm, rv = (rm64, rv64) if dtype == torch.float64 else (rm32, rv32)
        y = affine_form(xx, rm.to(dtype), rv.to(dtype), w, b, eps, dtype)
        y.backward(go.to(dtype))
        return [t.detach() for t in (y, xx.grad, w.grad, b.grad)]
    (y64, gx64, gw64, gb64), (y32, gx32, gw32, gb32) = eval_restate(torch.float64), eval_restate(torch.float32)
    view, leaf, split = place_nan(x, c["layout"], dev, True)
    with torch.no_grad():
        both("eval y", mine(view), y64, y32, 2e-5)
    ye = mine(view)
    assert type(ye.grad_fn).__name__ == _AffineCols.__name__ + "Backward"
    ye.backward(go.to(dev))
    both("eval y (autograd)", ye, y64, y32, 2e-5)
    g, slack = split(leaf.grad)
    slack_is_zero("eval x", slack)
    both("eval x.grad", g, gx64, gx32, 2e-5 * max(1.0, gx64.abs().max().item()))
    both("eval weight.grad", mine.weight.grad, gw64, gw32, 1e-4 * max(1.0, gw64.abs().max().item()))
    both("eval bias.grad", mine.bias.grad, gb64, gb32, 1e-4 * max(1.0, gb64.abs().max().item()))


@pytest.mark.parametrize("block", range(4))
def test_batchnorm_sweep_under_the_guard(dev, monkeypatch, block):
    report = []
    with guarded(monkeypatch) as guard:
        for k in range(block * 4, block * 4 + 4):
            c = bn_case(k)
            try:
                run_bn_case(dev, c, report)
            except (AssertionError, RuntimeError) as exc:
                raise type(exc)(f"{c}: {exc}") from exc
        finish(guard)
    for name, err, own in report:
        print(f"MEASURED bn block={block} {name}: error {err:.3e}, float32 restatement off by {own:.3e}")


# ---- loss -----------------------------------------------------------------------------------------------------------------

LOSS_C = [1, 3, 4, 8, 12, 20, 36, 64, 65, 128, 132, 256, 260, 300]
LOSS_N = [1, 63, 64, 65, 257, 1025]
LOSS_MASKS = [None, "bool", "uint8", "none selected"]
LOSS_LAYOUTS = [("fresh",), ("block", "pad", 4, 1), ("block", "pad", 1, 1), ("offset", 1), ("block", "2F", 0, 1)]
LOSS_CASES = 28
BLOCKED_CASES = [(C, B) for C in (8, 64, 256) for B in (1, 2, 4)]


def loss_case(k):
    return {"k": k, "C": LOSS_C[k % 14], "N": LOSS_N[(k + k // 14) % 6], "mask": LOSS_MASKS[(k + k // 4) % 4],
            "layout": LOSS_LAYOUTS[(k + k // 5) % 5], "reduction": ("mean", "sum")[(k // 2) % 2],
            "upstream": (1.7, -0.5)[k % 2]}


def blocked_case(j):
    C, B = BLOCKED_CASES[j]
    return {"j": j, "C": C, "B": B, "bias": j % 2 == 0, "N": LOSS_N[(j + 1) % 6], "mask": LOSS_MASKS[j % 3]}


def loss_data(N, C, mask_kind, seed):
    """Logits (two equal maxima in some rows, the label the second), labels (-1, C and 2**40 among them), mask."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, C, generator=gen) * 3
    y = torch.randint(0, C, (N,), generator=gen)
    rows = torch.randperm(N, generator=gen)
    ties = []
    if C >= 2:
        for r in rows[:max(1, N // 8)].tolist():
            j = sorted(torch.randperm(C, generator=gen)[:2].tolist())
            z[r, j[0]] = z[r, j[1]] = z[r].max() + 1.0
            y[r] = j[1]
            ties.append((r, j[0], j[1]))
    odd = [-1, C, 2 ** 40]
    for i, r in enumerate(rows[max(1, N // 8):max(1, N // 8) + (3 if N >= 8 else 0)].tolist()):
        y[r] = odd[i]
    if N == 1 and seed % 3 == 0:
        y[0] = odd[seed % 2]
    if mask_kind is None:
        mask = None
    elif mask_kind == "none selected":
        mask = torch.zeros(N, dtype=torch.bool)
    else:
        mask = torch.rand(N, generator=gen) < 0.6
        if mask_kind == "uint8":
            mask = mask.to(torch.uint8)
    return z, y, mask, ties


def loss_reference(z64, y, mask):
    """(selected rows, nll sum, count, arg-max hits (the first maximum, as argmax on the CPU takes it))."""
    C = z64.size(1)
    sel = (y >= 0) & (y < C)
    if mask is not None:
        sel = sel & mask.bool()
    logp = torch.log_softmax(z64, 1)
    nll = -logp[sel, y[sel]].sum()
    hits = int((z64[sel].argmax(1) == y[sel]).sum())
    return sel, nll, int(sel.sum()), hits


def sum_bar(count):
    """|nll sum - float64| of the parity tests is 1e-2 over 5000 rows; here per selected row a handful of float32
    roundings at magnitudes up to 16 (1e-5), and never more than the parity tests' bar."""
    return min(1e-2, 1e-5 * max(count, 1))


def run_loss_case(dev, c):
    from rgb_experiment_amd import ops
    N, C, red, up = c["N"], c["C"], c["reduction"], c["upstream"]
    z, y, mask, _ = loss_data(N, C, c["mask"], 300 + c["k"])
    yd, md = y.to(dev), None if mask is None else mask.to(dev)
    z64 = z.double().requires_grad_(True)
    sel, nll64, count, hits = loss_reference(z64, y, mask)
    ref = nll64 / count if red == "mean" and count else (nll64 * NAN if red == "mean" else nll64)
    if count:
        (ref * up).backward()
        g64 = z64.grad
    else:
        g64 = torch.zeros(N, C, dtype=torch.float64)   # what torch gives for an empty selection
    # cross-entropy from the logits, with statistics and backward
    view, leaf, split = place_nan(z, c["layout"], dev, True)
    loss, stats = ops.masked_ce_loss(view, yd, md, reduction=red, with_stats=True)
    s = stats.tolist()
    assert s[1] == count and s[2] == hits, ("ce stats", s, count, hits)
    assert abs(s[0] - nll64.item()) <= sum_bar(count), ("ce nll sum", s[0], nll64.item())
    if count or red == "sum":
        assert abs(loss.item() - ref.item()) < 1e-4 * max(1.0, abs(ref.item())), ("ce loss", loss.item(), ref.item())
    else:
        assert math.isnan(loss.item()), ("ce loss over no row", loss.item())
    (loss * up).backward()
    g, slack = split(leaf.grad)
    slack_is_zero("logits", slack)
    within("ce grad", g, g64, 1e-6 * max(1.0, g64.abs().max().item() * 10))
    assert not bool(g[~sel.to(dev)].any()), "ce grad: a row outside the selection is not zero"
    one = ops.masked_ce_accuracy(view.detach(), yd, md).tolist()
    assert one[1:] == [count, hits] and abs(one[0] - nll64.item()) <= sum_bar(count), ("ce accuracy", one)
    # the two-step route through log-probabilities
    logp32 = torch.log_softmax(z.double(), 1).float()
    lp64 = logp32.double().requires_grad_(True)
    nll2 = -lp64[sel, y[sel]].sum()
    hits2 = int((lp64[sel].argmax(1) == y[sel]).sum())
    ref2 = nll2 / count if red == "mean" and count else (nll2 * NAN if red == "mean" else nll2)
    if count:
        (ref2 * up).backward()
        gl64 = lp64.grad
    else:
        gl64 = torch.zeros(N, C, dtype=torch.float64)
    view, leaf, split = place_nan(logp32, c["layout"], dev, True)
    got = ops.masked_nll_loss(view, yd, md, reduction=red)
    if count or red == "sum":
        bar = 1e-5 if red == "mean" else sum_bar(count)
        assert abs(got.item() - ref2.item()) < bar, ("nll loss", got.item(), ref2.item())
    else:
        assert math.isnan(got.item()), ("nll loss over no row", got.item())
    (got * up).backward()
    g, slack = split(leaf.grad)
    slack_is_zero("logp", slack)
    within("nll grad", g, gl64, 1e-6)
    two = ops.masked_nll_accuracy(view.detach(), yd, md).tolist()
    assert two[1:] == [count, hits2] and abs(two[0] - nll2.item()) <= sum_bar(count), ("nll accuracy", two)


def run_blocked_case(dev, c):
    from rgb_experiment_amd import ops
    N, C, B = c["N"], c["C"], c["B"]
    z, y, mask, ties = loss_data(N, C, c["mask"], 900 + c["j"])
    bias = None
    if c["bias"]:
        # multiples of 1/4, and the tied logits moved so that logit + bias is one integer in both columns: the float32
        # sums the kernel forms are exact there, and the two maxima stay equal
        bias = torch.round(torch.randn(C, generator=torch.Generator().manual_seed(c["j"])) * 4) / 4
        for r, j0, j1 in ties:
            top = math.ceil(float((z[r] + bias).max())) + 1.0
            z[r, j0], z[r, j1] = top - bias[j0], top - bias[j1]
    full = (z if bias is None else z + bias).double()   # the kernel adds the bias in float32: the same sums
    _, nll64, count, hits = loss_reference(full, y, mask)
    blk = F0._to_blocked(z.to(dev), B)
    if (C // B) % 4:   # C = 8 in four blocks: the entry point takes block widths that are multiples of 4, and says so
        with pytest.raises(RuntimeError, match="block width % 4 == 0"):
            ops.masked_ce_accuracy_blocked(blk, y.to(dev), None if mask is None else mask.to(dev),
                                           None if bias is None else bias.to(dev))
        return
    got = ops.masked_ce_accuracy_blocked(blk, y.to(dev), None if mask is None else mask.to(dev),
                                         None if bias is None else bias.to(dev)).tolist()
    assert got[1:] == [count, hits] and abs(got[0] - nll64.item()) <= sum_bar(count), ("blocked", got, nll64.item(), count, hits)


@pytest.mark.parametrize("block", range(4))
def test_loss_sweep_under_the_guard(dev, monkeypatch, block):
    with guarded(monkeypatch) as guard:
        for k in range(block * 7, block * 7 + 7):
            c = loss_case(k)
            try:
                run_loss_case(dev, c)
            except (AssertionError, RuntimeError) as exc:
                raise type(exc)(f"{c}: {exc}") from exc
        for j in range(len(BLOCKED_CASES)):
            if j % 4 == block:
                c = blocked_case(j)
                try:
                    run_blocked_case(dev, c)
                except (AssertionError, RuntimeError) as exc:
                    raise type(exc)(f"{c}: {exc}") from exc
        finish(guard)


# ---- GEMM -----------------------------------------------------------------------------------------------------------------

GEMM_M = [1, 63, 64, 65, 128, 129]
GEMM_N = [1, 127, 128, 129, 260]
GEMM_K = [0, 1, 31, 32, 33, 511, 512, 513, 1025, 4096, 4099]
GEMM_CASES = 22
ROW_LISTS = ["empty", "all", "one", 31, 32, 33]
GEMM_ROWS_CASES = 6
GEMM_BN_CASES = 4


def gemm_bar(K):
    return 1e-5 + 8e-6 * K ** 0.5    # test_gemm_tn


def gemm_case(k):
    M, N = GEMM_M[(k + k // 11) % 6], GEMM_N[k % 5]
    form = lambda w, i: ("padded" if (k + i) % 3 else "fresh") if w % 4 else ("fresh", "block")[(k + i) % 2]
    return {"k": k, "K": GEMM_K[k % 11], "M": M, "N": N, "a": form(M, 0), "b": form(N, 1),
            "alpha": (1.0, 0.5, -1.0)[k % 3], "colsum": k % 4 != 3, "views": k % 3 != 1}


def gemm_rows_case(j):
    return {"j": j, "K": (600, 33, 513, 1025, 4096, 4099)[j], "M": (64, 128)[j % 2], "N": (128, 260)[(j // 2) % 2],
            "rows": ROW_LISTS[j], "colsum": j % 2 == 0}


def gemm_bn_case(j):
    return {"j": j, "K": (33, 513, 1025, 4099)[j], "M": (64, 128)[j % 2], "N": (128, 260)[(j // 2) % 2], "colsum": j % 2 == 1}


def gemm_operand(t, form, dev):
    """fresh | the [:, :w] view of a buffer with 16-byte rows whose pad columns hold NaN (w % 4 != 0) | a column block."""
    K, w = t.shape
    if form == "fresh":
        return t.to(dev)
    if form == "padded":
        base = torch.full((K, (w + 3) // 4 * 4), NAN, device=dev)
    else:
        base = torch.full((K, w + 8), NAN, device=dev)
    base[:, :w] = t.to(dev)
    return base[:, :w]


def run_gemm_case(dev, c):
    from rgb_experiment_amd import ops
    K, M, N = c["K"], c["M"], c["N"]
    rng = random.Random(c["k"])
    gen = torch.Generator().manual_seed(500 + c["k"])
    a, b = torch.randn(K, M, generator=gen), torch.randn(K, N, generator=gen)
    want = c["alpha"] * (a.double().t() @ b.double())
    want_sums = a.double().sum(0)
    ad, bd = gemm_operand(a, c["a"], dev), gemm_operand(b, c["b"], dev)
    kw, checks = {}, []
    if c["views"]:
        kw["out"], chk = out_view((M, N), dev, rng)
        checks.append(chk)
        if c["colsum"]:
            kw["sums_out"], chk = out_view((M,), dev, rng)
            checks.append(chk)
    res = ops.gemm_tn(ad, bd, alpha=c["alpha"], colsum=c["colsum"], **kw)
    got, sums = res if c["colsum"] else (res, None)
    if c["views"]:
        assert got.data_ptr() == kw["out"].data_ptr()
    for chk in checks:
        chk("gemm_tn")
    within("a^T b", got, want, gemm_bar(K))
    if sums is not None:
        within("column sums", sums, want_sums, gemm_bar(K))


def run_gemm_rows_case(dev, c):
    from rgb_experiment_amd import ops
    K, M, N = c["K"], c["M"], c["N"]
    gen = torch.Generator().manual_seed(700 + c["j"])
    a, b = torch.randn(K, M, generator=gen), torch.randn(K, N, generator=gen)
    if c["rows"] == "empty":
        rows = torch.zeros(0, dtype=torch.int64)
    elif c["rows"] == "all":
        rows = torch.arange(K)
    elif c["rows"] == "one":
        rows = torch.tensor([K - 1])
    else:   # inside one slab: consecutive staged tiles of the operand
        start = int(torch.randint(0, 200, (1,), generator=gen))
        rows = start + torch.randperm(64, generator=gen)[:c["rows"]].sort()[0]
    keep = torch.zeros(K, dtype=torch.bool)
    keep[rows] = True
    a0, b0 = a * keep[:, None], b * keep[:, None]
    an, bn = a.clone(), b.clone()
    an[~keep], bn[~keep] = NAN, NAN           # the rows the list leaves out are never read
    rd = rows.to(torch.int32).to(dev)
    res = ops.gemm_tn_rows(an.to(dev), bn.to(dev), rd, colsum=c["colsum"], rows_only=True)
    full = ops.gemm_tn(a0.to(dev), b0.to(dev), colsum=c["colsum"])
    got, sums = res if c["colsum"] else (res, None)
    fgot, fsums = full if c["colsum"] else (full, None)
    assert torch.equal(got, fgot), "row-list product differs from the product over the zeroed operands"
    within("a^T b over the rows", got, a0.double().t() @ b0.double(), gemm_bar(K))
    if sums is not None:
        assert torch.equal(sums, fsums), "row-list column sums differ"
        within("column sums over the rows", sums, a0.double().sum(0), gemm_bar(K))


def run_gemm_bn_case(dev, c):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import batchnorm as B
    K, M, N = c["K"], c["M"], c["N"]
    gen = torch.Generator().manual_seed(800 + c["j"])
    g, x, b = (torch.randn(K, w, generator=gen).to(dev) for w in (M, M, N))
    # coefficients that keep the transformed operand at the unit scale test_gemm_tn's bar is for: gx = g + O(0.1)
    mean, ca, cb = (torch.randn(M, generator=gen).to(dev) * 0.1 for _ in range(3))
    rstd, ck = (torch.rand(M, generator=gen).to(dev) * 0.2 + 0.9 for _ in range(2))
    got, sums = ops.gemm_tn_bn_bwd(g, x, mean, rstd, ca, cb, ck, b, colsum=c["colsum"])
    gx = B.bwd_apply(g, x, mean, rstd, ca, cb, ck)
    two = ops.gemm_tn(gx, b, colsum=c["colsum"])
    want, want_sums = two if c["colsum"] else (two, None)
    assert torch.equal(got, want), "the fused form differs from bwd_apply followed by gemm_tn"
    if c["colsum"]:
        assert torch.equal(sums, want_sums)
    g64 = (g.cpu().double() - ca.cpu().double() - (x.cpu().double() - mean.cpu().double()) * rstd.cpu().double()
           * cb.cpu().double()) * ck.cpu().double()
    assert g64.pow(2).mean().sqrt().item() < 1.25
    within("bn_bwd product", got, g64.t() @ b.cpu().double(), gemm_bar(K))


@pytest.mark.parametrize("block", range(4))
def test_gemm_sweep_under_the_guard(dev, monkeypatch, block):
    jobs = [(run_gemm_case, gemm_case(k)) for k in range(GEMM_CASES) if k % 4 == block]
    jobs += [(run_gemm_rows_case, gemm_rows_case(j)) for j in range(GEMM_ROWS_CASES) if j % 4 == block]
    jobs += [(run_gemm_bn_case, gemm_bn_case(j)) for j in range(GEMM_BN_CASES) if j % 4 == block]
    with guarded(monkeypatch) as guard:
        for fn, c in jobs:
            try:
                fn(dev, c)
            except (AssertionError, RuntimeError) as exc:
                raise type(exc)(f"{fn.__name__} {c}: {exc}") from exc
        finish(guard)


# ---- rows and operands ----------------------------------------------------------------------------------------------------

ROWS_D = [1, 4, 7, 132]
FOLD_SIZES = [1, 31, 32, 33, 65]
FOLD_CASES = 10


def fold_case(k):
    return {"k": k, "n_out": FOLD_SIZES[k % 5], "K": FOLD_SIZES[(2 * k + k // 5) % 5], "wide": k % 2 == 0,
            "root": k % 3 != 0, "bias": (k // 2) % 2 == 0, "bias2": k % 4 == 1, "bn": k % 5 != 4}


def run_rows_case(dev, d):
    from rgb_experiment_amd import ops
    rng = random.Random(d)
    gen = torch.Generator().manual_seed(40 + d)
    n = 301
    src = torch.randn(n, d, generator=gen)
    lay = LAYOUTS[d % len(LAYOUTS)]
    for idx in (torch.zeros(0, dtype=torch.int64), torch.randint(0, n, (517,), generator=gen),
                torch.randperm(n, generator=gen)[:200]):
        view = place_nan(src, lay, dev)[0]
        id32 = idx.to(torch.int32).to(dev)
        got = ops.gather_rows(view, id32)
        assert torch.equal(got.cpu(), src[idx]), ("gather_rows", d, idx.numel())
        if idx.numel():
            out, untouched = out_view((idx.numel(), d), dev, rng)
            assert ops.gather_rows(view, id32, out=out).data_ptr() == out.data_ptr()
            untouched("gather_rows")
            assert torch.equal(out.cpu(), src[idx]), ("gather_rows out=", d)
    for idx in (torch.zeros(0, dtype=torch.int64), torch.randperm(n, generator=gen)[:200]):
        rows = torch.randn(idx.numel(), d, generator=gen)
        dst0 = torch.randn(n, d, generator=gen)
        dst, untouched = out_view((n, d), dev, rng)
        dst.copy_(dst0)
        ops.scatter_add_rows(place_nan(rows, lay, dev)[0], idx.to(torch.int32).to(dev), dst)
        untouched("scatter_add_rows")
        want = dst0.clone()
        want[idx] += rows          # unique indices: one float32 addition per element
        assert torch.equal(dst.cpu(), want), ("scatter_add_rows", d, idx.numel())
    # blocked -> rows (+ bias), the width a multiple of the block count
    for B in (1, 2, 4):
        cols = {1: 4, 4: 8, 7: 12, 132: 132}[d]     # (the entry point takes block widths that are multiples of 4)
        m = torch.randn(n, B * cols, generator=gen)
        bias = torch.randn(B * cols, generator=gen) if B != 2 else None
        blk = F0._to_blocked(m.to(dev), B)
        want = m if bias is None else m + bias
        assert torch.equal(ops.blocked_to_rows(blk, bias=None if bias is None else bias.to(dev)).cpu(), want), ("blocked_to_rows", d, B)
        out, untouched = out_view((n, B * cols), dev, rng, aligned=True)
        ops.blocked_to_rows(blk, out=out, bias=None if bias is None else bias.to(dev))
        untouched("blocked_to_rows")
        assert torch.equal(out.cpu(), want), ("blocked_to_rows out=", d, B)


def run_fold_case(dev, c):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import BatchNorm1d
    n_out, K = c["n_out"], c["K"]
    g = torch.Generator().manual_seed(60 + c["k"])
    W, Wr = torch.randn(n_out, K, generator=g), torch.randn(n_out, K, generator=g)
    b, b2 = torch.randn(n_out, generator=g), torch.randn(n_out, generator=g)
    lay = ("block", "pad", 3, 0) if c["wide"] else ("fresh",)     # W as a view with ld > K
    Wd, Wrd = place_nan(W, lay, dev)[0], place_nan(Wr, lay, dev)[0]
    bn = None
    scale, shift = torch.ones(n_out, dtype=torch.float64), torch.zeros(n_out, dtype=torch.float64)
    if c["bn"]:
        bn = BatchNorm1d(n_out).eval()
        with torch.no_grad():
            bn.weight.copy_(torch.rand(n_out, generator=g) + 0.5)
            bn.bias.copy_(torch.rand(n_out, generator=g) * 2 - 1)
            bn.running_mean.copy_(torch.rand(n_out, generator=g) * 2 - 1)
            bn.running_var.copy_(torch.rand(n_out, generator=g) * 2.8 + 0.2)
        scale = bn.weight.detach().double() * torch.rsqrt(bn.running_var.double() + bn.eps)
        shift = bn.bias.detach().double() - bn.running_mean.double() * scale
        bn.to(dev)
    wt, bo, wrt = ops.fold_bn_linear(Wd, b.to(dev) if c["bias"] else None, b2.to(dev) if c["bias2"] else None,
                                     root_weight=Wrd if c["root"] else None, bn=bn)
    close = lambda got, want, rtol, atol: within("fold", got, want, atol + rtol * want.abs())
    close(wt, (W.double() * scale[:, None]).t(), 1e-6, 1e-7)          # test_fold_bn_linear_operands' bars
    assert wt.is_contiguous() and tuple(wt.shape) == (K, n_out)
    if c["root"]:
        close(wrt, (Wr.double() * scale[:, None]).t(), 1e-6, 1e-7)
    else:
        assert wrt is None
    if c["bias"] or c["bias2"] or c["bn"]:
        total = (b.double() if c["bias"] else 0) + (b2.double() if c["bias2"] else 0)
        close(bo, total * scale + shift, 1e-5, 1e-6)
    else:
        assert bo is None
    if not c["bn"]:
        assert torch.equal(wt.cpu(), W.t().contiguous()), "without a BatchNorm: the plain transpose"


@pytest.mark.parametrize("d", ROWS_D)
def test_rows_sweep_under_the_guard(dev, monkeypatch, d):
    with guarded(monkeypatch) as guard:
        run_rows_case(dev, d)
        for k in range(FOLD_CASES):
            if k % len(ROWS_D) == ROWS_D.index(d):
                c = fold_case(k)
                try:
                    run_fold_case(dev, c)
                except (AssertionError, RuntimeError) as exc:
                    raise type(exc)(f"{c}: {exc}") from exc
        finish(guard)


# ---- graph preparation ------------------------------------------------------------------------------------------------------

SMALL_CSR_CASES = [c for c in CSR_CASES if c[0] <= 1000] + [(3, 4000, 10, 100)]   # the last: rows past LONG_ROW_SLOTS


def split_restated(rowptr, T):
    """graph.make_row_split in plain Python."""
    deg = (rowptr[1:] - rowptr[:-1]).tolist()
    begin, end, row, long_row, ptr = [], [], [], [], [0]
    for i, dg in enumerate(deg):
        if dg > T:
            long_row.append(i)
            for s in range(int(rowptr[i]), int(rowptr[i + 1]), T):
                begin.append(s)
                end.append(min(s + T, int(rowptr[i + 1])))
                row.append(i)
            ptr.append(len(begin))
    return None if not long_row else {"chunk_begin": begin, "chunk_end": end, "chunk_row": row, "long_row": long_row,
                                      "long_chunk_ptr": ptr, "n_chunks": len(begin), "n_long": len(long_row), "threshold": T}


def run_graph_case(dev, n, e, loops, dups, mode, weighted):
    from rgb_experiment_amd import graph as G
    ei = rand_graph(n, e, seed=n + e, loops=loops, dups=dups)
    ew = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(e)) + 0.25 if weighted else None
    G.clear_cache()
    eid = ei.to(dev)
    g = G.get_graph(eid, n, mode, None if ew is None else ew.to(dev))
    rei, ids = O.rewrite_edges(ei, n, mode)
    E2 = rei.size(1)
    if ew is None:
        wts = torch.ones(E2, dtype=torch.float64)
    elif mode == G.LOOPS_KEEP:
        wts = ew.double()
    elif mode == G.LOOPS_ADD_REMAINING:
        wts = O.add_remaining_self_loops(ei, ew.double(), 1.0, n)[1]
    else:
        wts = torch.cat([ew.double()[ei[0] != ei[1]], torch.ones(n, dtype=torch.float64)])
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, rei[1], wts)
    dis = deg.pow(-0.5)
    dis[torch.isinf(dis)] = 0
    w_edge = dis[rei[0]] * wts * dis[rei[1]]
    for name, csr, agg, other, wname in (("fwd", g.fwd, rei[1], rei[0], "w"), ("bwd", g.bwd, rei[0], rei[1], "w_t")):
        rowptr, col, perm = O.csr_from_edges(agg, other, ids, n)
        assert csr.nnz == E2, name
        assert torch.equal(csr.rowptr.cpu(), rowptr), (name, "rowptr")
        assert torch.equal(csr.col.cpu()[:csr.nnz], col), (name, "col")
        assert torch.equal(csr.perm.cpu()[:csr.nnz], perm), (name, "perm")
        want_split = split_restated(rowptr.long(), G.LONG_ROW_SLOTS)
        assert (csr.split is None) == (want_split is None), (name, "split")
        if want_split is not None:
            for key, val in want_split.items():
                have = csr.split[key]
                assert (have.cpu().tolist() if torch.is_tensor(have) else have) == val, (name, "split", key)
        slot = O.csr_from_edges(agg, other, torch.arange(E2), n)[2].long()
        # test_norm_vectors: 1e-7; test_weighted_gcn_norm_matches_the_oracle: 1e-6 of the entry, a zero exactly zero
        within(wname, getattr(g, wname)[:csr.nnz], w_edge[slot], 1e-6 * w_edge[slot].abs() if weighted else 1e-7)
    if not weighted:
        cnt = (O.csr_from_edges(rei[1], rei[0], ids, n)[0].long().diff()).clamp(min=1).float()
        assert torch.equal(g.inv_deg.cpu()[:n], 1.0 / cnt), "inv_deg"
        if g.bwd.nnz:
            assert torch.equal(g.w_mean_t.cpu()[:g.bwd.nnz], (1.0 / cnt)[g.bwd.col.cpu()[:g.bwd.nnz].long()]), "w_mean_t"
    within("dis", g.dis[:n], dis, 1e-6 * dis.abs() if weighted else 1e-7)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_graph_preparation_under_the_guard(dev, monkeypatch, mode):
    with guarded(monkeypatch) as guard:
        for n, e, loops, dups in SMALL_CSR_CASES:
            for weighted in (False, True):
                try:
                    run_graph_case(dev, n, e, loops, dups, mode, weighted)
                except (AssertionError, RuntimeError) as exc:
                    raise type(exc)(f"n={n} e={e} mode={mode} weighted={weighted}: {exc}") from exc
        finish(guard)
