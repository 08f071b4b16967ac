"""bfloat16 storage of the gathered matrix on the MI355X: the conversion kernel bit for bit against the CPU's
tensor.to(torch.bfloat16), rgbx_spmm_csr_bf16 against the float64 oracle (oracle/ref_cpu.py: propagate) evaluated on the
WIDENED bfloat16 inputs, its bfloat16 output, hub rows, ops.propagate_rows_bf16's autograd contract, the three layers and two
models built with gather_dtype, and experiment().

Bars. After widening (exact: bits << 16) the kernel's arithmetic is the fp32 gather's, so against the oracle ON THE ROUNDED
INPUTS the bar is tests/test_gpu_parity.py's: TOL = 1e-4 * max(1, max|want|). Against the UNROUNDED float64 oracle the
rounding comes on top. bfloat16 keeps 8 significant bits; rounding to nearest moves a value v by at most u |v| with
u = 2^-8 (tests/test_bf16_host.py pins both the constant and that truncation would break it). The gather is linear, so with
D = bf16(h) - h, |D| <= u |h| elementwise:
    |P bf16(h) - P h| = |P D| <= |P| |D| <= u |P| |h|                                     (forward, P the aggregation)
    |P^T bf16(g) - P^T g| <= u |P^T| |g|                                                  (backward, g = dL/dout)
A dense product behind or in front of the gather carries the bound through in absolute values — for an elementwise
error bound B on a matrix M: |(M + E) W^T - M W^T| <= B |W|^T, |(M + E)^T x - M^T x| <= B^T |x| — which gives per layer
(W the weight the gathered half goes through, h = x W^T (+ b_l where the bias sits inside the mean), z = g W):
    in > out  (transform, round, gather):  out: u |P||h|       g_x: (u |P^T||g|) |W|     g_W: (u |P^T||g|)^T |x|
                                           g_b_l (MySAGEConv, inside the mean): column sums of u |P^T||g|
    in <= out (round, gather, transform):  out: (u |P||x|) |W|^T    g_x: u |P^T||z|      g_W: |g|^T (u |P||x|)
Everything that does not pass through the rounded matrix (the root product, the biases outside the mean) has bound 0.
Each comparison allows that bound PLUS the fp32 bar TOL of its quantity; no other constant enters."""
import re

import pytest
import torch

from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
U = 2.0 ** -8
WIDTHS = [8, 24, 64, 128, 256]
KINDS = ["gcn", "mean", "sum"]
N = 300
DEGS = [0, 1, 63, 64, 65, 200, 62, 199]  # slots of the first rows as given; with one self-loop added: 1, 2, 64, 65, 66, 201, 63, 200
# event kinds of launches that gather neighbour rows (the plain dense product records 'linear_fwd', the fused
# aggregate + transform forms '<kind>_linear_fwd' / 'cached_aggregate_linear_fwd')
GATHER = re.compile(r"(^|_)(gcn|mean|sum)_(fwd|bwd)|_linear_fwd|^spmm")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bar(want):
    return TOL * max(1.0, want.abs().max().item())


def bits16(t):
    return t.cpu().contiguous().view(torch.int16)


def degree_graph(seed=3, n=N, degs=DEGS, rest=2500):
    """Rows 0..len(degs)-1 with exactly degs[i] in-edges (no self-loops among them), the others random (some stay empty)."""
    g = torch.Generator().manual_seed(seed)
    k = len(degs)
    src = torch.cat([torch.randint(k, n, (m,), generator=g) for m in degs])
    dst = torch.cat([torch.full((m,), i, dtype=torch.int64) for i, m in enumerate(degs)])
    rnd = torch.randint(k, n, (2, rest), generator=g)
    rnd = rnd[:, rnd[1] % 11 != 0]  # rows without any slot
    ei = torch.cat([torch.stack([src, dst]), rnd], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=g)]


MODE = {"gcn": 1, "mean": 0, "sum": 0}


@pytest.fixture(scope="module")
def cases(dev):
    """Per kind: the device graph, the rewritten edge list and the per-edge weights of the oracle — made once, read-only."""
    from rgb_experiment_amd.graph import Graph
    ei = degree_graph()
    out = {}
    for kind in KINDS:
        g = Graph(ei.to(dev), N, MODE[kind])
        if kind == "gcn":
            rei, w = O.gcn_norm(ei, None, N)
        else:
            rei, _ = O.rewrite_edges(ei, N, MODE[kind])
            w = None
            if kind == "mean":
                w = (1.0 / torch.bincount(rei[1], minlength=N).clamp(min=1).float())[rei[1]]
        out[kind] = (g, rei, w)
    lens = (out["sum"][0].fwd.rowptr[1:] - out["sum"][0].fwd.rowptr[:-1]).cpu()
    assert lens[:len(DEGS)].tolist() == DEGS and (lens == 0).sum() > 1
    return out


def oracle_P(rei, w, m, transposed=False):
    """float64 P m (or P^T m) over the oracle's edge list; `m` may be |m| and w |w| for the bound."""
    e = rei.flip(0) if transposed else rei
    return O.propagate(e, m.double(), N, None if w is None else w.double(), "add")


# ---- conversion ----------------------------------------------------------------------------------------------------------

SPECIAL_BITS = [
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,              # +-0, +-inf
    0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF812345,  # NaNs: quiet, signalling payloads
    0x00000001, 0x80000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x807FFFFF,  # fp32 subnormals
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000,              # the largest finite fp32 (-> inf), around the last tie
    0x3F808000, 0xBF808000, 0x3F818000, 0xBF818000,              # exactly halfway: lower neighbour even, then odd
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00800000, 0x3F800000, 0x477FE000,
]


def special_values(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, d, generator=g) * torch.tensor(10.0).pow(torch.randint(-20, 20, (n, 1), generator=g).float())
    sp = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in SPECIAL_BITS], dtype=torch.int32).view(torch.float32)
    flat = t.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:4 * sp.numel()]
    flat[pos] = sp.repeat(4)[:pos.numel()]
    return t


@pytest.mark.parametrize("d", [8, 24, 64, 256, 7, 1, 12])
def test_conversion_matches_the_cpu_bit_for_bit(dev, d):
    from rgb_experiment_amd import ops
    t = special_values(97, d, d)
    got = ops.to_bf16_rows(t.to(dev))
    assert got.dtype == torch.bfloat16 and got.shape == t.shape and got.is_contiguous()
    assert torch.equal(bits16(got), bits16(t.to(torch.bfloat16)))


def test_conversion_reads_column_slices_and_takes_empty_input(dev):
    from rgb_experiment_amd import ops
    base = special_values(131, 48, 1)
    bd = base.to(dev)
    for c0, c1 in ((8, 32), (0, 40), (3, 10), (4, 12), (16, 48)):  # on and off the 16-byte grid, lds = 48 > d
        got = ops.to_bf16_rows(bd[:, c0:c1])
        assert torch.equal(bits16(got), bits16(base[:, c0:c1].contiguous().to(torch.bfloat16))), (c0, c1)
    assert torch.equal(bits16(ops.to_bf16_rows(bd[5:6, 8:16])), bits16(base[5:6, 8:16].contiguous().to(torch.bfloat16)))
    for shape in ((0, 8), (0, 5), (4, 0)):
        empty = ops.to_bf16_rows(torch.empty(shape, device=dev))
        assert empty.shape == shape and empty.dtype == torch.bfloat16
    with pytest.raises(RuntimeError, match="float32"):
        ops.to_bf16_rows(bd.to(torch.bfloat16))


# ---- the raw gather against the oracle on the widened inputs -----------------------------------------------------------------

@pytest.fixture(scope="module")
def table():
    """[N, 256] N(0,1) features, their CPU rounding, and the widened values the oracle reads (made once)."""
    x = torch.randn(N, 256, generator=torch.Generator().manual_seed(11))
    xb = x.to(torch.bfloat16)
    return x, xb, xb.float()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_gather_forward_and_transposed(dev, cases, table, kind, d):
    from rgb_experiment_amd import ops
    g, rei, w = cases[kind]
    _, xb, xw = table
    xbd = xb[:, :d].contiguous().to(dev)
    for transposed, csr in ((False, g.fwd), (True, g.bwd)):
        ws, rs = ops._kind_weights(g, kind, transposed)
        got = ops.spmm_bf16_raw(csr, ws, rs, xbd, kind="probe_bf16")
        assert got.dtype == torch.float32 and got.shape == (N, d)
        want = oracle_P(rei, w, xw[:, :d], transposed)
        assert (got.cpu().double() - want).abs().max().item() < bar(want), (kind, d, transposed)
        if ws is not None:  # the same rows without per-slot weights
            plain = ops.spmm_bf16_raw(csr, None, None, xbd)
            want1 = oracle_P(rei, None, xw[:, :d], transposed)
            assert (plain.cpu().double() - want1).abs().max().item() < bar(want1)


@pytest.mark.parametrize("d", WIDTHS)
def test_gather_epilogue_slices_and_aliasing(dev, cases, table, d):
    """a, rs, w, b * y with b != 1, bias, out aliasing y, and all three fp32 / bf16 matrices as column slices (ld > d)."""
    from rgb_experiment_amd import ops
    g, rei, w = cases["gcn"]
    _, xb, xw = table
    gen = torch.Generator().manual_seed(d)
    rs, bias, y = torch.rand(N, generator=gen) + 0.5, torch.randn(d, generator=gen), torch.randn(N, d, generator=gen)
    wide_x = torch.zeros(N, d + 16, dtype=torch.bfloat16)
    wide_x[:, 8:8 + d] = xb[:, :d]
    wide_y = torch.full((N, d + 12), 7.0)
    wide_y[:, 4:4 + d] = y
    wyd = wide_y.to(dev)
    xs, ys = wide_x.to(dev)[:, 8:8 + d], wyd[:, 4:4 + d]
    want = 0.7 * rs.double()[:, None] * oracle_P(rei, w, xw[:, :d]) - 1.3 * y.double() + bias.double()
    wide_o = torch.full((N, d + 8), -3.0, device=dev)
    got = ops.spmm_bf16_raw(g.fwd, g.w, rs.to(dev), xs, y=ys, a=0.7, b=-1.3, bias=bias.to(dev), out=wide_o[:, 8:])
    assert got.data_ptr() == wide_o[:, 8:].data_ptr()
    assert (got.cpu().double() - want).abs().max().item() < bar(want)
    assert torch.equal(wide_o[:, :8].cpu(), torch.full((N, 8), -3.0))  # nothing beyond the slice is written
    again = ops.spmm_bf16_raw(g.fwd, g.w, rs.to(dev), xs, y=ys, a=0.7, b=-1.3, bias=bias.to(dev), out=ys)  # out aliases y
    assert torch.equal(again, got)
    assert again.data_ptr() == ys.data_ptr()
    assert torch.equal(wyd[:, :4], ys.new_full((N, 4), 7.0)) and torch.equal(wyd[:, 4 + d:], ys.new_full((N, 8), 7.0))


def test_gather_beyond_256_columns_runs_in_blocks(dev, cases):
    from rgb_experiment_amd import ops
    g, rei, w = cases["gcn"]
    x = torch.randn(N, 520, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    got = ops.spmm_bf16_raw(g.fwd, g.w, None, x.to(dev))
    want = oracle_P(rei, w, x.float())
    assert (got.cpu().double() - want).abs().max().item() < bar(want)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.spmm_bf16_raw(g.fwd, g.w, None, x.to(dev)[:, :12].contiguous())
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.spmm_bf16_raw(g.fwd, g.w, None, x.to(dev).float())


@pytest.mark.parametrize("d", WIDTHS)
def test_bf16_output_is_the_fp32_output_rounded(dev, cases, table, d):
    """out_bf16 == out.to(torch.bfloat16) of the SAME launch's arithmetic, also when only out_bf16 is written; rows that
    overflow to inf, gather an inf or a NaN included."""
    from rgb_experiment_amd import _lib, ops
    g, _, _ = cases["sum"]
    _, xb, _ = table
    x = xb[:, :d].clone()
    hot = torch.unique(g.fwd.col[:g.fwd.nnz].cpu().long())[:3].tolist()  # three rows that some target does gather
    x[hot[0]] = torch.finfo(torch.bfloat16).max
    x[hot[1], ::2] = float("nan")
    x[hot[2], 1::2] = float("-inf")
    xd = x.to(dev)
    rs = torch.full((N,), 1.003, device=dev)  # bf16 max * 1.003 is finite in fp32 and beyond the last bf16 tie
    out = torch.empty(N, d, device=dev)
    both = torch.empty(N, d, dtype=torch.bfloat16, device=dev)
    lib, csr = _lib.load(), g.fwd
    args = (csr.rowptr.data_ptr(), csr.col.data_ptr(), None, rs.data_ptr(), xd.data_ptr(), d, None, 0, None)
    _lib.check(lib.rgbx_spmm_csr_bf16(*args, out.data_ptr(), d, both.data_ptr(), d, N, d, 1.0, 0.0, None,
                                      _lib.stream_ptr()), "rgbx_spmm_csr_bf16")
    only = ops.spmm_bf16_raw(csr, None, rs, xd, out_dtype=torch.bfloat16)
    f32 = ops.spmm_bf16_raw(csr, None, rs, xd)
    assert torch.equal(f32.view(torch.int32), out.view(torch.int32))  # same bits with and without the second output
    o = out.cpu()
    assert torch.isinf(o).any() and torch.isnan(o).any() and torch.isfinite(o).any()
    want = bits16(o.to(torch.bfloat16))
    assert torch.equal(bits16(both), want)
    assert only.dtype == torch.bfloat16 and torch.equal(bits16(only), want)


# ---- hub rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [24, 64, 256])
def test_hub_rows_split_reproducible_and_equal_to_unsplit(dev, table, monkeypatch, d):
    """One row above the threshold (200 slots against 199; the 199-slot row stays whole), forward and — on the flipped
    graph — in the transposed CSR."""
    from rgb_experiment_amd import graph as G
    from rgb_experiment_amd import ops
    ei = degree_graph()
    _, xb, xw = table
    xbd = xb[:, :d].contiguous().to(dev)
    gen = torch.Generator().manual_seed(d)
    w_e = torch.rand(ei.size(1), generator=gen) + 0.5
    runs = {}
    for threshold in (199, 10 ** 9):
        monkeypatch.setattr(G, "LONG_ROW_SLOTS", threshold)
        for flipped in (False, True):
            e = ei.flip(0) if flipped else ei
            g = G.Graph(e.to(dev), N, 0)
            csr = g.bwd if flipped else g.fwd  # either way: rows = ei's targets, the hub among them
            assert (csr.split is not None) == (threshold == 199)
            if csr.split is not None:
                assert csr.split["n_long"] == 1 and csr.split["n_chunks"] == 2
            ws = w_e.to(dev)[csr.perm[:csr.nnz].long()]
            for weights in (ws, None):
                got = ops.spmm_bf16_raw(csr, weights, None, xbd)
                assert torch.equal(got, ops.spmm_bf16_raw(csr, weights, None, xbd))  # two launches: the same bits
                want = oracle_P(ei, None if weights is None else w_e, xw[:, :d])
                assert (got.cpu().double() - want).abs().max().item() < bar(want)
                runs[(threshold, flipped, weights is None)] = (got, bar(want))
    for (threshold, flipped, plain), (got, tol) in runs.items():
        if threshold == 199:
            assert (got - runs[(10 ** 9, flipped, plain)][0]).abs().max().item() < tol


# ---- propagate_rows_bf16: one autograd node ----------------------------------------------------------------------------------

class Sink(list):
    def kinds(self):
        return [str(k) for k, _, _ in self]


@pytest.fixture
def sink():
    from rgb_experiment_amd import ops
    s = Sink()
    ops.set_event_sink(s)
    yield s
    ops.set_event_sink(None)


@pytest.mark.parametrize("addend,with_bias", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("kind", KINDS)
def test_propagate_rows_bf16_autograd(dev, cases, sink, kind, addend, with_bias):
    from rgb_experiment_amd import ops
    g, rei, w = cases[kind]
    n = 24
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(N, 2 * n if addend else n, generator=gen)
    bias = torch.randn(n, generator=gen) if with_bias else None
    go = torch.randn(N, n, generator=gen)
    hd = h.to(dev).requires_grad_(True)
    bd = None if bias is None else bias.to(dev).requires_grad_(True)
    out = ops.propagate_rows_bf16(hd, g, kind, n=n, bias=bd)
    assert sink.kinds() == ["rows_to_bf16", f"{kind}_fwd_bf16"]
    out.backward(go.to(dev))
    assert sink.kinds()[2:] == ["rows_to_bf16", f"{kind}_bwd_bf16"]
    left = h[:, :n]
    want = oracle_P(rei, w, left) + (h[:, n:].double() if addend else 0) + (bias.double() if with_bias else 0)
    wabs = None if w is None else w.abs()
    assert ((out.detach().cpu().double() - want).abs() <= U * oracle_P(rei, wabs, left.abs()) + bar(want)).all()
    want_g = oracle_P(rei, w, go, transposed=True)
    got_g = hd.grad.cpu().double()
    assert ((got_g[:, :n] - want_g).abs() <= U * oracle_P(rei, wabs, go.abs(), transposed=True) + bar(want_g)).all()
    if addend:
        assert (got_g[:, n:] - go.double()).abs().max().item() < bar(go)
    if with_bias:
        assert (bd.grad.cpu().double() - go.double().sum(0)).abs().max().item() < bar(go.double().sum(0))
    # the rounding is real: the same launch on fp32 rows gives other numbers
    assert not torch.equal(out.detach(), ops.propagate_rows(hd.detach(), g, kind, n=n, bias=None if bd is None else bd.detach()))


def test_passes_nobody_asks_for_do_not_launch(dev, cases, sink):
    from rgb_experiment_amd import ops
    g, _, _ = cases["mean"]
    gen = torch.Generator().manual_seed(6)
    h, bias, go = torch.randn(N, 16, generator=gen).to(dev), torch.randn(8, generator=gen).to(dev), torch.randn(N, 8).to(dev)
    b = bias.clone().requires_grad_(True)
    ops.propagate_rows_bf16(h, g, "mean", n=8, bias=b).backward(go)  # only the bias takes a gradient
    assert sink.kinds() == ["rows_to_bf16", "mean_fwd_bf16"] and b.grad is not None
    del sink[:]
    hg = h.clone().requires_grad_(True)
    ops.propagate_rows_bf16(hg, g, "mean", n=8, bias=bias).backward(go)  # only h does
    assert sink.kinds() == ["rows_to_bf16", "mean_fwd_bf16", "rows_to_bf16", "mean_bwd_bf16"] and hg.grad is not None
    del sink[:]
    with torch.no_grad():
        ops.propagate_bf16(h[:, :5], g, "sum")  # padded to 8 columns inside
    assert sink.kinds() == ["rows_to_bf16", "sum_fwd_bf16"]


def test_partitioned_graphs_are_refused(dev):
    from rgb_experiment_amd import ops

    class Partitioned:
        is_distributed = True
    with pytest.raises(NotImplementedError, match="partitioned"):
        ops.propagate_rows_bf16(torch.zeros(4, 8, device=dev), Partitioned(), "gcn")


# ---- layers ----------------------------------------------------------------------------------------------------------------

LAYERS = ["GCNConv", "SAGEConv", "MySAGEConv"]
SHAPES = [(40, 16), (12, 40), (20, 7)]  # in > out, in < out (12 columns: padded to 16 for the gather), out = 7 padded to 8


def dense_P(ei, name):
    """The layer's aggregation as a dense float64 matrix (out = P @ x), from the oracle's own propagate."""
    eye = torch.eye(N, dtype=torch.float64)
    if name == "GCNConv":
        rei, w = O.gcn_norm(ei, None, N)
        return O.propagate(rei, eye, N, w.double(), "add")
    rei, _ = O.rewrite_edges(ei, N, 2 if name == "MySAGEConv" else 0)
    return O.propagate(rei, eye, N, None, "mean")


def oracle_layer(name, x, ei, p):
    if name == "GCNConv":
        return O.gcn_conv(x, ei, p["lin.weight"], p["bias"])
    if name == "SAGEConv":
        return O.sage_conv(x, ei, p["lin_l.weight"], p["lin_l.bias"], p["lin_r.weight"])
    return O.my_sage_conv(x, ei, p["lin_l.weight"], p["lin_l.bias"], p["lin_r.weight"], p["lin_r.bias"])


@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("name", LAYERS)
def test_layers_against_the_float64_oracle(dev, sink, name, cin, cout):
    """Output, input gradient and parameter gradients within the bound derived in the module docstring (u |P||.| carried
    through the dense products in absolute values) plus the fp32 bar; only *_bf16 gathers run; the fp32 layer differs."""
    from rgb_experiment_amd import nn as RN
    from rgb_experiment_amd.graph import clear_cache
    ei = degree_graph(seed=cin + cout)
    gen = torch.Generator().manual_seed(cin * 100 + cout)
    x, go = torch.randn(N, cin, generator=gen), torch.randn(N, cout, generator=gen)
    torch.manual_seed(cin + 3)
    conv = getattr(RN, name)(cin, cout, gather_dtype="bf16")
    with torch.no_grad():
        for prm in conv.parameters():
            if prm.dim() == 1:
                prm.uniform_(-1, 1)
    plain = getattr(RN, name)(cin, cout)
    plain.load_state_dict(conv.state_dict())
    p64 = {k: v.detach().clone().double().requires_grad_(True) for k, v in conv.state_dict().items()}
    x64 = x.double().requires_grad_(True)
    want = oracle_layer(name, x64, ei, p64)
    want.backward(go.double())

    conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev))
    fwd_kinds = sink.kinds()
    out.backward(go.to(dev))
    gathers = [k for k in sink.kinds() if GATHER.search(k)]
    kind = "gcn" if name == "GCNConv" else "mean"
    assert gathers == [f"{kind}_fwd_bf16", f"{kind}_bwd_bf16"] and f"{kind}_fwd_bf16" in fwd_kinds, sink.kinds()

    P = dense_P(ei, name)
    Pa, g64, xa = P.abs(), go.double(), x.double().abs()
    wkey = "lin.weight" if name == "GCNConv" else "lin_l.weight"
    W = p64[wkey].detach()
    bound = {k: torch.zeros_like(v) for k, v in p64.items()}
    if cin > cout:
        h = x.double() @ W.t()
        if name == "MySAGEConv":
            h = h + p64["lin_l.bias"].detach()  # inside the mean: rounded with the rows
        b_out = U * (Pa @ h.abs())
        b_gh = U * (Pa.t() @ g64.abs())
        b_gx, bound[wkey] = b_gh @ W.abs(), b_gh.t() @ xa
        if name == "MySAGEConv":
            bound["lin_l.bias"] = b_gh.sum(0)
    else:
        b_z = U * (Pa @ xa)
        b_out = b_z @ W.abs().t()
        b_gx = U * (Pa.t() @ (g64 @ W).abs())
        bound[wkey] = g64.abs().t() @ b_z
    w_d = want.detach()
    assert out.shape == (N, cout)
    assert ((out.detach().cpu().double() - w_d).abs() <= b_out + bar(w_d)).all()
    assert ((xd.grad.cpu().double() - x64.grad).abs() <= b_gx + bar(x64.grad)).all()
    for k, prm in conv.named_parameters():
        assert prm.grad is not None and prm.grad.shape == p64[k].shape
        assert ((prm.grad.cpu().double() - p64[k].grad).abs() <= bound[k] + bar(p64[k].grad)).all(), k

    del sink[:]
    plain.to(dev)
    with torch.no_grad():
        ref32 = plain(x.to(dev), ei.to(dev))
        again = conv(x.to(dev), ei.to(dev))
    assert torch.equal(again, out.detach())  # the inference forward: the same launches, the same bits
    assert (ref32.cpu().double() - w_d).abs().max().item() < bar(w_d)
    assert not torch.equal(ref32, out.detach())
    clear_cache()


def test_layer_refusals_on_the_device(dev):
    from rgb_experiment_amd.nn import GCNConv
    ei = degree_graph().to(dev)
    conv = GCNConv(16, 8, gather_dtype="bf16").to(dev)
    x = torch.randn(N, 16, device=dev)
    ew = torch.rand(ei.size(1), device=dev) + 0.5
    with pytest.raises(ValueError, match="edge_weight"):
        conv(x, ei, ew.clone().requires_grad_(True))
    out = conv(x, ei, ew)  # a constant weight only changes the graph's per-slot weights
    rei, w = O.gcn_norm(ei.cpu(), ew.cpu(), N)
    W, b = conv.lin.weight.detach().cpu().double(), conv.bias.detach().cpu().double()
    h = x.cpu().double() @ W.t()
    want = O.propagate(rei, h, N, w.double(), "add") + b
    assert ((out.detach().cpu().double() - want).abs() <= U * O.propagate(rei, h.abs(), N, w.double().abs(), "add")
            + bar(want)).all()


# ---- models ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["GCN", "GraphSAGE2"])
def test_models_run_only_bf16_gathers_and_keep_their_loss_contract(dev, sink, name):
    from rgb_experiment_amd import models, ops
    ei = degree_graph(seed=8).to(dev)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(N, 20, generator=gen).to(dev)
    y = torch.randint(0, 5, (N,), generator=gen).to(dev)
    mask_a, mask_b = (torch.rand(N, generator=gen) < 0.5).to(dev), (torch.rand(N, generator=gen) < 0.3).to(dev)
    torch.manual_seed(1)
    net = getattr(models, name)(num_layers=2, hidden_unit=32, input_dim=20, output_dim=5, dropout_rate=0.5,
                                gather_dtype="bf16").to(dev)
    banned = re.compile(r"_linear_fwd$|^gcn_fwd$|^mean_fwd$")

    def check(kinds, backward):
        gathers = [k for k in kinds if GATHER.search(k)]
        assert gathers and all(k.endswith("_bf16") for k in gathers), kinds
        assert not [k for k in kinds if banned.search(k)], kinds
        assert any(k.endswith("_bwd_bf16") for k in gathers) == backward, kinds

    net.train()
    loss, stats = net.masked_ce(x, ei, y, mask_a)
    check(sink.kinds(), False)
    del sink[:]
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    check(sink.kinds(), True)
    del sink[:]
    logits = net(x, ei)["emb"]
    loss2, stats2 = ops.ce_from_logits(logits, y, mask_a)
    assert torch.equal(loss.detach(), loss2.detach()) and torch.equal(stats, stats2)  # BatchNorm on batch statistics both times
    check(sink.kinds(), False)

    net.eval()
    with torch.no_grad():
        del sink[:]
        logits = net(x, ei)["emb"]
        check(sink.kinds(), False)
        del sink[:]
        loss, stats = net.masked_ce(x, ei, y, mask_a)
        pair = net.masked_ce_pair(x, ei, y, mask_a, mask_b)
        check(sink.kinds(), False)
        want_a, want_b = ops.masked_ce_accuracy(logits, y, mask_a), ops.masked_ce_accuracy(logits, y, mask_b)
        assert torch.equal(stats, want_a) and torch.equal(pair, torch.stack([want_a, want_b]))
        assert loss is None or torch.equal(loss, (want_a[0] / want_a[1]).float())


# ---- experiment() ------------------------------------------------------------------------------------------------------------

def toy_data(n=240, f=12, c=3, seed=4):
    import rgb_experiment_amd as R
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, c, (n,), generator=g)
    x = torch.randn(n, f, generator=g) + torch.nn.functional.one_hot(y, f).float() * 2
    return R.Data(x=x, y=y, edge_index=torch.randint(0, n, (2, 5 * n), generator=g))


def test_experiment_takes_the_keyword_and_none_changes_nothing(dev):
    import rgb_experiment_amd as R
    data = toy_data()
    init = {"num_layers": 2, "hidden_unit": 64, "dropout_rate": 0.5}
    kw = dict(specify_data=True, data=data, model_name="gcn", learning_rate=0.01, epoch=3, need_to_reappear=True,
              print_print=False, return_model=True, implement_early_stopping=False, need_all_metrics=False)
    a = R.experiment(dict(init, gather_dtype="bf16"), **kw)
    assert all(c.gather_dtype is torch.bfloat16 for c in a["model"].convs)
    losses = a["history"]["train_loss"]
    assert len(losses) == 3 and all(torch.isfinite(torch.as_tensor(float(v))) for v in losses)
    b = R.experiment(dict(init, gather_dtype="bf16"), **kw)
    assert a["history"] == b["history"]  # same seed: bit-identical curves
    default = R.experiment(dict(init), **kw)
    explicit = R.experiment(dict(init, gather_dtype=None), **kw)
    assert default["history"] == explicit["history"]
    assert all(c.gather_dtype is None for c in default["model"].convs)
    assert default["history"] != a["history"]
    for k, v in default["model"].state_dict().items():
        assert torch.equal(v, explicit["model"].state_dict()[k]), k
