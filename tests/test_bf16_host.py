"""bfloat16 storage of the gathered matrix on the host: the C ABI's new entries (truth table, argument checks before any
launch, exports), the `gather_dtype` keyword of GCNConv / SAGEConv / MySAGEConv / GCN / GraphSAGE / GraphSAGE2 with every
refusal and every switched-off shortcut, and the error arithmetic tests/test_gpu_bf16.py relies on. No GPU needed.

The arithmetic: bfloat16 keeps 8 significant bits, so rounding to nearest changes a value by at most 2^-8 of its
magnitude (half a unit in the last place) and truncation by up to 2^-7. A weighted gather is linear in the gathered rows,
hence |P round(h) - P h| <= 2^-8 |P| |h| elementwise — pinned below against float64 on inputs where truncation breaks the
same bound (the bound is tight enough to tell the two apart)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("rgbx_spmm_csr_bf16_supported", "rgbx_spmm_csr_bf16", "rgbx_rows_f32_to_bf16")
U_BF16 = 2.0 ** -8  # unit roundoff of bfloat16, round to nearest


def _lib():
    from rgb_experiment_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L, L.load()


# ---- C ABI -------------------------------------------------------------------------------------------------------------

def test_supported_truth_table():
    _, lib = _lib()
    for d in (8, 24, 64, 256):
        assert lib.rgbx_spmm_csr_bf16_supported(d), d
    for d in (0, 4, 12, 260, 264):
        assert not lib.rgbx_spmm_csr_bf16_supported(d), d


def test_gather_argument_errors_come_before_any_launch():
    """Fake, never dereferenced pointers (as tests/test_abi.py): every rejected call returns from the host checks."""
    _, lib = _lib()
    p, q = 0x10000, 0x20000  # 16-byte aligned, non-null (q: an out_bf16 that does not alias x)

    def call(x=p, ldx=8, y=None, ldy=0, bias=None, out=p, ldo=8, ob=None, ldob=0, N=10, d=8, rowptr=p, col=p):
        return lib.rgbx_spmm_csr_bf16(rowptr, col, None, None, x, ldx, y, ldy, bias, out, ldo, ob, ldob, N, d, 1.0, 0.0,
                                      None, None)
    assert call(x=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert call(rowptr=None) == -1 and call(col=None) == -1
    assert call(out=None) == -1 and b"out" in lib.rgbx_last_error_string()      # no output at all
    assert call(ldx=4) == -1                                                       # ldx < d
    assert call(ldo=4) == -1 and call(out=None, ob=q, ldob=4) == -1
    assert call(y=p, ldy=4) == -1
    assert call(N=-1) == -1
    assert call(ldx=12) == -3                                                      # ldx % 8
    assert call(out=None, ob=q, ldob=12) == -3
    assert call(x=p + 2) == -3 and call(x=p + 8) == -3                             # misaligned x
    assert call(out=None, ob=q + 8, ldob=8) == -3
    assert call(out=None, ob=p, ldob=8) == -1 and call(out=None, ob=q, ldob=8, N=0) == 0          # out_bf16 aliasing x
    assert call(y=p + 4, ldy=8) == -3 and call(out=p + 8) == -3 and call(bias=p + 4) == -3
    assert call(ldo=10) == -3
    assert call(d=12, ldx=16, ldo=12) == -5 and b"8" in lib.rgbx_last_error_string()
    assert call(d=4, ldx=8) == -5 and call(d=264, ldx=264, ldo=264) == -5
    assert call(N=0) == 0                                                          # nothing to do
    assert call(N=0, x=None, out=None) == 0
    from rgb_experiment_amd._lib import RowSplit
    sp = RowSplit(4, 3, 1, p, p, p, p, p, None)                                    # a plan without its partial buffer
    assert lib.rgbx_spmm_csr_bf16(p, p, None, None, p, 8, None, 0, None, p, 8, None, 0, 10, 8, 1.0, 0.0, ctypes.byref(sp),
                                  None) == -1
    sp = RowSplit(4, 3, 1, p, p, p, p, p, p + 4)
    assert lib.rgbx_spmm_csr_bf16(p, p, None, None, p, 8, None, 0, None, p, 8, None, 0, 10, 8, 1.0, 0.0, ctypes.byref(sp),
                                  None) == -3


def test_conversion_argument_errors_come_before_any_launch():
    _, lib = _lib()
    p = 0x10000
    cvt = lib.rgbx_rows_f32_to_bf16
    assert cvt(None, 8, p, 8, 10, 8, None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert cvt(p, 8, None, 8, 10, 8, None) == -1
    assert cvt(p, 4, p, 8, 10, 8, None) == -1      # lds < d
    assert cvt(p, 8, p, 4, 10, 8, None) == -1      # ldd < d
    assert cvt(p, 8, p, 8, -1, 8, None) == -1
    assert cvt(p + 2, 8, p, 8, 10, 8, None) == -3  # a float on a 2-byte boundary
    assert cvt(p, 8, p + 1, 8, 10, 8, None) == -3
    assert cvt(p, 8, p, 8, 0, 8, None) == 0        # n = 0: nothing to do
    assert cvt(None, 8, None, 8, 0, 8, None) == 0
    assert cvt(p, 8, p, 8, 10, 0, None) == 0


def test_exports_and_header():
    L, lib = _lib()
    text = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS and name in L.SIGNATURES
        assert hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert len(L.SIGNATURES["rgbx_spmm_csr_bf16"]) == 19
    assert len(L.SIGNATURES["rgbx_rows_f32_to_bf16"]) == 7
    assert lib.rgbx_version() == 501
    assert "spmm_bf16.hip" in open(os.path.join(ROOT, "rgb_experiment_amd", "csrc", "Makefile")).read()


def test_mat_stays_fp32_only_and_bf16_has_its_own_helper():
    L, _ = _lib()
    t = torch.zeros(3, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32"):
        L.mat(t)
    with pytest.raises(RuntimeError, match="bfloat16"):
        L.mat_bf16(torch.zeros(3, 16))
    assert L.mat_bf16(t) == (t.data_ptr(), 16)
    assert L.mat_bf16(t[:, :8]) == (t.data_ptr(), 16)  # a column slice keeps the leading dimension
    with pytest.raises(RuntimeError, match="contiguous"):
        L.mat_bf16(t.t())


def test_ops_refuse_wrong_dtypes_widths_and_cpu_tensors():
    from rgb_experiment_amd import ops
    for name in ("to_bf16_rows", "spmm_bf16_raw", "propagate_rows_bf16", "propagate_bf16", "pad_rows8"):
        assert hasattr(ops, name), name
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.spmm_bf16_raw(None, None, None, torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="HIP|CPU fallback"):
        ops.to_bf16_rows(torch.zeros(4, 8))
    with pytest.raises(ValueError, match="kind"):
        ops.propagate_rows_bf16(torch.zeros(4, 8), None, "max")
    w, b, n = ops.pad_rows8(torch.ones(7, 3), torch.ones(7))
    assert n == 8 and tuple(w.shape) == (8, 3) and tuple(b.shape) == (8,)
    assert torch.equal(w[7], torch.zeros(3)) and b[7] == 0 and torch.equal(w[:7], torch.ones(7, 3))
    w16 = torch.ones(16, 3)
    assert ops.pad_rows8(w16)[0] is w16 and ops.pad_rows8(w16)[-1] == 16

    class FakeDist:
        is_distributed = True
    with pytest.raises(NotImplementedError, match="partitioned"):
        ops.propagate_rows_bf16(torch.zeros(4, 8), FakeDist(), "gcn")
    with pytest.raises(NotImplementedError, match="partitioned"):
        ops.propagate_bf16(torch.zeros(4, 8), FakeDist(), "mean")


# ---- the keyword ---------------------------------------------------------------------------------------------------------

FLAGS = ("accepts_ce", "accepts_ce_pair", "emits_colsums", "owns_next_bn_backward")


def _layers():
    from rgb_experiment_amd.nn import GCNConv, MySAGEConv, SAGEConv
    return GCNConv, SAGEConv, MySAGEConv


@pytest.mark.parametrize("value", [torch.bfloat16, "bf16", "bfloat16"])
def test_accepted_values_select_bfloat16(value):
    for cls in _layers():
        conv = cls(12, 5, gather_dtype=value)
        assert conv.gather_dtype is torch.bfloat16


@pytest.mark.parametrize("value", ["fp16", "float32", torch.float16, torch.float32, 16, True, ["bf16"], ("bf16",), ""])
def test_other_values_are_refused(value):
    for cls in _layers():
        with pytest.raises(ValueError, match="gather_dtype"):
            cls(12, 5, gather_dtype=value)


def test_keyword_is_the_last_constructor_argument_and_defaults_to_none():
    import inspect
    from rgb_experiment_amd.models import GCN, GraphSAGE, GraphSAGE2
    for cls in _layers() + (GCN, GraphSAGE, GraphSAGE2):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "gather_dtype" and params[-1].default is None, cls


@pytest.mark.parametrize("aggr", ["max", "min", "add", "sum", "std", "var", ["mean"], ["mean", "max"]])
def test_refused_together_with_another_aggregation(aggr):
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    with pytest.raises(ValueError):
        SAGEConv(12, 5, aggr=aggr, gather_dtype="bf16")
    if isinstance(aggr, str):
        with pytest.raises(ValueError, match="gather_dtype"):
            MySAGEConv(12, 5, aggr=aggr, gather_dtype="bf16")
    assert SAGEConv(12, 5, aggr="mean", gather_dtype="bf16").aggr == "mean"


def test_state_dict_is_the_fp32_layers():
    for cls in _layers():
        torch.manual_seed(5)
        a = cls(12, 5)
        torch.manual_seed(5)
        b = cls(12, 5, gather_dtype="bf16")
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype == torch.float32 and torch.equal(sa[k], sb[k]), k  # same draws, too
        a.load_state_dict(sb)


def test_shortcuts_are_off_per_instance_and_default_layers_keep_theirs():
    from rgb_experiment_amd.models._stack import _layer_maps
    today = {"folds_post_affine": True, "emits_colsums": True, "owns_next_bn_backward": True, "accepts_ce": True,
             "accepts_ce_pair": True, "gather_dtype": None}
    for cls in _layers():
        plain, conv = cls(6, 16), cls(6, 16, gather_dtype="bf16")
        for flag in FLAGS:
            assert getattr(conv, flag) is False, (cls, flag)
            assert flag not in vars(plain)  # a default-built layer sets nothing on the instance
        for flag, value in today.items():
            assert getattr(cls, flag) is value and getattr(plain, flag) is value, (cls, flag)
        assert "gather_dtype" not in vars(plain)
        assert _layer_maps(conv) is None and _layer_maps(plain) is not None
        assert conv.eval_operands() is None and plain.eval_operands is not None
        x, ei = torch.zeros(4, 6), torch.tensor([[0, 1], [1, 2]])
        assert conv.aggregate_input(x, ei) is None
        assert conv.forward_folded(x, ei, (None, None, None)) is None


def test_models_pass_the_keyword_to_every_conv():
    from rgb_experiment_amd import models
    from rgb_experiment_amd.models import GCN, GraphSAGE, GraphSAGE2
    for cls in (GCN, GraphSAGE, GraphSAGE2):
        for value in (torch.bfloat16, "bf16", "bfloat16"):
            net = cls(num_layers=3, hidden_unit=16, input_dim=10, output_dim=4, dropout_rate=0.5, gather_dtype=value)
            assert [c.gather_dtype for c in net.convs] == [torch.bfloat16] * 3
            assert net._collapsed_operands() is None
            assert all(op is None for op in net._eval_operands())
        net = cls(num_layers=2, hidden_unit=16, input_dim=10, output_dim=4, dropout_rate=0.5)
        assert [c.gather_dtype for c in net.convs] == [None, None]
        with pytest.raises(ValueError, match="gather_dtype"):
            cls(num_layers=2, hidden_unit=16, input_dim=10, output_dim=4, dropout_rate=0.5, gather_dtype="half")
    with pytest.raises(ValueError):
        GraphSAGE2(2, 16, 10, 4, 0.5, aggr="max", gather_dtype="bf16")
    # the way experiment() builds a model: MODELS[name](input_dim=..., output_dim=..., **model_init_param)
    from rgb_experiment_amd.itexperiments import MODELS
    net = MODELS["gcn"](input_dim=10, output_dim=4, **{"num_layers": 2, "hidden_unit": 64, "dropout_rate": 0.5,
                                                       "gather_dtype": "bf16"})
    assert all(c.gather_dtype is torch.bfloat16 for c in net.convs)
    assert hasattr(models, "REGISTRY")


def test_registry_and_model_keys_are_unchanged():
    from rgb_experiment_amd import models
    from rgb_experiment_amd.itexperiments import MODELS
    for name in ("gcn", "graphsage", "graphsage2"):
        assert name in MODELS
    assert not [k for k in MODELS if "bf16" in k.lower() or "bfloat" in k.lower()]
    assert not [k for k in models.REGISTRY if "bf16" in str(k).lower() or "bfloat" in str(k).lower()]


def test_cpu_tensors_are_still_refused():
    for cls in _layers():
        conv = cls(4, 3, gather_dtype="bf16")
        with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback|HIP"):
            conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
        wide = cls(3, 4, gather_dtype="bf16")
        with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback|HIP"):
            wide(torch.randn(5, 3), torch.tensor([[0, 1], [1, 2]]))


def test_learned_edge_weight_is_refused_before_anything_runs():
    from rgb_experiment_amd.nn import GCNConv
    conv = GCNConv(4, 3, gather_dtype="bf16")
    ew = torch.ones(2, requires_grad=True)
    with pytest.raises(ValueError, match="edge_weight"):
        conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]), ew)


# ---- the error bound the GPU tests rely on ---------------------------------------------------------------------------------

def _truncate_bf16(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def test_rounding_keeps_the_gather_within_the_bound_and_truncation_does_not():
    """N = 300, d = 16, 12 in-edges per node, N(0,1) features and weights. This pins the TEST INPUTS (and the constant
    2^-8), not the product: whatever rounds to nearest passes, whatever truncates fails."""
    n, d, deg = 300, 16, 12
    g = torch.Generator().manual_seed(20)
    src = torch.randint(0, n, (n * deg,), generator=g)
    dst = torch.arange(n).repeat_interleave(deg)
    w = torch.randn(n * deg, generator=g)
    h = torch.randn(n, d, generator=g)

    def gather(m):
        return torch.zeros(n, d, dtype=torch.float64).index_add_(0, dst, w.double()[:, None] * m.double()[src])
    exact = gather(h)
    bound = U_BF16 * torch.zeros(n, d, dtype=torch.float64).index_add_(0, dst, w.double().abs()[:, None] * h.double().abs()[src])
    rounded = h.to(torch.bfloat16).float()
    truncated = _truncate_bf16(h)
    assert torch.equal(rounded.to(torch.bfloat16), h.to(torch.bfloat16))  # widening is exact
    r_round = ((gather(rounded) - exact).abs() / bound).max().item()
    r_trunc = ((gather(truncated) - exact).abs() / bound).max().item()
    print(f"max |error| / (2^-8 |P||h|): rounded {r_round:.3f}, truncated {r_trunc:.3f}")
    assert r_round <= 1.0
    assert r_trunc > 1.0
    # elementwise, the rounding itself: half a unit in the last place, and truncation up to a whole one
    assert ((rounded - h).abs() <= U_BF16 * h.abs()).all()
    assert ((truncated - h).abs() > U_BF16 * h.abs()).any()


def test_cpu_rounding_is_nearest_even_on_the_special_values():
    """What the conversion kernel is held to on the GPU, stated on the CPU: ties go to the even neighbour, the largest
    finite fp32 overflows to inf, NaN stays a quiet NaN."""
    bits = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0x00000001, 0x00008000, 0x7FC00000],
                        dtype=torch.int64).to(torch.int32)
    got = bits.view(torch.float32).to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    assert got[:7].tolist() == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x7F80, 0x0000, 0x0000]
    assert (int(got[7]) & 0x7FC0) == 0x7FC0  # exponent all ones and the quiet bit
