"""rgbx_gemm_tn_rows_f32 with the list entries fetched one tile ahead of their rows: ops.gemm_tn_rows against ops.gemm_tn
on the operand with the other rows zeroed, product and column sums bit for bit. The lists put zero, one and two tiles of
look-ahead and a ragged last tile inside one K-slab (K = 5000 rows: 10 slabs of 512)."""
import pytest
import torch

from rgb_experiment_amd import ops

pytestmark = pytest.mark.gpu

K = 5000
SLAB = 512  # choose_splits: ceil(K / 512) = 10 slabs, each ceil(500 / 32) * 32 rows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _lists():
    g = torch.Generator().manual_seed(3)
    out = {"p60": (torch.rand(K, generator=g) < 0.6).nonzero().reshape(-1), "one": torch.tensor([2345]),
           "empty": torch.zeros(0, dtype=torch.int64),
           "last_slab": torch.arange(9 * SLAB + 3, K, 2)}
    for n in (31, 32, 33, 65):  # inside slab 1 = rows [512, 1024)
        out[f"slab1_{n}"] = SLAB + 5 + 7 * torch.arange(n)
    return out


@pytest.fixture(scope="module")
def operands(dev):
    g = torch.Generator().manual_seed(1)
    return torch.randn(K, 128, generator=g).to(dev), torch.randn(K, 128, generator=g).to(dev)


@pytest.mark.parametrize("M,N", [(128, 128), (64, 128), (32, 40)])
def test_rows_form_equals_plain_product_on_zeroed_operand(dev, operands, M, N):
    a_full, b_full = operands
    b = b_full[:, :N].contiguous()
    for name, rows in _lists().items():
        assert rows.numel() == 0 or (int(rows.max()) < K and bool((rows[1:] > rows[:-1]).all()))
        a = torch.zeros(K, M, device=dev)
        a[rows.to(dev)] = a_full[rows.to(dev), :M]
        want, want_sums = ops.gemm_tn(a, b, colsum=True)
        got, got_sums = ops.gemm_tn_rows(a, b, rows.to(dev).to(torch.int32), colsum=True)
        assert torch.equal(got, want), name
        assert torch.equal(got_sums, want_sums), name
