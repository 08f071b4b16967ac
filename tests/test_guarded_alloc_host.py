"""tests/_guarded_alloc.py on the CPU: what the guard hands out, what Guard.check() catches (the only place an
out-of-bounds write is staged on purpose: on CPU tensors, inside memory the test owns), which modules come under guard,
and that the draw tables of tests/test_gpu_guarded_alloc.py reach every size their kernels branch at."""
import importlib
import os
import pkgutil
import re
import sys

import pytest
import torch

import _guarded_alloc as GA
import test_gpu_guarded_alloc as T

DTYPES = [torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.bool]
SHAPES = [(5,), (1,), (3, 7), (2, 300), (4, 3, 8), (0, 6), (0,)]


def interior_is(t, dtype):
    if dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    want = {torch.bool: True, torch.uint8: 0xFF}.get(dtype, 0)
    return bool((t == want).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_what_the_guard_hands_out(dtype):
    guard = GA.Guard()
    for shape in SHAPES:
        t = guard.empty(shape, dtype=dtype)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t._base is None
        band = GA.band_elements(shape, t.element_size())
        assert band >= max(128, 2 * (shape[-1] if len(shape) >= 2 else 1))
        assert (band * t.element_size()) % 512 == 0
        # the CPU allocator aligns to 64 bytes, not 512: the offset from the base is what the guard decides
        assert t.storage_offset() == band and (t.storage_offset() * t.element_size()) % 512 == 0
        assert t.untyped_storage().nbytes() == (2 * band + t.numel()) * t.element_size()
        assert interior_is(t, dtype), (shape, t)
    assert guard.empty(2, 3, dtype=dtype).shape == (2, 3)
    like = guard.empty_like(torch.zeros(3, 4).t(), dtype=dtype)
    assert like.shape == (4, 3) and like.stride() == (1, 4) and interior_is(like, dtype)
    assert guard.empty_like(torch.zeros(6, 4)[:, :3], dtype=dtype).is_contiguous()
    strided = guard.empty_strided((3, 2), (4, 1), dtype=dtype)
    assert strided.stride() == (4, 1) and strided.storage_offset() % 128 == 0
    z = guard.zeros(4, 5, dtype=dtype)
    assert not bool(z.any()) and z.is_contiguous()
    assert not bool(guard.zeros_like(z).any()) and guard.zeros_like(z).dtype == dtype
    f = guard.full((7,), 1, dtype=dtype)
    assert bool((f == 1).all())
    assert guard.allocations == len(SHAPES) + 8
    assert guard.float_allocations == (guard.allocations if dtype.is_floating_point else 0)
    guard.check()


def test_keyword_arguments_and_defaults():
    guard = GA.Guard()
    assert guard.empty(3).dtype == torch.float32
    assert guard.full((2,), 1.5).dtype == torch.float32 and guard.full((2,), 3).dtype == torch.int64
    assert guard.full((2,), True).dtype == torch.bool
    assert guard.empty((2, 2), dtype=torch.float32, device="cpu", pin_memory=False,
                       memory_format=torch.contiguous_format).is_contiguous()
    assert guard.empty((2, 2), device=torch.device("cpu"), requires_grad=True).requires_grad
    assert guard.zeros_like(torch.ones(2, dtype=torch.float64), dtype=torch.float32).dtype == torch.float32
    site = [s for s in guard.counts() if s.startswith(os.path.join("tests", "test_guarded_alloc_host.py"))]
    assert len(site) == 6 and sum(guard.counts().values()) == 7, guard.counts()
    assert GA.per_module(guard.counts()) == {os.path.join("tests", "test_guarded_alloc_host.py"): 7}
    guard.check()


def _kernel(out, base_offset, how):
    """A CPU 'kernel' that writes next to the buffer it was given."""
    flat = torch.empty(0, dtype=out.dtype).set_(out.untyped_storage())
    if how == "before":
        flat[base_offset - 1] = 1
    elif how == "after":
        flat[base_offset + out.numel()] = 1
    else:   # one whole row past the end
        torch.as_strided(flat, (out.size(0) + 1, out.size(1)), (out.size(1), 1), base_offset)[-1] = 1
    return how


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64, torch.uint8, torch.bool],
                         ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("how,offset", [("before", -1), ("after", 12), ("row past the end", 12)])
def test_check_names_the_allocation_that_was_overrun(dtype, how, offset):
    guard = GA.Guard()
    quiet = guard.empty((5, 5), dtype=dtype)
    line = sys._getframe().f_lineno + 1
    out = guard.empty((3, 4), dtype=dtype)   # <- the call site the report must name
    _kernel(out, out.storage_offset(), how)
    with pytest.raises(AssertionError) as err:
        guard.check()
    text = str(err.value)
    assert "test_guarded_alloc_host.py:%d" % line in text and "(3, 4)" in text and str(dtype) in text, text
    assert "offset %d of the buffer" % offset in text, text
    assert ("4 band element" if how == "row past the end" else "1 band element") in text, text
    assert "(5, 5)" not in text and quiet is not None
    guard.check()   # the records are gone: a second check starts clean


def test_a_canonical_nan_in_a_band_is_seen():
    """What a kernel that strays with a NaN of its own stores differs from the band's NaN bit for bit."""
    guard = GA.Guard()
    out = guard.empty((4,), dtype=torch.float32)
    torch.empty(0).set_(out.untyped_storage())[out.storage_offset() + 4] = float("nan")
    with pytest.raises(AssertionError, match="offset 4 of the buffer"):
        guard.check()


def test_every_allocating_module_comes_under_the_guard(monkeypatch):
    """The module list is found, not typed. Every module whose source calls one of the three `empty` forms is in it
    (a module added later cannot escape), and it is exactly the set that calls one of the six."""
    import rgb_experiment_amd as pkg
    three, six = set(), set()
    for info in pkgutil.walk_packages(pkg.__path__, pkg.__name__ + "."):
        if info.name.startswith(pkg.__name__ + ".dist"):
            continue
        path = importlib.util.find_spec(info.name).origin
        src = open(path).read() if path and path.endswith(".py") else ""
        if re.search(r"torch\.(empty|empty_like|empty_strided)\(", src):
            three.add(info.name)
        if re.search(r"torch\.(empty|empty_like|empty_strided|zeros|zeros_like|full)\(", src):
            six.add(info.name)
    found = set(GA.allocating_modules())
    assert three and three <= found and found == six, (sorted(three - found), sorted(found ^ six))
    assert {"rgb_experiment_amd.ops", "rgb_experiment_amd.graph", "rgb_experiment_amd.nn.batchnorm", "rgb_experiment_amd.nn.conv",
            "rgb_experiment_amd.utils.edges", "rgb_experiment_amd.utils.mask"} == three
    with GA.guarded(monkeypatch) as guard:
        for name in found:
            mod = importlib.import_module(name)
            assert isinstance(mod.torch, GA.TorchProxy), name    # it names its allocator `torch`, and the proxy is in place
            assert mod.torch.Tensor is torch.Tensor and mod.torch.float32 is torch.float32
            assert isinstance(torch.ones(1), mod.torch.Tensor)
        assert guard.allocations == 0
    for name in found:
        assert importlib.import_module(name).torch is torch, name


def test_batchnorm_host_path_runs_clean_under_the_guard(monkeypatch):
    from rgb_experiment_amd.nn import BatchNorm1d
    from rgb_experiment_amd.nn import batchnorm as B
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(37, 5, generator=gen) * 2 + 1
    go = torch.randn(37, 5, generator=gen)
    ref, mine = torch.nn.BatchNorm1d(5), BatchNorm1d(5)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with GA.guarded(monkeypatch) as guard:
        ya, yb = ref(xa), mine(xb)
        ya.backward(go)
        yb.backward(go)
        ga, gb = xa.grad.clone(), xb.grad.clone()
        mine.eval(), ref.eval()
        ye = mine(xb)
        ye.sum().backward()    # _AffineCols: torch.zeros_like under the guard
        assert torch.allclose(ye, ref(xa), atol=1e-5)
        assert B.torch is not torch and guard.allocations >= 2, guard.counts()
        assert all(site.startswith(os.path.join("rgb_experiment_amd", "nn", "batchnorm.py")) for site in guard.counts())
        guard.check()
    assert torch.allclose(ya, yb, atol=1e-5) and torch.allclose(ga, gb, atol=1e-4)
    assert torch.allclose(mine.running_var, ref.running_var, atol=1e-5) and int(mine.num_batches_tracked) == 1


# ---- the draw tables of the GPU sweep ------------------------------------------------------------------------------------

def values(cases, key):
    return {c[key] for c in cases}


def test_the_sweep_draws_reach_every_listed_value():
    bn = [T.bn_case(k) for k in range(T.BN_CASES)]
    assert values(bn, "d") == {1, 3, 4, 7, 64, 132, 257, 1028} and values(bn, "n") == {1, 2, 15, 16, 17, 255, 257, 4097}
    assert values(bn, "colsums") == {True, False} and len(values(bn, "layout")) >= 5
    assert all(c["offset"] is not None for c in bn if c["d"] > 1)
    assert {c["layout"][0] for c in bn} == {"fresh", "block", "offset"}
    loss = [T.loss_case(k) for k in range(T.LOSS_CASES)]
    assert values(loss, "C") == {1, 3, 4, 8, 12, 20, 36, 64, 65, 128, 132, 256, 260, 300}
    assert values(loss, "N") == {1, 63, 64, 65, 257, 1025}
    assert values(loss, "mask") == {None, "bool", "uint8", "none selected"}
    assert values(loss, "reduction") == {"mean", "sum"} and all(c["upstream"] != 1 for c in loss)
    # logits as a column block with ld > C, aligned (vector kernels: C % 4 == 0, C <= 256) and one float off
    vec = [c for c in loss if c["C"] % 4 == 0 and c["C"] <= 256]
    assert {c["layout"] for c in vec} >= {("fresh",), ("block", "pad", 4, 1), ("block", "pad", 1, 1), ("offset", 1)}
    assert {c["layout"] for c in loss if c not in vec} >= {("fresh",), ("block", "pad", 4, 1), ("block", "pad", 1, 1)}
    for c in loss:   # every case holds a tied row with the label second, and (eight rows or more) the three odd labels
        z, y, _, ties = T.loss_data(c["N"], c["C"], c["mask"], 300 + c["k"])
        assert (c["C"] < 2) or all(z[r, a] == z[r, b] == z[r].max() and a < b and (y[r] == b or c["N"] == 1)
                                   for r, a, b in ties) and ties
        assert c["N"] < 8 or {-1, c["C"], 2 ** 40} <= set(y.tolist())
    blocked = [T.blocked_case(j) for j in range(len(T.BLOCKED_CASES))]
    assert {(c["C"], c["B"]) for c in blocked} == {(C, B) for C in (8, 64, 256) for B in (1, 2, 4)}
    assert values(blocked, "bias") == {True, False}
    assert {j % 4 for j in range(len(T.BLOCKED_CASES))} <= set(range(4))
    gemm = [T.gemm_case(k) for k in range(T.GEMM_CASES)]
    assert values(gemm, "M") == {1, 63, 64, 65, 128, 129} and values(gemm, "N") == {1, 127, 128, 129, 260}
    assert values(gemm, "K") == {0, 1, 31, 32, 33, 511, 512, 513, 1025, 4096, 4099}
    assert values(gemm, "a") == values(gemm, "b") == {"fresh", "padded", "block"}
    assert all(c["M"] % 4 for c in gemm if c["a"] == "padded") and all(c["N"] % 4 for c in gemm if c["b"] == "padded")
    assert {(c["colsum"], c["views"]) for c in gemm} == {(a, b) for a in (True, False) for b in (True, False)}
    assert values(gemm, "alpha") == {1.0, 0.5, -1.0}
    assert any(c["K"] >= 4096 and (c["a"] == "padded" or c["b"] == "padded") for c in gemm)   # the aligning copy
    rows = [T.gemm_rows_case(j) for j in range(T.GEMM_ROWS_CASES)]
    assert [c["rows"] for c in rows] == ["empty", "all", "one", 31, 32, 33] and values(rows, "colsum") == {True, False}
    assert all(c["M"] % 4 == 0 and c["N"] % 4 == 0 for c in rows + [T.gemm_bn_case(j) for j in range(T.GEMM_BN_CASES)])
    assert {j % 4 for j in range(T.GEMM_ROWS_CASES)} | {j % 4 for j in range(T.GEMM_BN_CASES)} <= set(range(4))
    assert T.ROWS_D == [1, 4, 7, 132]
    fold = [T.fold_case(k) for k in range(T.FOLD_CASES)]
    assert values(fold, "n_out") == values(fold, "K") == {1, 31, 32, 33, 65}
    for key in ("wide", "root", "bias", "bias2", "bn"):
        assert values(fold, key) == {True, False}, key
    assert {k % len(T.ROWS_D) for k in range(T.FOLD_CASES)} == set(range(len(T.ROWS_D)))
    assert [c for c in T.CSR_CASES if c[0] <= 1000] == T.SMALL_CSR_CASES[:-1] and len(T.SMALL_CSR_CASES) == 7


def test_the_sweep_blocks_cover_every_case():
    """The parametrised GPU tests run cases k with block * size <= k < (block + 1) * size, or k % blocks == block."""
    assert T.BN_CASES == 4 * 4 and T.LOSS_CASES == 4 * 7
    assert T.split_restated(torch.tensor([0, 3, 2051, 2051]), 1024) == {
        "chunk_begin": [3, 1027], "chunk_end": [1027, 2051], "chunk_row": [1, 1], "long_row": [1], "long_chunk_ptr": [0, 2],
        "n_chunks": 2, "n_long": 1, "threshold": 1024}
    assert T.split_restated(torch.tensor([0, 1024]), 1024) is None
