"""_lib.call / _lib.launch: how Python arguments reach a C entry point (host only; nothing is launched).

A recording fake stands in for the library (`_lib.use`) to show what arrives; the real library, which loads without a
GPU (tests/test_abi.py), shows that a non-zero return code and a wrong argument count surface as errors."""
import ctypes

import pytest
import torch

from rgb_experiment_amd import _lib


class _Recorder:
    """Every attribute is an entry point that records its arguments and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry

    def rgbx_last_error_string(self):
        return b"recorded failure"


@pytest.fixture
def fake():
    saved = _lib._lib
    rec = _Recorder()
    _lib.use(rec)
    try:
        yield rec
    finally:
        _lib.use(saved)


def _address(ref):
    """The address a ctypes.byref(...) argument points at."""
    return ctypes.cast(ref, ctypes.c_void_p).value


def test_tensors_none_tuples_and_bools(fake):
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    _lib.call("rgbx_probe", t, None, _lib.mat(t, "t"), _lib.mat_opt(None, "y"), True, False, 7, 0.5)
    (name, args), = fake.calls
    assert name == "rgbx_probe"
    assert args == (t.data_ptr(), 0, t.data_ptr(), 3, 0, 0, 1, 0, 7, 0.5)
    assert all(type(a) is int for a in args[:9])  # True arrives as the int 1, not as a bool


def test_structures_arrive_by_reference(fake):
    split = _lib.RowSplit(1024, 3, 2)
    n = ctypes.c_int64(0)
    _lib.call("rgbx_probe", split, None, ctypes.byref(n))
    (_, (ref, null, out)), = fake.calls
    assert _address(ref) == ctypes.addressof(split)
    assert null == 0  # no plan: a null pointer in the split position
    assert _address(out) == ctypes.addressof(n)  # an explicit byref passes through


def test_mat_variants():
    t = torch.zeros((4, 8), dtype=torch.float32)[:, :5]
    assert _lib.mat(t, "t") == (t.data_ptr(), 8)
    assert _lib.mat_opt(t, "t") == _lib.mat(t, "t")
    assert _lib.mat_opt(None, "t") == (0, 0)
    with pytest.raises((AttributeError, RuntimeError)):  # a missing REQUIRED operand never turns into a null pointer
        _lib.mat(None, "t")
    b = torch.zeros((2, 8), dtype=torch.bfloat16)
    assert _lib.mat_bf16(b, "b") == (b.data_ptr(), 8)
    with pytest.raises(RuntimeError, match="b: expected a 2-D bfloat16 tensor, got torch.float32"):
        _lib.mat_bf16(t, "b")
    with pytest.raises(RuntimeError, match="t: expected a 2-D float32 tensor, got torch.bfloat16"):
        _lib.mat(b, "t")


def test_a_non_zero_return_names_the_entry_point(fake):
    fake.rc = 3
    with pytest.raises(RuntimeError, match=r"rgbx_probe failed \(hipError 3\): recorded failure"):
        _lib.call("rgbx_probe", 1)
    fake.rc = -2
    with pytest.raises(RuntimeError, match=r"rgbx_other failed \(argument error -2\)"):
        _lib.call("rgbx_other")


def test_launch_brackets_the_call_alone(fake, monkeypatch):
    """launch = call with the stream appended; the bracket opens after marshalling and closes before the check."""
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0xABC0)
    order = []

    class Bracket:
        def __enter__(self):
            order.append(("enter", len(fake.calls)))

        def __exit__(self, *exc):
            order.append(("exit", len(fake.calls)))
            return False

    t = torch.zeros(3)
    _lib.launch("rgbx_probe", t, 5)
    _lib.launch("rgbx_probe", t, 5, bracket=Bracket())
    assert fake.calls == [("rgbx_probe", (t.data_ptr(), 5, 0xABC0))] * 2
    assert order == [("enter", 1), ("exit", 2)]
    fake.rc = 1
    with pytest.raises(RuntimeError, match="rgbx_probe failed"):
        _lib.launch("rgbx_probe", t, 5, bracket=Bracket())
    assert order[2:] == [("enter", 2), ("exit", 3)]  # the bracket was left before the check raised


def test_real_library_argument_error_and_argument_count():
    _lib.load()
    n = ctypes.c_size_t(0)
    with pytest.raises(RuntimeError, match=r"rgbx_csr_workspace_bytes failed \(argument error -1\)"):
        _lib.call("rgbx_csr_workspace_bytes", -1, 4, ctypes.byref(n))
    _lib.call("rgbx_csr_workspace_bytes", 1000, 10, ctypes.byref(n))
    assert n.value >= 3 * 1010 * 4
    with pytest.raises((TypeError, ctypes.ArgumentError)):  # ctypes refuses the call: the declared signature has three
        _lib.call("rgbx_csr_workspace_bytes", 1000, 10)
    with pytest.raises(AttributeError):
        _lib.call("rgbx_no_such_entry_point")
