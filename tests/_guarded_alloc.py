"""Guarded, poisoned allocations for the package's own buffers (a test helper: no conftest, no pytest setting).

Every package module names its allocator as the module global `torch`. `guarded(monkeypatch)` replaces that name, in every
module of `rgb_experiment_amd` outside `dist/` whose source allocates through it, with a proxy that forwards everything to
the real torch except `empty`, `empty_like`, `empty_strided`, `zeros`, `zeros_like` and `full`. Those six go to a `Guard`:

    [ band | numel elements | band ]      one torch.full, the caller gets the middle

* band = max(128 elements, 2 rows of the request), rounded up to a multiple of 512 bytes: the buffer keeps the alignment
  class of a fresh allocation, so the kernels' choice between float4 and scalar paths (`aligned16(ptr)`, `ld % 4`) is the
  one an unguarded run makes. A row is the last dimension of a request of two or more dimensions, one element otherwise.
* interior (`empty*` only; `zeros*` / `full` hold what was asked for): NaN for floating types, 0 for integers, 1 for bool,
  0xFF for uint8. An element a kernel skips then reads as NaN in whatever is compared with the float64 reference; an
  unwritten index reads as 0, a valid row or slot of everything, never a wild address.
  uint8 departs from the 1 the plan named: the package's uint8 buffers are almost all raw workspaces that the kernels read
  as floats or ints. 0x01010101 is a denormal as a float (an unwritten record would pass unseen) and row 16,843,009 as an
  index (a wild address); 0xFF bytes read as NaN through a float view and as -1 through an int view (the package's own
  "ignored" label, at worst one row before a buffer's start), and as a mask byte they are as true as 1.
* band: NaN with the payload 0x5A.. for floating types (a kernel that stores a NaN it computed stores the canonical one,
  which differs bit for bit), -2 for integers, 0x5A for uint8 and bool — values the package never writes.

The buffer handed out shares the base's storage at an offset (Tensor.set_), is contiguous (or has the strides
`empty_like` / `empty_strided` would give), and is no autograd view. `Guard.check()` compares every band with its fill,
bit for bit, and names the allocation's call site, shape, dtype and the first offending offset (negative: before the
buffer; >= numel: past its end). Every base stays alive until `check()`.

Tensor-method allocations stay unguarded (they do not go through the module global):
    rgb_experiment_amd/nn/conv.py:856, 1711          x.new_zeros
    rgb_experiment_amd/ops.py:704, 1648, 1803        stats.new_zeros(())
    rgb_experiment_amd/ops.py:1941, 1945             wi.new_zeros
    rgb_experiment_amd/ops.py:4248, 4260             x.new_zeros / t.new_zeros(1)
    rgb_experiment_amd/utils/edges.py:24             edge_index.new_empty((2, 0))
No allocation of the discovered modules is exempt. (The pinned host staging buffers are `dist/comm.py`'s, and no `dist`
code runs under the guard; neither does a hipGraph capture.)"""
import contextlib
import importlib
import importlib.util
import math
import os
import pkgutil
import re
import sys
from collections import Counter

import torch as _torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = "rgb_experiment_amd"
NAMES = ("empty", "empty_like", "empty_strided", "zeros", "zeros_like", "full")
ALLOC_RE = re.compile(r"\btorch\.(%s)\(" % "|".join(NAMES))
MIN_BAND = 128      # elements
BAND_ROWS = 2
BAND_BYTES = 512    # the band's byte length is a multiple of this

_BITS = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}
# floating types: (bits of the band's NaN, as a value of the same-size integer type)
_BAND_NAN = {_torch.float32: 0x7FC5A5A5, _torch.float64: 0x7FF85A5A5A5A5A5A, _torch.bfloat16: 0x7FDA, _torch.float16: 0x7EDA}
_INT_BAND = -2
_BYTE_BAND = 0x5A


def band_elements(shape, itemsize):
    row = int(shape[-1]) if len(shape) >= 2 else 1
    band = max(MIN_BAND, BAND_ROWS * row)
    unit = BAND_BYTES // math.gcd(BAND_BYTES, itemsize)
    return -(-band // unit) * unit


def interior_fill(dtype):
    if dtype.is_floating_point:
        return float("nan")
    if dtype == _torch.bool:
        return True
    return 0xFF if dtype == _torch.uint8 else 0


def _call_site():
    f = sys._getframe(1)
    here = __file__
    while f is not None and f.f_code.co_filename == here:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d" % (os.path.relpath(f.f_code.co_filename, ROOT), f.f_lineno)


def _size(args):
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class Guard:
    def __init__(self):
        self._records = []      # (flat base in its storage type, band, extent, site, shape, dtype)
        self._counts = Counter()
        self.float_allocations = 0
        self.allocations = 0

    # ---- the one allocation ------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, device, stride=None, fill=None, pin_memory=False, requires_grad=False):
        dtype = dtype or _torch.get_default_dtype()
        shape = tuple(shape)
        if stride is None:
            stride = _torch.empty(shape, device="meta").stride()
        stride = tuple(int(s) for s in stride)
        numel = math.prod(shape)
        extent = 1 + sum((n - 1) * s for n, s in zip(shape, stride)) if numel else 0
        itemsize = _torch.empty((), dtype=dtype, device="meta").element_size()
        band = band_elements(shape, itemsize)
        total = 2 * band + extent
        kw = dict(device=device, pin_memory=pin_memory) if pin_memory else dict(device=device)
        if dtype.is_floating_point:
            base = _torch.full((total,), _BAND_NAN[dtype], dtype=_BITS[itemsize], **kw)
            typed = base.view(dtype)
        elif dtype in (_torch.bool, _torch.uint8):
            base = _torch.full((total,), _BYTE_BAND, dtype=_torch.uint8, **kw)
            typed = base.view(dtype)
        else:
            base = typed = _torch.full((total,), _INT_BAND, dtype=dtype, **kw)
        if extent:
            typed[band:band + extent].fill_(interior_fill(dtype) if fill is None else fill)
        out = _torch.empty(0, dtype=dtype, device=base.device)
        out.set_(typed.untyped_storage(), band, shape, stride)
        site = _call_site()
        self._records.append((base, band, extent, site, shape, dtype))
        self._counts[site] += 1
        self.allocations += 1
        self.float_allocations += bool(dtype.is_floating_point)
        return out.requires_grad_() if requires_grad else out

    @staticmethod
    def _like_stride(t, memory_format):
        meta = _torch.empty_strided(t.shape, t.stride(), device="meta")
        return _torch.empty_like(meta, memory_format=memory_format or _torch.preserve_format).stride()

    @staticmethod
    def _format_stride(shape, memory_format):
        if memory_format in (None, _torch.contiguous_format):
            return None
        return _torch.empty(shape, device="meta", memory_format=memory_format).stride()

    # ---- the six names -----------------------------------------------------------------------------------------------
    def empty(self, *size, dtype=None, device=None, pin_memory=False, memory_format=None, requires_grad=False):
        shape = _size(size)
        return self._alloc(shape, dtype, device, self._format_stride(shape, memory_format), None, pin_memory, requires_grad)

    def zeros(self, *size, dtype=None, device=None, pin_memory=False, requires_grad=False):
        return self._alloc(_size(size), dtype, device, None, 0, pin_memory, requires_grad)

    def full(self, size, fill_value, *, dtype=None, device=None, pin_memory=False, requires_grad=False):
        if dtype is None:
            dtype = fill_value.dtype if isinstance(fill_value, _torch.Tensor) else _torch.full((), fill_value, device="meta").dtype
        return self._alloc(_size((size,)), dtype, device, None, fill_value, pin_memory, requires_grad)

    def empty_strided(self, size, stride, *, dtype=None, device=None, pin_memory=False, requires_grad=False):
        return self._alloc(tuple(size), dtype, device, stride, None, pin_memory, requires_grad)

    def empty_like(self, t, *, dtype=None, device=None, pin_memory=False, memory_format=None, requires_grad=False):
        return self._alloc(t.shape, dtype or t.dtype, t.device if device is None else device,
                           self._like_stride(t, memory_format), None, pin_memory, requires_grad)

    def zeros_like(self, t, *, dtype=None, device=None, pin_memory=False, memory_format=None, requires_grad=False):
        return self._alloc(t.shape, dtype or t.dtype, t.device if device is None else device,
                           self._like_stride(t, memory_format), 0, pin_memory, requires_grad)

    # ---- the verdict -------------------------------------------------------------------------------------------------
    def counts(self):
        """{call site (file:line): guarded allocations made there}."""
        return dict(self._counts)

    def check(self):
        """Every band still holds its fill, bit for bit; the bases are released afterwards."""
        records, self._records = self._records, []
        flags = {}
        for i, (base, band, extent, _, _, _) in enumerate(records):
            fill = base[0]  # checked below against the constant, so a damaged first element does not hide the rest
            bad = (base[:band] != fill).any() | (base[band + extent:] != fill).any()
            flags.setdefault(base.device, []).append((i, bad))
        suspects = []
        for dev, fl in flags.items():
            firsts = _torch.stack([records[i][0][0].to(_torch.int64) for i, _ in fl]).cpu().tolist()
            bads = _torch.stack([b for _, b in fl]).cpu().tolist()
            for (i, _), first, bad in zip(fl, firsts, bads):
                if bad or first != self._band_bits(records[i][5]):
                    suspects.append(i)
        problems = []
        for i in suspects:
            base, band, extent, site, shape, dtype = records[i]
            want = self._band_bits(dtype)
            flat = base.cpu().to(_torch.int64)
            wrong = _torch.cat([flat[:band] != want, _torch.zeros(extent, dtype=_torch.bool), flat[band + extent:] != want])
            where = _torch.nonzero(wrong).flatten()
            problems.append("%s: shape %s dtype %s: %d band element(s) overwritten, the first at offset %d of the buffer "
                            "(it has %d)" % (site, tuple(shape), dtype, where.numel(), int(where[0]) - band, extent))
        assert not problems, "writes outside a guarded buffer:\n  " + "\n  ".join(problems)

    @staticmethod
    def _band_bits(dtype):
        if dtype.is_floating_point:
            return _BAND_NAN[dtype]
        return _BYTE_BAND if dtype in (_torch.bool, _torch.uint8) else _INT_BAND


class TorchProxy:
    """The module global `torch` of a package module under guard: the real torch but for the six allocators."""

    def __init__(self, guard):
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        if name in NAMES:
            return getattr(self.__dict__["_guard"], name)
        return getattr(_torch, name)


def allocating_modules():
    """Names of the package modules (dist/ left out) whose source calls one of the six allocators through `torch.`: found
    by walking the package, so a module added later is under guard without being listed anywhere."""
    pkg = importlib.import_module(PACKAGE)
    found = []
    for info in pkgutil.walk_packages(pkg.__path__, PACKAGE + "."):
        if info.name.startswith(PACKAGE + ".dist"):
            continue
        spec = importlib.util.find_spec(info.name)
        if spec is None or not spec.origin or not spec.origin.endswith(".py"):
            continue
        with open(spec.origin) as f:
            if ALLOC_RE.search(f.read()):
                found.append(info.name)
    return sorted(found)


@contextlib.contextmanager
def guarded(monkeypatch, guard=None):
    """with guarded(monkeypatch) as guard: ...; [torch.cuda.synchronize();] guard.check()"""
    guard = guard or Guard()
    proxy = TorchProxy(guard)
    with monkeypatch.context() as m:
        for name in allocating_modules():
            mod = importlib.import_module(name)
            if getattr(mod, "torch", None) is _torch:
                m.setattr(mod, "torch", proxy)
        yield guard


def per_module(counts):
    """{module file: guarded allocations} of Guard.counts()."""
    out = Counter()
    for site, k in counts.items():
        out[site.rsplit(":", 1)[0]] += k
    return dict(out)
