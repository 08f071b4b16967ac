"""Host side of the column selection carried in the column stream and of the loss epilogue's no-fill flag: the ctypes
mirrors of the two structs against the header, and the argument errors of rgbx_col_tag_i32 / rgbx_fused_layer_t.col_tag
(returned before any launch: no GPU needed). The GPU side is tests/test_gpu_col_tag.py."""
import ctypes
import os
import re

import pytest

from rgb_experiment_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rgbx_hip.h")

_CTYPES = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}


def _header_fields(tag):
    """[(name, ctypes type)] of `typedef struct <tag> { ... }` in the header, in declaration order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s\s*\{(.*?)\}" % tag, text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(",")]  # "const float* x" / "int64_t a", "b"
        base, name0 = first.rsplit(" ", 1)
        for d in [name0] + rest:
            pointer = "*" in base or "*" in d
            fields.append((d.replace("*", "").strip(),
                           ctypes.c_void_p if pointer else _CTYPES[base.replace("const ", "").strip()]))
    return fields


@pytest.mark.parametrize("tag, mirror", [("rgbx_fused_layer", _lib.FusedLayer), ("rgbx_ce_epilogue", _lib.CeEpilogue)])
def test_struct_mirrors_match_the_header(tag, mirror):
    assert _header_fields(tag) == list(mirror._fields_)
    names = [n for n, _ in mirror._fields_]
    assert names[-1] == {"rgbx_fused_layer": "col_tag", "rgbx_ce_epilogue": "no_fill"}[tag]  # appended: old callers' layout stays


def test_argument_errors_of_the_new_entry_and_field():
    lib = _lib.load()
    p = 0x10000
    assert lib.rgbx_col_tag_i32(None, p, 5, 10, p, None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert lib.rgbx_col_tag_i32(p, None, 5, 10, p, None) == -1
    assert lib.rgbx_col_tag_i32(p, p, 5, 10, None, None) == -1
    assert lib.rgbx_col_tag_i32(p, p, -1, 10, p, None) == -1
    assert lib.rgbx_col_tag_i32(p, p, 5, -1, p, None) == -1
    assert lib.rgbx_col_tag_i32(p, p, 2**31, 10, p, None) == -2      # RGBX_E_RANGE
    assert lib.rgbx_col_tag_i32(None, None, 0, 10, None, None) == 0  # nothing to do
    L = _lib.FusedLayer()
    for k, v in dict(rowptr=p, col=p, x=p, ldx=128, wt=p, out=p, ldo=128, N=10, K=128, Nout=128, col_tag=p).items():
        setattr(L, k, v)
    assert lib.rgbx_fused_layer_f32(ctypes.byref(L), None) == -1 and b"col_tag" in lib.rgbx_last_error_string()
