"""Host-side argument checks of the loss-gradient launch over a row list (rgbx_ce_epilogue_t.rows with grad_scale on
rgbx_fused_layer_f32) and its scratch-size query. Every call returns before a launch (fake, never dereferenced pointers):
no GPU needed. A call in the allowed combination is told apart from a refused one by an error that the entry point raises
only AFTER the row-list checks: the alignment check of x."""
import ctypes

P = 0x10000  # 16-byte aligned, non-null
OK, E_ARG, E_RANGE, E_ALIGN = 0, -1, -2, -3
N, K, C = 1000, 128, 64


def _call(grad=True, z_out=True, dense=False, w_pos=False, groups=1, n_rows=10, rows=P, out=P, ldo=C, x=P + 4):
    """One rgbx_fused_layer_f32 call with a row list; by default the allowed loss-gradient combination with a
    misaligned x, which is reported (E_ALIGN, "x / x_root / z_out") only once every row-list check has passed."""
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    ce = _lib.CeEpilogue(P, P, P if grad else None, P, P, groups)
    ce.rows, ce.n_rows = rows, n_rows
    L = _lib.FusedLayer()
    L.rowptr, L.col, L.w = (None if dense else P), P, P
    L.x, L.ldx, L.wt = x, K, P
    L.out, L.ldo = out, ldo
    if z_out:
        L.z_out = P
    L.ldz = K
    if w_pos:
        L.w_pos, L.z_pos_out = P, P
    L.ce = ctypes.addressof(ce)
    L.N, L.K, L.Nout = N, K, C
    rc = lib.rgbx_fused_layer_f32(ctypes.byref(L), None)
    return rc, lib.rgbx_last_error_string()


def test_row_list_with_gradient_passes_its_checks_in_the_allowed_combination():
    for kw in (dict(), dict(z_out=False), dict(n_rows=N), dict(n_rows=1)):
        rc, msg = _call(**kw)
        assert rc == E_ALIGN and b"x / x_root" in msg, (kw, msg)
    # the statistics-only list form is what it was: accepted without z_out (also with two statistics sets), refused with
    rc, msg = _call(grad=False, z_out=False)
    assert rc == E_ALIGN and b"x / x_root" in msg
    rc, msg = _call(grad=False, z_out=False, groups=2)
    assert rc == E_ALIGN and b"x / x_root" in msg
    rc, msg = _call(grad=False, z_out=True)
    assert rc == E_ARG and b"row list" in msg


def test_row_list_with_gradient_is_refused_elsewhere():
    for kw in (dict(w_pos=True), dict(dense=True), dict(groups=2), dict(n_rows=-1), dict(n_rows=N + 1),
               dict(rows=None)):
        rc, msg = _call(**kw)
        assert rc == E_ARG and b"row list" in msg, (kw, msg)
    # the zero fill of the unlisted rows stores 16 bytes at a time
    for kw in (dict(out=P + 4), dict(ldo=C + 2)):
        rc, msg = _call(**kw)
        assert rc == E_ALIGN and b"row list" in msg, (kw, msg)
    # without the list, a misaligned `out` is no obstacle to the loss gradient
    rc, msg = _call(rows=None, n_rows=0, out=P + 4)
    assert rc == E_ALIGN and b"x / x_root" in msg


def test_scratch_query():
    """Tile records and gather sums as always, (ceil(N / 32) + 64) * 3 doubles, then N floats and N bytes."""
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(0)
    for rows, want in ((1, 65 * 3 + 1 + 1), (32, 65 * 3 + 16 + 4), (33, 66 * 3 + 17 + 5)):
        assert lib.rgbx_ce_rows_grad_scratch_doubles(rows, ctypes.byref(n)) == OK
        assert n.value == want, (rows, n.value)
    assert lib.rgbx_ce_rows_grad_scratch_doubles(0, ctypes.byref(n)) == OK and n.value == 64 * 3
    assert lib.rgbx_ce_rows_grad_scratch_doubles(-1, ctypes.byref(n)) == E_ARG
    assert lib.rgbx_ce_rows_grad_scratch_doubles(5, None) == E_ARG
