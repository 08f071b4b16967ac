"""Host-side argument checks of the two extra forms of the weight-gradient GEMM (rgbx_gemm_tn_bn_bwd_f32,
rgbx_gemm_tn_rows_f32) and their workspace query. Every rejected call returns before a launch (fake, never dereferenced
pointers): no GPU needed."""
import ctypes


def _lib():
    from rgb_experiment_amd import _lib
    return _lib.load()


P = 0x10000  # 16-byte aligned, non-null
OK, E_ARG, E_RANGE, E_ALIGN, E_WS = 0, -1, -2, -3, -4


def _ws(lib, K, M, N):
    n = ctypes.c_size_t(0)
    assert lib.rgbx_gemm_tn_workspace_bytes(K, M, N, ctypes.byref(n)) == OK
    return n.value


def test_workspace_query_is_the_plain_gemms():
    """Both forms run the slabs of rgbx_gemm_tn_f32 on K rows: S partial [M, N] tiles and S partial [M] column sums."""
    lib = _lib()
    assert _ws(lib, 1000, 128, 128) >= (128 * 128 + 128) * 4
    # K = 70 001: ceil(K / 512) = 137 slabs of at least 16 staged tiles
    assert _ws(lib, 70001, 128, 128) == 137 * (128 * 128 + 128) * 4
    assert _ws(lib, 70001, 32, 64) == 137 * (32 * 64 + 32) * 4
    n = ctypes.c_size_t(0)
    assert lib.rgbx_gemm_tn_workspace_bytes(-1, 128, 128, ctypes.byref(n)) == E_ARG


def test_bn_bwd_form_argument_checks():
    lib = _lib()
    K, M, N = 1000, 128, 128
    ws = _ws(lib, K, M, N)

    def call(G=P, ldg=M, X=P, ldx=M, mean=P, B=P, ldb=N, C=P, ldc=N, K=K, M=M, N=N, wsp=P, wsb=ws):
        return lib.rgbx_gemm_tn_bn_bwd_f32(G, ldg, X, ldx, mean, P, P, P, P, B, ldb, C, ldc, None, K, M, N, 1.0, wsp,
                                           wsb, None)

    assert call(wsb=16) == E_WS and b"workspace" in lib.rgbx_last_error_string()
    assert call(wsp=None) == E_WS
    assert call(K=-1) == E_ARG
    assert call(M=0) == OK and call(N=0) == OK              # nothing to do
    assert call(G=None) == E_ARG and call(B=None) == E_ARG and call(C=None) == E_ARG
    assert call(X=None) == E_ARG and call(mean=None) == E_ARG
    assert call(ldg=64) == E_ARG and call(ldx=64) == E_ARG and call(ldb=64) == E_ARG and call(ldc=64) == E_ARG
    assert call(M=2**31) == E_RANGE
    # the 16-byte path only: the caller runs the apply kernel and the plain GEMM otherwise
    assert call(G=P + 4) == E_ALIGN and b"16-byte" in lib.rgbx_last_error_string()
    assert call(X=P + 4) == E_ALIGN and call(B=P + 4) == E_ALIGN
    assert call(ldg=130) == E_ALIGN and call(ldx=129) == E_ALIGN and call(ldb=131) == E_ALIGN


def test_row_list_form_argument_checks():
    lib = _lib()
    K, M, N = 1000, 64, 128
    ws = _ws(lib, K, M, N)

    def call(A=P, lda=M, B=P, ldb=N, rows=P, n_rows=10, C=P, K=K, M=M, N=N, wsb=ws):
        return lib.rgbx_gemm_tn_rows_f32(A, lda, B, ldb, rows, n_rows, C, N, None, K, M, N, 1.0, P, wsb, None)

    assert call(wsb=16) == E_WS
    assert call(n_rows=-1) == E_ARG and call(n_rows=K + 1) == E_ARG and b"row list" in lib.rgbx_last_error_string()
    assert call(rows=None) == E_ARG
    assert call(A=None) == E_ARG and call(lda=32) == E_ARG
    assert call(M=0) == OK
    assert call(K=2**31, n_rows=0) == E_RANGE            # the list holds int32 row numbers
    assert call(A=P + 8) == E_ALIGN and call(B=P + 4) == E_ALIGN and call(lda=66) == E_ALIGN
