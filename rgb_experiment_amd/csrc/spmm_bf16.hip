// CSR row-gather SpMM with the gathered table stored as bfloat16 (gfx950):
//   out[i,:] = a*rs[i]*sum_p w[p]*widen(x[col[p],:]) + b*y[i,:] + bias[:]
// The expression, the one-wave-per-target-row scheme, the index hand-round and the hub-row split are spmm.hip's
// (rgbx_spmm_csr_f32); only the storage of x differs. The gather is memory-bound and the table is most of its bytes
// (degree 30, d = 64: 30 x 256 B of ~8.2 KB per target row), so halving the table's element halves that term; every sum and
// the whole epilogue stay in fp32. Helpers shared with spmm.hip are restated here (as pna.hip does with multi_aggr.hip's),
// spmm.hip and spmm_internal.h are untouched.
//
// Lane layout: a lane holds 8 contiguous bf16 columns = one 16-byte load (global_load_dwordx4), widened exactly with a
// shift (even column) and a mask (odd column) per dword. G = d/8 lanes, rounded up to a power of two, cover one neighbour
// row (surplus lanes inactive); the wave's NG = 64/G groups read NG neighbour rows per wave-instruction — d = 64: G = 8,
// eight rows per instruction, a row exactly one 128-byte line. U instructions are issued back to back, so U * 1 KiB are in
// flight per wave as in the f32 kernel (twice its rows). The groups' partial sums are folded by xor shuffle at the end.
//
// Rounding (rgbx_rows_f32_to_bf16 and the out_bf16 store): to nearest, ties to even, on the fp32 bit pattern
// (bits + 0x7fff + lsb) >> 16 — overflow carries into the exponent and gives inf as IEEE does; every NaN becomes the
// quiet NaN 0xffff, which is what torch's vectorised CPU conversion writes.
#include "rgbx_common.h"

#ifndef RGBX_BF16_UNROLL
#define RGBX_BF16_UNROLL 4
#endif

namespace rgbx {
namespace {

constexpr int kVec = 8;  // bf16 columns per lane

using u4v = __attribute__((ext_vector_type(4))) unsigned int;
using f4v = __attribute__((ext_vector_type(4))) float;

struct Bf16Args {
  const int* rowptr;
  const int* col;
  const float* w;
  const float* rs;
  const uint16_t* x;
  const float* y;
  const float* bias;
  float* out;
  uint16_t* out_bf16;
  int64_t ldx, ldy, ldo, ldob;
  int N, d;
  float a, b;
  int skip_longer;  // > 0: rows with more slots than this are left to the split-row kernels
};

__device__ __forceinline__ unsigned int bf16_round_bits(float f) {
  const unsigned int u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffu;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ u4v pack_bf16x8(const float (&r)[kVec]) {
  u4v o;
  o.x = bf16_round_bits(r[0]) | (bf16_round_bits(r[1]) << 16);
  o.y = bf16_round_bits(r[2]) | (bf16_round_bits(r[3]) << 16);
  o.z = bf16_round_bits(r[4]) | (bf16_round_bits(r[5]) << 16);
  o.w = bf16_round_bits(r[6]) | (bf16_round_bits(r[7]) << 16);
  return o;
}

__device__ __forceinline__ void load_f8(float (&v)[kVec], const float* p) {
  const f4v lo = *reinterpret_cast<const f4v*>(p);
  const f4v hi = *reinterpret_cast<const f4v*>(p + 4);
  v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
  v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}

// Weighted sum of the gathered bf16 rows of slots [start, end) into acc (this lane's 8 columns, base pointer xc). On
// return the NG groups' partial sums are folded: every lane of a column holds the total.
template <int G, bool HAS_W>
__device__ __forceinline__ void accumulate_slots_bf16(const Bf16Args& A, int start, int end, const uint16_t* xc,
                                                      bool active, int lane, int g, float (&acc)[kVec]) {
  constexpr int NG = kWave / G;
  constexpr int U = NG * RGBX_BF16_UNROLL > kWave ? (kWave / NG) : RGBX_BF16_UNROLL;  // NG * U slots per step, <= 64
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int mycol = 0;
    float myw = 0.f;
    if (lane < n) {
      mycol = A.col[base + lane];
      if constexpr (HAS_W) myw = A.w[base + lane];
    }
    for (int k = 0; k < n; k += NG * U) {
      u4v v[U];
      float ww[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int src = __shfl(mycol, idx & 63);
        if constexpr (HAS_W) ww[u] = __shfl(myw, idx & 63);
        const bool ok = active && idx < n;
        v[u] = u4v{0u, 0u, 0u, 0u};
        if (ok) v[u] = *reinterpret_cast<const u4v*>(xc + (int64_t)src * A.ldx);
        if constexpr (HAS_W) { if (!ok) ww[u] = 0.f; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const unsigned int q[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float lo = __uint_as_float(q[i] << 16);
          const float hi = __uint_as_float(q[i] & 0xffff0000u);
          if constexpr (HAS_W) {
            acc[2 * i] = fmaf(ww[u], lo, acc[2 * i]);
            acc[2 * i + 1] = fmaf(ww[u], hi, acc[2 * i + 1]);
          } else {
            acc[2 * i] += lo;
            acc[2 * i + 1] += hi;
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < kVec; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
}

// The epilogue of rgbx_spmm_csr_f32 (same operation order) over 8 columns, then the fp32 and / or the bf16 store.
__device__ __forceinline__ void bf16_epilogue(const Bf16Args& A, int row, int c, const float (&acc)[kVec]) {
  const float scale = A.rs ? A.a * A.rs[row] : A.a;
  float r[kVec];
#pragma unroll
  for (int i = 0; i < kVec; ++i) r[i] = scale * acc[i];
  if (A.y) {
    float yv[kVec];
    load_f8(yv, A.y + (int64_t)row * A.ldy + c);
#pragma unroll
    for (int i = 0; i < kVec; ++i) r[i] = fmaf(A.b, yv[i], r[i]);
  }
  if (A.bias) {
    float bv[kVec];
    load_f8(bv, A.bias + c);
#pragma unroll
    for (int i = 0; i < kVec; ++i) r[i] += bv[i];
  }
  if (A.out) {  // non-temporal, as the f32 kernel: nobody reads the row in this launch, the table wants the caches
    float* o = A.out + (int64_t)row * A.ldo + c;
    __builtin_nontemporal_store(f4v{r[0], r[1], r[2], r[3]}, reinterpret_cast<f4v*>(o));
    __builtin_nontemporal_store(f4v{r[4], r[5], r[6], r[7]}, reinterpret_cast<f4v*>(o + 4));
  }
  if (A.out_bf16) *reinterpret_cast<u4v*>(A.out_bf16 + (int64_t)row * A.ldob + c) = pack_bf16x8(r);
}

template <int G, bool HAS_W>
__global__ void __launch_bounds__(256) spmm_bf16_kernel(const Bf16Args A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * kVec;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;  // wave-uniform
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;  // split-row kernels own it
  float acc[kVec];
#pragma unroll
  for (int i = 0; i < kVec; ++i) acc[i] = 0.f;
  accumulate_slots_bf16<G, HAS_W>(A, start, end, A.x + c, active, lane, g, acc);
  if (g == 0 && active) bf16_epilogue(A, row, c, acc);
}

// One wave per chunk of a long row: raw weighted sums (no epilogue) into partial[chunk, d] (fp32).
template <int G, bool HAS_W>
__global__ void __launch_bounds__(256)
spmm_bf16_chunk_kernel(const Bf16Args A, int n_chunks, const int* __restrict__ chunk_begin,
                       const int* __restrict__ chunk_end, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * kVec;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    float acc[kVec];
#pragma unroll
    for (int i = 0; i < kVec; ++i) acc[i] = 0.f;
    accumulate_slots_bf16<G, HAS_W>(A, start, end, A.x + c, active, lane, g, acc);
    if (g == 0 && active) {
      float* p = partial + (int64_t)ch * A.d + c;
      *reinterpret_cast<f4v*>(p) = f4v{acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<f4v*>(p + 4) = f4v{acc[4], acc[5], acc[6], acc[7]};
    }
  }
}

// One wave per long row: partials added in chunk order, then the normal epilogue.
__global__ void __launch_bounds__(256)
spmm_bf16_combine_kernel(const Bf16Args A, int n_long, const int* __restrict__ long_row,
                         const int* __restrict__ long_chunk_ptr, const float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int c = lane * kVec;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    if (c >= A.d) continue;  // d <= 256: 32 lanes cover the row
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    float acc[kVec];
#pragma unroll
    for (int i = 0; i < kVec; ++i) acc[i] = 0.f;
    for (int ch = c0; ch < c1; ++ch) {
      float p[kVec];
      load_f8(p, partial + (int64_t)ch * A.d + c);
#pragma unroll
      for (int i = 0; i < kVec; ++i) acc[i] += p[i];
    }
    bf16_epilogue(A, row, c, acc);
  }
}

template <int G>
int launch_bf16(const Bf16Args& A, const rgbx_row_split_t* sp, hipStream_t s) {
  constexpr int kWavesPerBlock = 4;
  // one row per wave, no grid cap: the dispatcher balances rows of different length (see spmm.hip launch)
  const int64_t blocks = cdiv(A.N, kWavesPerBlock);
  if (A.w)
    spmm_bf16_kernel<G, true><<<(int)blocks, 256, 0, s>>>(A);
  else
    spmm_bf16_kernel<G, false><<<(int)blocks, 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("spmm_bf16_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, kWavesPerBlock);
    if (cb > kMaxGrid) cb = kMaxGrid;
    if (A.w)
      spmm_bf16_chunk_kernel<G, true><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                             sp->partial);
    else
      spmm_bf16_chunk_kernel<G, false><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                              sp->partial);
    RGBX_CHECK_LAUNCH("spmm_bf16_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, kWavesPerBlock);
    if (lb > kMaxGrid) lb = kMaxGrid;
    spmm_bf16_combine_kernel<<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->long_row, sp->long_chunk_ptr, sp->partial);
    RGBX_CHECK_LAUNCH("spmm_bf16_combine_kernel");
  }
  return RGBX_OK;
}

// dst[r, c] = round-to-nearest-even(src[r, c]); a thread converts 8 columns (two 16-byte loads, one 16-byte store).
__global__ void __launch_bounds__(256)
rows_to_bf16_vec_kernel(const float* __restrict__ src, int64_t lds, uint16_t* __restrict__ dst, int64_t ldd, int64_t n,
                        int d8) {
  const int64_t total = n * d8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / d8;
    const int c = (int)(i - row * d8) * kVec;
    float v[kVec];
    load_f8(v, src + row * lds + c);
    *reinterpret_cast<u4v*>(dst + row * ldd + c) = pack_bf16x8(v);
  }
}

__global__ void __launch_bounds__(256)
rows_to_bf16_kernel(const float* __restrict__ src, int64_t lds, uint16_t* __restrict__ dst, int64_t ldd, int64_t n, int d) {
  const int64_t total = n * d;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / d;
    const int c = (int)(i - row * d);
    dst[row * ldd + c] = (uint16_t)bf16_round_bits(src[row * lds + c]);
  }
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_spmm_csr_bf16_supported(int64_t d) { return d >= 8 && d <= 256 && d % 8 == 0; }

extern "C" int rgbx_spmm_csr_bf16(const int32_t* rowptr, const int32_t* col, const float* w, const float* rs,
                                  const uint16_t* x, int64_t ldx, const float* y, int64_t ldy, const float* bias,
                                  float* out, int64_t ldo, uint16_t* out_bf16, int64_t ldob, int64_t N, int64_t d,
                                  float a, float b, const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "spmm_bf16: negative size");
  if (N == 0) return RGBX_OK;
  if (!rowptr || !col || !x) return fail(RGBX_E_ARG, "spmm_bf16: null pointer");
  if (!out && !out_bf16) return fail(RGBX_E_ARG, "spmm_bf16: neither out nor out_bf16 given");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "spmm_bf16: N exceeds int32");
  if (!rgbx_spmm_csr_bf16_supported(d))
    return fail(RGBX_E_SHAPE, "spmm_bf16: needs d %% 8 == 0 and 8 <= d <= 256 (got %lld); pad the rows", (long long)d);
  if (ldx < d || (out && ldo < d) || (out_bf16 && ldob < d) || (y && ldy < d))
    return fail(RGBX_E_ARG, "spmm_bf16: leading dimension < d");
  if ((const void*)out_bf16 == (const void*)x) return fail(RGBX_E_ARG, "spmm_bf16: out_bf16 must not alias x");
  if (!aligned16(x) || ldx % 8 || (out_bf16 && (!aligned16(out_bf16) || ldob % 8)))
    return fail(RGBX_E_ALIGN, "spmm_bf16: x / out_bf16 rows must be 16-byte aligned (ld %% 8 == 0)");
  if ((y && (!aligned16(y) || ldy % 4)) || (out && (!aligned16(out) || ldo % 4)) || (bias && !aligned16(bias)))
    return fail(RGBX_E_ALIGN, "spmm_bf16: y / out / bias must be 16-byte aligned with ld %% 4 == 0");
  Bf16Args A{rowptr, col, w, rs, x, y, bias, out, out_bf16, ldx, ldy, ldo, ldob, (int)N, (int)d, a, b, 0};
  const rgbx_row_split_t* sp = nullptr;
  if (split && split->threshold > 0 && split->n_chunks > 0) {
    if (split->n_long <= 0 || !split->chunk_begin || !split->chunk_end || !split->long_row || !split->long_chunk_ptr ||
        !split->partial)
      return fail(RGBX_E_ARG, "spmm_bf16: incomplete row-split plan");
    if (!aligned16(split->partial)) return fail(RGBX_E_ALIGN, "spmm_bf16: split->partial must be 16-byte aligned");
    sp = split;
    A.skip_longer = split->threshold;
  }
  hipStream_t s = (hipStream_t)stream;
  const int lanes = (int)(d / kVec);
  if (lanes <= 1) return launch_bf16<1>(A, sp, s);
  if (lanes <= 2) return launch_bf16<2>(A, sp, s);
  if (lanes <= 4) return launch_bf16<4>(A, sp, s);
  if (lanes <= 8) return launch_bf16<8>(A, sp, s);
  if (lanes <= 16) return launch_bf16<16>(A, sp, s);
  return launch_bf16<32>(A, sp, s);
}

extern "C" int rgbx_rows_f32_to_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t n, int64_t d,
                                     rgbx_stream_t stream) {
  if (n < 0 || d < 0) return fail(RGBX_E_ARG, "rows_f32_to_bf16: negative size");
  if (n == 0 || d == 0) return RGBX_OK;
  if (!src || !dst) return fail(RGBX_E_ARG, "rows_f32_to_bf16: null pointer");
  if (n >= INT32_MAX || d >= INT32_MAX) return fail(RGBX_E_RANGE, "rows_f32_to_bf16: size exceeds int32");
  if (lds < d || ldd < d) return fail(RGBX_E_ARG, "rows_f32_to_bf16: leading dimension < d");
  if (reinterpret_cast<uintptr_t>(src) % 4 || reinterpret_cast<uintptr_t>(dst) % 2)
    return fail(RGBX_E_ALIGN, "rows_f32_to_bf16: src / dst must be aligned to their element");
  hipStream_t s = (hipStream_t)stream;
  const bool vec = d % kVec == 0 && lds % 4 == 0 && ldd % kVec == 0 && aligned16(src) && aligned16(dst);
  int64_t blocks = cdiv(vec ? n * (d / kVec) : n * d, 256);
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  if (vec)
    rows_to_bf16_vec_kernel<<<(int)blocks, 256, 0, s>>>(src, lds, dst, ldd, n, (int)(d / kVec));
  else
    rows_to_bf16_kernel<<<(int)blocks, 256, 0, s>>>(src, lds, dst, ldd, n, (int)d);
  RGBX_CHECK_LAUNCH("rows_f32_to_bf16");
  return RGBX_OK;
}
