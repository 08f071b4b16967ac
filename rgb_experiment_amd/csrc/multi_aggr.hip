// One-pass multi-aggregation over a CSR for gfx950 (sum, mean, var, std, max, min of a neighbourhood from ONE gather), and its
// source-side backward.
//   forward : per target row i and column c, over the slots p of row i (n = their number, v_p = x[col[p], c]):
//               sum = S,  mean = S / max(n, 1),  var = mean(v^2) - mean(v)^2 (biased, not clamped),
//               std = sqrt(var) where var > 1e-5, else 0  (PyG's StdAggregation: sqrt(max(var, 1e-5)), masked at the floor),
//               max / min and their arg = rgbx_spmm_csr_extremum_f32's, value for value and slot for slot
//   backward: gx[j,c] = sum_q a[i,c] + x[j,c] * sum_q b[i,c] + sum_q gmax[i,c] [argmax[i,c] == t2f[q]] + (the same for min),
//             over the slots q of transposed row j, i = col_t[q]; a, b are per-target rows the caller prepares.
// Replaces MessagePassing.propagate with PyG's MultiAggregation(mode='cat') / aggr='std' | 'var' behind SAGEConv(aggr=[...])
// (reference models/graphsage2.py:20-23 passes the keyword through) [PyG]. A statistic whose pointer is NULL is neither
// computed nor stored: every combination is its own template instantiation.
//
// Lane layout: extremum.hip's. One wave owns one target row, split into NG = 64/G groups of G lanes; a group reads ONE
// neighbour row per step with 16-byte loads, U steps are issued back to back, and the 64 column indices of a row chunk are
// read once, coalesced, and handed to the groups with ds_bpermute. Every lane keeps the running statistics of its 4 columns.
//
// Second moment: sum(v^2)/n - (sum(v)/n)^2 in fp32 loses a nearly constant neighbourhood (the values' offset squared swamps
// their spread). The wave accumulates DEVIATIONS from a per-(row, column) shift k — the value of the row's first slot —
//   D = sum (v - k),  Q = sum (v - k)^2,     var = Q/n - (D/n)^2
// which is the same number for every k and is well conditioned for k inside the data. The NG groups of a wave share k, so
// their (D, Q) add, in a fixed butterfly. The chunks of a hub row each take their own first slot; two records
// (n, D, Q, k) merge exactly by re-basing the second onto the first one's shift (delta = k_b - k_a):
//   D = D_a + D_b + n_b delta,   Q = Q_a + Q_b + delta (2 D_b + n_b delta)
// (Chan's pairwise update written for shifted sums), in chunk order. A neighbourhood whose values are all equal has
// D = Q = delta = 0 in every record, so var and std are exactly 0 (duplicate edges, degree-1 rows). The plain sum S is kept
// beside D (S = D + n k would cancel) and added in the same fixed order.
//
// Extrema: strict > / < while a group walks its slots in ascending order, groups and chunks merged under "better value, or
// equal value and lower slot" — the comparisons of extremum.hip, so values and arg are EQUAL to that kernel's.
// Inputs are finite. No float atomics anywhere: two runs give the same bits.
#include "rgbx_common.h"

namespace rgbx {
namespace {

using f4v = __attribute__((ext_vector_type(4))) float;
using i4v = __attribute__((ext_vector_type(4))) int;

__device__ __forceinline__ void load_ivec4(int (&v)[4], const int* p) {
  const int4 t = *reinterpret_cast<const int4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

__device__ __forceinline__ void store_ivec4(int* p, const int (&v)[4]) {
  *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void nt_store(float* p, const float (&v)[4]) {
  f4v o = {v[0], v[1], v[2], v[3]};
  __builtin_nontemporal_store(o, reinterpret_cast<f4v*>(p));
}

// `a` at slot `sa` beats `b` at slot `sb`: strictly better, or equal and from a lower slot (-1 = no slot: the highest unsigned)
template <bool MAX>
__device__ __forceinline__ bool beats(float a, int sa, float b, int sb) {
  const bool better = MAX ? a > b : a < b;
  return better || (a == b && (unsigned)sa < (unsigned)sb);
}

constexpr float kStdFloor = 1e-5f;  // PyG StdAggregation: sqrt(var.clamp(min=1e-5)), 0 where that is <= sqrt(1e-5)

struct MultiArgs {
  const int* rowptr;
  const int* col;
  const float* x;
  int64_t ldx;
  rgbx_multi_out_t o;
  int N, d;
  int skip_longer;
};

// This lane's 4 columns. M1: sum / mean wanted, M2: var / std wanted, MAX / MIN: that extremum wanted; members of a
// statistic that is not wanted are never touched.
struct Rec {
  int n;  // slots behind dev / sq
  float s[4];
  float dev[4], sq[4], shift[4];
  float maxv[4], minv[4];
  int maxs[4], mins[4];
};

template <bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void rec_init(Rec& R) {
  R.n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (M1) R.s[i] = 0.f;
    if constexpr (M2) { R.dev[i] = 0.f; R.sq[i] = 0.f; R.shift[i] = 0.f; }
    if constexpr (MAX) { R.maxv[i] = -INFINITY; R.maxs[i] = -1; }
    if constexpr (MIN) { R.minv[i] = INFINITY; R.mins[i] = -1; }
  }
}

// (na, dev, sq, shift) <- itself merged with (nb, db, qb, kb), re-based onto its own shift (onto kb where it is empty)
__device__ __forceinline__ void merge_moments(int na, float& dev, float& sq, float& shift, int nb, float db, float qb, float kb) {
  const float k = na == 0 ? kb : shift;
  const float delta = kb - k;
  const float fb = (float)nb;
  // (explicit fma: every template form rounds alike, whatever the compiler would contract)
  dev = dev + fmaf(fb, delta, db);
  sq = sq + fmaf(delta, fmaf(fb, delta, 2.f * db), qb);
  shift = k;
}

// Slots [start, end): the statistics of this lane's 4 columns (base pointer xc), the NG groups merged on return. Every
// group deviates from the SAME shift, the value of slot `start`, so the groups' shifted sums simply add.
template <int G, bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void multi_slots(const MultiArgs& A, int start, int end, const float* xc, bool active, int lane,
                                            int g, Rec& R) {
  constexpr int NG = kWave / G;
  constexpr int U = 4;
  rec_init<M1, M2, MAX, MIN>(R);
  R.n = end - start;
  if constexpr (M2) {
    if (active && end > start) load_vec<4>(R.shift, xc + (int64_t)A.col[start] * A.ldx);  // one row, the same for all groups
  }
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int mycol = lane < n ? A.col[base + lane] : 0;
    for (int k = 0; k < n; k += NG * U) {
      float v[U][4];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int src = __shfl(mycol, idx & 63);
        ok[u] = active && idx < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[u][i] = 0.f;
        if (ok[u]) load_vec<4>(v[u], xc + (int64_t)src * A.ldx);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int p = base + k + u * NG + g;  // ascending within the group: strict comparison keeps the lowest slot
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (M1) R.s[i] += v[u][i];
          if constexpr (M2) {
            const float dv = ok[u] ? v[u][i] - R.shift[i] : 0.f;
            R.dev[i] += dv;
            R.sq[i] = fmaf(dv, dv, R.sq[i]);
          }
          if constexpr (MAX) {
            const bool take = ok[u] && v[u][i] > R.maxv[i];
            R.maxv[i] = take ? v[u][i] : R.maxv[i];
            R.maxs[i] = take ? p : R.maxs[i];
          }
          if constexpr (MIN) {
            const bool take = ok[u] && v[u][i] < R.minv[i];
            R.minv[i] = take ? v[u][i] : R.minv[i];
            R.mins[i] = take ? p : R.mins[i];
          }
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (M1) R.s[i] += __shfl_xor(R.s[i], off);
      if constexpr (M2) {
        R.dev[i] += __shfl_xor(R.dev[i], off);
        R.sq[i] += __shfl_xor(R.sq[i], off);
      }
      if constexpr (MAX) {
        const float ob = __shfl_xor(R.maxv[i], off);
        const int os = __shfl_xor(R.maxs[i], off);
        const bool take = beats<true>(ob, os, R.maxv[i], R.maxs[i]);
        R.maxv[i] = take ? ob : R.maxv[i];
        R.maxs[i] = take ? os : R.maxs[i];
      }
      if constexpr (MIN) {
        const float ob = __shfl_xor(R.minv[i], off);
        const int os = __shfl_xor(R.mins[i], off);
        const bool take = beats<false>(ob, os, R.minv[i], R.mins[i]);
        R.minv[i] = take ? ob : R.minv[i];
        R.mins[i] = take ? os : R.mins[i];
      }
    }
  }
}

// The finished statistics of row `row` (n slots), columns c..c+3, each into its own matrix. A row without slots stores 0
// everywhere and arg -1.
template <bool M1, bool M2, bool MAX, bool MIN>
__device__ __forceinline__ void multi_store(const MultiArgs& A, int row, int c, int n, const Rec& R) {
  const rgbx_multi_out_t& o = A.o;
  const float inv = 1.f / (float)max(n, 1);
  float t[4];
  if constexpr (M1) {
    if (o.sum) nt_store(o.sum + (int64_t)row * o.ld_sum + c, R.s);
    if (o.mean) {
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = R.s[i] * inv;
      nt_store(o.mean + (int64_t)row * o.ld_mean + c, t);
    }
  }
  if constexpr (M2) {
    float var[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float md = R.dev[i] * inv;
      var[i] = fmaf(-md, md, R.sq[i] * inv);
    }
    if (o.var) nt_store(o.var + (int64_t)row * o.ld_var + c, var);
    if (o.std) {
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = var[i] > kStdFloor ? sqrtf(var[i]) : 0.f;
      nt_store(o.std + (int64_t)row * o.ld_std + c, t);
    }
  }
  if constexpr (MAX) {
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = R.maxs[i] < 0 ? 0.f : R.maxv[i];
    nt_store(o.max + (int64_t)row * o.ld_max + c, t);
    if (o.argmax) {
      i4v s = {R.maxs[0], R.maxs[1], R.maxs[2], R.maxs[3]};
      __builtin_nontemporal_store(s, reinterpret_cast<i4v*>(o.argmax + (int64_t)row * o.ld_argmax + c));
    }
  }
  if constexpr (MIN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i] = R.mins[i] < 0 ? 0.f : R.minv[i];
    nt_store(o.min + (int64_t)row * o.ld_min + c, t);
    if (o.argmin) {
      i4v s = {R.mins[0], R.mins[1], R.mins[2], R.mins[3]};
      __builtin_nontemporal_store(s, reinterpret_cast<i4v*>(o.argmin + (int64_t)row * o.ld_argmin + c));
    }
  }
}

template <int G, bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256) multi_kernel(const MultiArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;  // the chunk + combine kernels own long rows
  Rec R;
  multi_slots<G, M1, M2, MAX, MIN>(A, start, end, A.x + c, active, lane, g, R);
  if (g == 0 && active) multi_store<M1, M2, MAX, MIN>(A, row, c, end - start, R);
}

// Chunk records in split->partial: one [n_chunks, d] section of 4-byte words per kept quantity, in this order.
template <bool M1, bool M2, bool MAX, bool MIN>
struct Sections {
  static constexpr int kS = 0;
  static constexpr int kDev = kS + (M1 ? 1 : 0);
  static constexpr int kSq = kDev + (M2 ? 1 : 0);
  static constexpr int kShift = kSq + (M2 ? 1 : 0);
  static constexpr int kMaxV = kShift + (M2 ? 1 : 0);
  static constexpr int kMaxS = kMaxV + (MAX ? 1 : 0);
  static constexpr int kMinV = kMaxS + (MAX ? 1 : 0);
  static constexpr int kMinS = kMinV + (MIN ? 1 : 0);
  static constexpr int kCount = kMinS + (MIN ? 1 : 0);
};

inline int sections_of(int which) {
  const bool m1 = which & (RGBX_MULTI_SUM | RGBX_MULTI_MEAN), m2 = which & (RGBX_MULTI_VAR | RGBX_MULTI_STD);
  return (m1 ? 1 : 0) + (m2 ? 3 : 0) + ((which & RGBX_MULTI_MAX) ? 2 : 0) + ((which & RGBX_MULTI_MIN) ? 2 : 0);
}

// One wave per chunk of a long row: the chunk's record into the partial sections.
template <int G, bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256)
multi_chunk_kernel(const MultiArgs A, int n_chunks, const int* __restrict__ chunk_begin, const int* __restrict__ chunk_end,
                   float* __restrict__ partial) {
  using S = Sections<M1, M2, MAX, MIN>;
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  const int64_t sec = (int64_t)n_chunks * A.d;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    Rec R;
    multi_slots<G, M1, M2, MAX, MIN>(A, start, end, A.x + c, active, lane, g, R);
    if (g == 0 && active) {
      float* p = partial + (int64_t)ch * A.d + c;
      if constexpr (M1) store_vec<4>(p + S::kS * sec, R.s);
      if constexpr (M2) {
        store_vec<4>(p + S::kDev * sec, R.dev);
        store_vec<4>(p + S::kSq * sec, R.sq);
        store_vec<4>(p + S::kShift * sec, R.shift);
      }
      if constexpr (MAX) {
        store_vec<4>(p + S::kMaxV * sec, R.maxv);
        store_ivec4(reinterpret_cast<int*>(p + S::kMaxS * sec), R.maxs);
      }
      if constexpr (MIN) {
        store_vec<4>(p + S::kMinV * sec, R.minv);
        store_ivec4(reinterpret_cast<int*>(p + S::kMinS * sec), R.mins);
      }
    }
  }
}

// One wave per long row: its chunk records merged in chunk order (ascending slots).
template <bool M1, bool M2, bool MAX, bool MIN>
__global__ void __launch_bounds__(256)
multi_combine_kernel(const MultiArgs A, int n_long, int n_chunks, const int* __restrict__ long_row,
                     const int* __restrict__ long_chunk_ptr, const int* __restrict__ chunk_begin,
                     const int* __restrict__ chunk_end, const float* __restrict__ partial) {
  using S = Sections<M1, M2, MAX, MIN>;
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int64_t sec = (int64_t)n_chunks * A.d;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < A.d; c += kWave * 4) {
      Rec R;
      rec_init<M1, M2, MAX, MIN>(R);
      for (int ch = c0; ch < c1; ++ch) {
        const float* p = partial + (int64_t)ch * A.d + c;
        const int nb = chunk_end[ch] - chunk_begin[ch];
        float v[4], q[4], k[4];
        int s[4];
        if constexpr (M1) {
          load_vec<4>(v, p + S::kS * sec);
#pragma unroll
          for (int i = 0; i < 4; ++i) R.s[i] += v[i];
        }
        if constexpr (M2) {
          load_vec<4>(v, p + S::kDev * sec);
          load_vec<4>(q, p + S::kSq * sec);
          load_vec<4>(k, p + S::kShift * sec);
#pragma unroll
          for (int i = 0; i < 4; ++i) merge_moments(R.n, R.dev[i], R.sq[i], R.shift[i], nb, v[i], q[i], k[i]);
        }
        if constexpr (MAX) {
          load_vec<4>(v, p + S::kMaxV * sec);
          load_ivec4(s, reinterpret_cast<const int*>(p + S::kMaxS * sec));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool take = v[i] > R.maxv[i];
            R.maxv[i] = take ? v[i] : R.maxv[i];
            R.maxs[i] = take ? s[i] : R.maxs[i];
          }
        }
        if constexpr (MIN) {
          load_vec<4>(v, p + S::kMinV * sec);
          load_ivec4(s, reinterpret_cast<const int*>(p + S::kMinS * sec));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool take = v[i] < R.minv[i];
            R.minv[i] = take ? v[i] : R.minv[i];
            R.mins[i] = take ? s[i] : R.mins[i];
          }
        }
        R.n += nb;
      }
      multi_store<M1, M2, MAX, MIN>(A, row, c, R.n, R);
    }
  }
}

template <int G, bool M1, bool M2, bool MAX, bool MIN>
int launch_multi(const MultiArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  // one row per wave, uncapped grid: rows differ in length and the dispatcher balances fresh blocks (as spmm.hip)
  multi_kernel<G, M1, M2, MAX, MIN><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("multi_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    multi_chunk_kernel<G, M1, M2, MAX, MIN><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                                  sp->partial);
    RGBX_CHECK_LAUNCH("multi_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    multi_combine_kernel<M1, M2, MAX, MIN><<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->n_chunks, sp->long_row,
                                                                 sp->long_chunk_ptr, sp->chunk_begin, sp->chunk_end,
                                                                 sp->partial);
    RGBX_CHECK_LAUNCH("multi_combine_kernel");
  }
  return RGBX_OK;
}

#define RGBX_MULTI_CASE(K) \
  case K: return launch_multi<G, ((K) & 1) != 0, ((K) & 2) != 0, ((K) & 4) != 0, ((K) & 8) != 0>(A, sp, s);

template <int G>
int launch_multi_which(const MultiArgs& A, int key, const rgbx_row_split_t* sp, hipStream_t s) {
  switch (key) {  // bit 0: sum / mean, bit 1: var / std, bit 2: max, bit 3: min
    RGBX_MULTI_CASE(1) RGBX_MULTI_CASE(2) RGBX_MULTI_CASE(3) RGBX_MULTI_CASE(4) RGBX_MULTI_CASE(5)
    RGBX_MULTI_CASE(6) RGBX_MULTI_CASE(7) RGBX_MULTI_CASE(8) RGBX_MULTI_CASE(9) RGBX_MULTI_CASE(10)
    RGBX_MULTI_CASE(11) RGBX_MULTI_CASE(12) RGBX_MULTI_CASE(13) RGBX_MULTI_CASE(14) RGBX_MULTI_CASE(15)
  }
  return fail(RGBX_E_ARG, "spmm_multi: no statistic wanted");
}
#undef RGBX_MULTI_CASE

// ---- backward over the transposed CSR ------------------------------------------------------------------------------------

struct MultiBwdArgs {
  const int* rowptr;  // transposed CSR: rows = sources, col = targets
  const int* col;
  const int* t2f;
  const float* a;
  const float* b;
  const float* x;
  const float* ge[2];  // the extremum cotangents that are present, max before min
  const int* ae[2];    // their winning slots
  int64_t lda, ldb, ldx, ldge[2], ldae[2];
  float* gx;
  int64_t ldgx;
  int N, d;
  int skip_longer;
};

// Slots in flight per group, by the 16-byte fragments L a slot loads (a, b: one each; an extremum: cotangent + arg): four for
// L <= 2, two for L <= 4, one beyond (the all-terms form loads six per slot), which keeps every form at <= 64 VGPRs.
template <bool TA, bool TB, int NE>
constexpr int bwd_depth() {
  constexpr int L = (TA ? 1 : 0) + (TB ? 1 : 0) + 2 * NE;
  return L <= 2 ? 4 : (L <= 4 ? 2 : 1);
}

// acc += a[tgt] (+ the extremum cotangents whose arg names this slot's forward slot), accb += b[tgt]; groups folded on return.
template <int G, bool TA, bool TB, int NE>
__device__ __forceinline__ void bwd_slots(const MultiBwdArgs& A, int start, int end, int c, bool active, int lane, int g,
                                          float (&acc)[4], float (&accb)[4]) {
  constexpr int NG = kWave / G;
  constexpr int U = bwd_depth<TA, TB, NE>();
  constexpr int NE1 = NE > 0 ? NE : 1;
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    int mycol = 0, myfwd = -2;
    if (lane < n) {
      mycol = A.col[base + lane];
      if constexpr (NE > 0) myfwd = A.t2f[base + lane];
    }
    for (int k = 0; k < n; k += NG * U) {
      float va[U][4], vb[U][4], ve[NE1][U][4];
      int we[NE1][U][4];
      int fs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int tgt = __shfl(mycol, idx & 63);
        fs[u] = NE > 0 ? __shfl(myfwd, idx & 63) : -2;
        const bool ok = active && idx < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          va[u][i] = 0.f;
          vb[u][i] = 0.f;
#pragma unroll
          for (int e = 0; e < NE1; ++e) { ve[e][u][i] = 0.f; we[e][u][i] = -1; }
        }
        if (ok) {
          if constexpr (TA) load_vec<4>(va[u], A.a + (int64_t)tgt * A.lda + c);
          if constexpr (TB) load_vec<4>(vb[u], A.b + (int64_t)tgt * A.ldb + c);
#pragma unroll
          for (int e = 0; e < NE; ++e) {
            load_ivec4(we[e][u], A.ae[e] + (int64_t)tgt * A.ldae[e] + c);
            load_vec<4>(ve[e][u], A.ge[e] + (int64_t)tgt * A.ldge[e] + c);
          }
        } else {
          fs[u] = -2;  // matches no arg (arg >= -1)
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (TA) acc[i] += va[u][i];
          if constexpr (TB) accb[i] += vb[u][i];
#pragma unroll
          for (int e = 0; e < NE; ++e) acc[i] += we[e][u][i] == fs[u] ? ve[e][u][i] : 0.f;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (TA || NE > 0) acc[i] += __shfl_xor(acc[i], off);
      if constexpr (TB) accb[i] += __shfl_xor(accb[i], off);
    }
  }
}

// acc + x[row] * accb for columns c..c+3
template <bool TB>
__device__ __forceinline__ void bwd_finish(const MultiBwdArgs& A, int row, int c, float (&acc)[4], const float (&accb)[4]) {
  if constexpr (TB) {
    float xv[4];
    load_vec<4>(xv, A.x + (int64_t)row * A.ldx + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = fmaf(xv[i], accb[i], acc[i]);
  }
}

template <int G, bool TA, bool TB, int NE>
__global__ void __launch_bounds__(256) multi_bwd_kernel(const MultiBwdArgs A) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= A.N) return;
  const int start = __builtin_amdgcn_readfirstlane(A.rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(A.rowptr[row + 1]);
  if (A.skip_longer > 0 && end - start > A.skip_longer) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
  bwd_slots<G, TA, TB, NE>(A, start, end, c, active, lane, g, acc, accb);
  if (g == 0 && active) {
    bwd_finish<TB>(A, row, c, acc, accb);
    nt_store(A.gx + (int64_t)row * A.ldgx + c, acc);
  }
}

// One wave per chunk of a long transposed row: the chunk's finished contribution (x[row] * sum b folded in) into partial.
template <int G, bool TA, bool TB, int NE>
__global__ void __launch_bounds__(256)
multi_bwd_chunk_kernel(const MultiBwdArgs A, int n_chunks, const int* __restrict__ chunk_begin,
                       const int* __restrict__ chunk_end, const int* __restrict__ chunk_row, float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int g = lane / G;
  const int c = (lane % G) * 4;
  const bool active = c < A.d;
  const int wpb = blockDim.x >> 6;
  for (int ch = blockIdx.x * wpb + (threadIdx.x >> 6); ch < n_chunks; ch += gridDim.x * wpb) {
    const int start = __builtin_amdgcn_readfirstlane(chunk_begin[ch]);
    const int end = __builtin_amdgcn_readfirstlane(chunk_end[ch]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, accb[4] = {0.f, 0.f, 0.f, 0.f};
    bwd_slots<G, TA, TB, NE>(A, start, end, c, active, lane, g, acc, accb);
    if (g == 0 && active) {
      bwd_finish<TB>(A, chunk_row[ch], c, acc, accb);
      store_vec<4>(partial + (int64_t)ch * A.d + c, acc);
    }
  }
}

// One wave per long row: chunk contributions added in chunk order.
__global__ void __launch_bounds__(256)
multi_bwd_combine_kernel(const MultiBwdArgs A, int n_long, const int* __restrict__ long_row,
                         const int* __restrict__ long_chunk_ptr, const float* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  for (int r = blockIdx.x * wpb + (threadIdx.x >> 6); r < n_long; r += gridDim.x * wpb) {
    const int row = long_row[r];
    const int c0 = long_chunk_ptr[r], c1 = long_chunk_ptr[r + 1];
    for (int c = lane * 4; c < A.d; c += kWave * 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      for (int ch = c0; ch < c1; ++ch) {
        float p[4];
        load_vec<4>(p, partial + (int64_t)ch * A.d + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += p[i];
      }
      store_vec<4>(A.gx + (int64_t)row * A.ldgx + c, acc);
    }
  }
}

template <int G, bool TA, bool TB, int NE>
int launch_multi_bwd(const MultiBwdArgs& A, const rgbx_row_split_t* sp, hipStream_t s) {
  multi_bwd_kernel<G, TA, TB, NE><<<(int)cdiv(A.N, 4), 256, 0, s>>>(A);
  RGBX_CHECK_LAUNCH("multi_bwd_kernel");
  if (sp) {
    int64_t cb = cdiv(sp->n_chunks, 4);
    if (cb > kMaxGrid) cb = kMaxGrid;
    multi_bwd_chunk_kernel<G, TA, TB, NE><<<(int)cb, 256, 0, s>>>(A, sp->n_chunks, sp->chunk_begin, sp->chunk_end,
                                                                sp->chunk_row, sp->partial);
    RGBX_CHECK_LAUNCH("multi_bwd_chunk_kernel");
    int64_t lb = cdiv(sp->n_long, 4);
    if (lb > kMaxGrid) lb = kMaxGrid;
    multi_bwd_combine_kernel<<<(int)lb, 256, 0, s>>>(A, sp->n_long, sp->long_row, sp->long_chunk_ptr, sp->partial);
    RGBX_CHECK_LAUNCH("multi_bwd_combine_kernel");
  }
  return RGBX_OK;
}

#define RGBX_MULTI_BWD_CASE(K) \
  case K: return launch_multi_bwd<G, ((K) & 1) != 0, ((K) & 2) != 0, ((K) >> 2)>(A, sp, s);

template <int G>
int launch_multi_bwd_which(const MultiBwdArgs& A, int key, const rgbx_row_split_t* sp, hipStream_t s) {
  switch (key) {  // bit 0: a, bit 1: b, bits 2-3: the number of extremum terms
    RGBX_MULTI_BWD_CASE(1) RGBX_MULTI_BWD_CASE(2) RGBX_MULTI_BWD_CASE(3) RGBX_MULTI_BWD_CASE(4) RGBX_MULTI_BWD_CASE(5)
    RGBX_MULTI_BWD_CASE(6) RGBX_MULTI_BWD_CASE(7) RGBX_MULTI_BWD_CASE(8) RGBX_MULTI_BWD_CASE(9) RGBX_MULTI_BWD_CASE(10)
    RGBX_MULTI_BWD_CASE(11)
  }
  return fail(RGBX_E_ARG, "multi_bwd: no term given");
}
#undef RGBX_MULTI_BWD_CASE

const rgbx_row_split_t* usable_split(const rgbx_row_split_t* split) {
  return (split && split->threshold > 0 && split->n_chunks > 0) ? split : nullptr;
}

bool complete_split(const rgbx_row_split_t* sp) {
  return sp->n_long > 0 && sp->chunk_begin && sp->chunk_end && sp->chunk_row && sp->long_row && sp->long_chunk_ptr &&
         sp->partial && aligned16(sp->partial);
}

bool vec_ok(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

}  // namespace
}  // namespace rgbx

using namespace rgbx;

#define RGBX_BY_LANES(FN, ...)                    \
  do {                                            \
    const int lanes_ = (int)(d / 4);              \
    if (lanes_ <= 1) return FN<1>(__VA_ARGS__);   \
    if (lanes_ <= 2) return FN<2>(__VA_ARGS__);   \
    if (lanes_ <= 4) return FN<4>(__VA_ARGS__);   \
    if (lanes_ <= 8) return FN<8>(__VA_ARGS__);   \
    if (lanes_ <= 16) return FN<16>(__VA_ARGS__); \
    if (lanes_ <= 32) return FN<32>(__VA_ARGS__); \
    return FN<64>(__VA_ARGS__);                   \
  } while (0)

extern "C" int rgbx_spmm_csr_multi_supported(int64_t d) { return d >= 4 && d % 4 == 0 && d <= 256; }

extern "C" int rgbx_spmm_csr_multi_partial_words(int64_t n_chunks, int64_t d, int which, int64_t* words) {
  if (!words) return fail(RGBX_E_ARG, "spmm_multi_partial_words: null pointer");
  if (n_chunks < 0 || d < 0) return fail(RGBX_E_ARG, "spmm_multi_partial_words: negative size");
  if (which <= 0 || which > RGBX_MULTI_ALL) return fail(RGBX_E_ARG, "spmm_multi_partial_words: `which` names no statistic");
  *words = n_chunks * d * sections_of(which);
  return RGBX_OK;
}

extern "C" int rgbx_spmm_csr_multi_f32(const int32_t* rowptr, const int32_t* col, const float* x, int64_t ldx,
                                       const rgbx_multi_out_t* out, int64_t N, int64_t d, const rgbx_row_split_t* split,
                                       rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "spmm_multi: negative size");
  if (!rowptr || !col || !x || !out) return fail(RGBX_E_ARG, "spmm_multi: null pointer");
  const rgbx_multi_out_t o = *out;
  const int key = ((o.sum || o.mean) ? 1 : 0) | ((o.var || o.std) ? 2 : 0) | (o.max ? 4 : 0) | (o.min ? 8 : 0);
  if (key == 0) return fail(RGBX_E_ARG, "spmm_multi: no statistic wanted (every output pointer is NULL)");
  if ((o.argmax && !o.max) || (o.argmin && !o.min)) return fail(RGBX_E_ARG, "spmm_multi: arg wanted without its extremum");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "spmm_multi: N exceeds int32");
  if (!rgbx_spmm_csr_multi_supported(d))
    return fail(RGBX_E_SHAPE, "spmm_multi: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld); pad or cut the rows", (long long)d);
  const void* ptrs[8] = {o.sum, o.mean, o.var, o.std, o.max, o.argmax, o.min, o.argmin};
  const int64_t lds[8] = {o.ld_sum, o.ld_mean, o.ld_var, o.ld_std, o.ld_max, o.ld_argmax, o.ld_min, o.ld_argmin};
  if (ldx < d) return fail(RGBX_E_ARG, "spmm_multi: leading dimension < d");
  for (int i = 0; i < 8; ++i) {
    if (ptrs[i] && lds[i] < d) return fail(RGBX_E_ARG, "spmm_multi: leading dimension < d");
    if (ptrs[i] && ptrs[i] == (const void*)x) return fail(RGBX_E_ARG, "spmm_multi: an output must not alias x");
  }
  if (!vec_ok(x, ldx)) return fail(RGBX_E_ALIGN, "spmm_multi: x must be 16-byte aligned with ld %% 4 == 0");
  for (int i = 0; i < 8; ++i)
    if (ptrs[i] && !vec_ok(ptrs[i], lds[i]))
      return fail(RGBX_E_ALIGN, "spmm_multi: every output must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "spmm_multi: incomplete row-split plan");
  MultiArgs A{rowptr, col, x, ldx, o, (int)N, (int)d, sp ? sp->threshold : 0};
  hipStream_t s = (hipStream_t)stream;
  RGBX_BY_LANES(launch_multi_which, A, key, sp, s);
}

extern "C" int rgbx_multi_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const int32_t* t2f,
                                  const rgbx_multi_grad_t* terms, float* gx, int64_t ldgx, int64_t N, int64_t d,
                                  const rgbx_row_split_t* split, rgbx_stream_t stream) {
  if (N < 0 || d < 0) return fail(RGBX_E_ARG, "multi_bwd: negative size");
  if (!rowptr_t || !col_t || !terms || !gx) return fail(RGBX_E_ARG, "multi_bwd: null pointer");
  const rgbx_multi_grad_t t = *terms;
  if ((t.gmax != nullptr) != (t.argmax != nullptr) || (t.gmin != nullptr) != (t.argmin != nullptr))
    return fail(RGBX_E_ARG, "multi_bwd: an extremum term needs both its cotangent and its arg");
  const int ne = (t.gmax ? 1 : 0) + (t.gmin ? 1 : 0);
  if (ne > 0 && !t2f) return fail(RGBX_E_ARG, "multi_bwd: null pointer (t2f)");
  if (t.b && !t.x) return fail(RGBX_E_ARG, "multi_bwd: the b term needs x");
  const int key = (t.a ? 1 : 0) | (t.b ? 2 : 0) | (ne << 2);
  if (key == 0) return fail(RGBX_E_ARG, "multi_bwd: no term given");
  if (N >= INT32_MAX) return fail(RGBX_E_RANGE, "multi_bwd: N exceeds int32");
  if (!rgbx_spmm_csr_multi_supported(d))
    return fail(RGBX_E_SHAPE, "multi_bwd: needs d %% 4 == 0 and 4 <= d <= 256 (got %lld); pad or cut the rows", (long long)d);
  const void* ptrs[7] = {t.a, t.b, t.b ? t.x : nullptr, t.gmax, t.argmax, t.gmin, t.argmin};
  const int64_t lds[7] = {t.ld_a, t.ld_b, t.ld_x, t.ld_gmax, t.ld_argmax, t.ld_gmin, t.ld_argmin};
  if (ldgx < d) return fail(RGBX_E_ARG, "multi_bwd: leading dimension < d");
  for (int i = 0; i < 7; ++i) {
    if (ptrs[i] && lds[i] < d) return fail(RGBX_E_ARG, "multi_bwd: leading dimension < d");
    if (ptrs[i] && ptrs[i] == (const void*)gx) return fail(RGBX_E_ARG, "multi_bwd: gx must not alias an input");
  }
  if (!vec_ok(gx, ldgx)) return fail(RGBX_E_ALIGN, "multi_bwd: gx must be 16-byte aligned with ld %% 4 == 0");
  for (int i = 0; i < 7; ++i)
    if (ptrs[i] && !vec_ok(ptrs[i], lds[i]))
      return fail(RGBX_E_ALIGN, "multi_bwd: every input must be 16-byte aligned with ld %% 4 == 0");
  if (N == 0) return RGBX_OK;
  const rgbx_row_split_t* sp = usable_split(split);
  if (sp && !complete_split(sp)) return fail(RGBX_E_ARG, "multi_bwd: incomplete row-split plan");
  MultiBwdArgs A{};
  A.rowptr = rowptr_t; A.col = col_t; A.t2f = t2f;
  A.a = t.a; A.lda = t.ld_a; A.b = t.b; A.ldb = t.ld_b; A.x = t.x; A.ldx = t.ld_x;
  int e = 0;
  if (t.gmax) { A.ge[e] = t.gmax; A.ldge[e] = t.ld_gmax; A.ae[e] = t.argmax; A.ldae[e] = t.ld_argmax; ++e; }
  if (t.gmin) { A.ge[e] = t.gmin; A.ldge[e] = t.ld_gmin; A.ae[e] = t.argmin; A.ldae[e] = t.ld_argmin; ++e; }
  A.gx = gx; A.ldgx = ldgx; A.N = (int)N; A.d = (int)d; A.skip_longer = sp ? sp->threshold : 0;
  hipStream_t s = (hipStream_t)stream;
  RGBX_BY_LANES(launch_multi_bwd_which, A, key, sp, s);
}
