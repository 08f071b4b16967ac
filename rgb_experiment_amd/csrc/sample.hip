// Neighbour sampling: fan-out mini-batches drawn on the device (GraphSAGE's sampler; the reference trains full-batch only,
// itexperiments.py:417-473). One hop = count + scan (how many slots every row keeps), pick (which ones), frontier (the
// distinct new nodes, ascending, get the next local ids), relabel (global -> local ids, slot -> input edge id).
//
// The draw. Row g keeps, of its deg slots of the forward CSR, the min(k, deg) slots with the smallest 64-bit keys
//   key(t) = draw32(seed[0], seed[1], kStreamSample + hop, g, t) << 32 | t,      t = slot - rowptr[g],
// written in ascending slot order: a uniform draw without replacement that depends on (seed, hop, g, t) alone, not on
// which lane, wave or kernel handles the row. Within a row the DRAWS are already distinct: mix32 is a bijection of 32-bit
// words (xor-shifts and odd multipliers), and for a fixed (seed, stream, g) its innermost argument is a constant plus
// t * 0x9E3779B9, an odd multiple of t, so draw32 maps the row's t < 2^32 one to one. "The k smallest keys" is therefore
// "the k smallest draws", and the low word of the key never decides anything.
//
// Selection = radix select of the k-th smallest draw, most significant bits first, over the 32 bits of the key's upper
// word; a slot is kept when key <= (that draw << 32 | 0xFFFFFFFF). Three kernels by row length:
//   deg <= kShortRowSlots (64)          a group of kGroupLanes (16) lanes per row, four rows per wave; a lane holds its
//                                       <= 4 keys in registers; one bit per round, counts summed inside the group
//   deg <= kWaveRowSlots (1024)         one wave per row; a lane recomputes the keys of its slots every round; one bit per
//                                       round, counts summed over the wave; stops as soon as the candidates that are left
//                                       are exactly the ones still to take
//   longer (hub rows)                   one workgroup of 256 threads per row; eight bits per round through a 256-bin LDS
//                                       histogram (integer atomicAdd: counts, order-independent); same early stop
// Rows with deg <= k (and every row under k = -1) are copied by the kernel of their length class. The kept slots' output
// positions come from ballots (and, in the workgroup kernel, per-wave counts in LDS) — no atomics decide a position.
#include "rgbx_common.h"
#include "rgbx_rng.h"

#include <rocprim/rocprim.hpp>

namespace rgbx {
namespace {

constexpr uint32_t kStreamSample = 0x082EFA98u;
constexpr int kGroupLanes = 16;
constexpr int kShortRowSlots = 64;
constexpr int kGroupKeys = kShortRowSlots / kGroupLanes;
constexpr int kWaveRowSlots = 1024;
constexpr int kBlock = 256;

__device__ __forceinline__ uint64_t sample_key(uint32_t s0, uint32_t s1, uint32_t stream, uint32_t g, uint32_t t) {
  return ((uint64_t)draw32(s0, s1, stream, g, t) << 32) | (uint64_t)t;
}

__device__ __forceinline__ int row_degree(const int32_t* __restrict__ rowptr, int N, int g, int* begin) {
  if (g < 0 || g >= N) {
    *begin = 0;
    return 0;
  }
  const int b = rowptr[g];
  *begin = b;
  const int d = rowptr[g + 1] - b;
  return d > 0 ? d : 0;
}

__device__ __forceinline__ int kept_of(int deg, int fanout) { return (fanout < 0 || fanout >= deg) ? deg : fanout; }

// cnt[r] = slots row r keeps (cnt[n_rows] = 0: the scan's total lands there); classes[0] / [1] = rows of the wave / the
// workgroup length class
__global__ void __launch_bounds__(kBlock)
sample_count_kernel(const int32_t* __restrict__ rowptr, int N, const int32_t* __restrict__ rows, int n_rows, int fanout,
                    int32_t* __restrict__ cnt, int32_t* __restrict__ classes) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r <= n_rows; r += (int64_t)gridDim.x * kBlock) {
    if (r == n_rows) {
      cnt[r] = 0;
      continue;
    }
    int begin;
    const int deg = row_degree(rowptr, N, rows[r], &begin);
    cnt[r] = kept_of(deg, fanout);
    if (classes && deg > kShortRowSlots) atomicAdd(&classes[deg > kWaveRowSlots ? 1 : 0], 1);
  }
}

// ---- short rows: kGroupLanes lanes per row ----------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
sample_pick_group_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                         const int32_t* __restrict__ rows, int n_rows, int fanout, const uint32_t* __restrict__ seed,
                         uint32_t stream, const int32_t* __restrict__ out_rowptr, int32_t* __restrict__ out_col,
                         int32_t* __restrict__ out_slot) {
  constexpr int kRowsPerBlock = kBlock / kGroupLanes;
  const int gl = threadIdx.x & (kGroupLanes - 1);
  const int shift = (threadIdx.x & (kWave - 1)) & ~(kGroupLanes - 1);  // first lane of this group in its wave
  const int64_t r = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kGroupLanes;
  // every lane of the wave runs the same rounds (the shuffles and ballots below need the whole wave converged): a group
  // without a row of this class carries deg = 0
  int begin = 0, deg = 0, g = 0, obase = 0;
  if (r < n_rows) {
    g = rows[r];
    deg = row_degree(rowptr, N, g, &begin);
    if (deg > kShortRowSlots) deg = 0;
    obase = out_rowptr[r];
  }
  const int keep = kept_of(deg, fanout);
  const bool select = keep < deg;
  const uint32_t s0 = seed[0], s1 = seed[1];
  uint64_t key[kGroupKeys];
#pragma unroll
  for (int i = 0; i < kGroupKeys; ++i) {
    const int t = gl + i * kGroupLanes;
    key[i] = (select && t < deg) ? sample_key(s0, s1, stream, (uint32_t)g, (uint32_t)t) : ~0ull;
  }
  // radix select, one bit per round over bits 63..32 (the draw; distinct within a row, see the head of the file). A
  // padding key (all ones) is never counted: only zero bits are.
  uint64_t prefix = 0, mask = 0;
  int krem = keep;
  for (int round = 0; round < 32; ++round) {
    const uint64_t bit = 1ull << (63 - round);
    int c0 = 0;
#pragma unroll
    for (int i = 0; i < kGroupKeys; ++i) c0 += ((key[i] & mask) == prefix && !(key[i] & bit)) ? 1 : 0;
#pragma unroll
    for (int o = kGroupLanes / 2; o > 0; o >>= 1) c0 += __shfl_xor(c0, o, kGroupLanes);
    if (krem > c0) {
      prefix |= bit;
      krem -= c0;
    }
    mask |= bit;
  }
  prefix |= 0xFFFFFFFFull;  // the k-th smallest draw, with whatever slot index goes with it
  int running = 0;
#pragma unroll
  for (int i = 0; i < kGroupKeys; ++i) {
    const int t = gl + i * kGroupLanes;
    const bool kf = t < deg && (!select || key[i] <= prefix);
    const uint32_t gm = (uint32_t)(__ballot(kf) >> shift) & ((1u << kGroupLanes) - 1u);
    const int pos = running + __popc(gm & ((1u << gl) - 1u));
    if (kf && pos < keep) {
      out_col[obase + pos] = col[begin + t];
      out_slot[obase + pos] = begin + t;
    }
    running += __popc(gm);
  }
}

// ---- medium rows: one wave per row -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
sample_pick_wave_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                        const int32_t* __restrict__ rows, int n_rows, int fanout, const uint32_t* __restrict__ seed,
                        uint32_t stream, const int32_t* __restrict__ out_rowptr, int32_t* __restrict__ out_col,
                        int32_t* __restrict__ out_slot) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wpb = kBlock / kWave;
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t r = (int64_t)blockIdx.x * wpb + threadIdx.x / kWave; r < n_rows; r += (int64_t)gridDim.x * wpb) {
    const int g = rows[r];
    int begin;
    const int deg = row_degree(rowptr, N, g, &begin);
    if (deg <= kShortRowSlots || deg > kWaveRowSlots) continue;  // (uniform over the wave)
    const int obase = out_rowptr[r];
    const int keep = kept_of(deg, fanout);
    if (keep == deg) {
      for (int t = lane; t < deg; t += kWave) {
        out_col[obase + t] = col[begin + t];
        out_slot[obase + t] = begin + t;
      }
      continue;
    }
    uint64_t prefix = 0, mask = 0;
    int krem = keep, ncand = deg;
    for (int round = 0; round < 32; ++round) {
      const uint64_t bit = 1ull << (63 - round);
      int c0 = 0;
      for (int t = lane; t < deg; t += kWave) {
        const uint64_t k = sample_key(s0, s1, stream, (uint32_t)g, (uint32_t)t);
        c0 += ((k & mask) == prefix && !(k & bit)) ? 1 : 0;
      }
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) c0 += __shfl_xor(c0, o, kWave);
      if (krem > c0) {
        prefix |= bit;
        krem -= c0;
        ncand -= c0;
      } else {
        ncand = c0;
      }
      mask |= bit;
      if (ncand == krem) {  // every candidate that is left is taken: the threshold is the largest key under the prefix
        prefix |= bit - 1;
        break;
      }
    }
    prefix |= 0xFFFFFFFFull;  // (distinct draws: the loop has stopped by bit 32 at the latest)
    int running = 0;
    for (int base = 0; base < deg; base += kWave) {
      const int t = base + lane;
      const bool kf = t < deg && sample_key(s0, s1, stream, (uint32_t)g, (uint32_t)t) <= prefix;
      const uint64_t bal = __ballot(kf);
      const int pos = running + __popcll(bal & ((1ull << lane) - 1ull));
      if (kf && pos < keep) {
        out_col[obase + pos] = col[begin + t];
        out_slot[obase + pos] = begin + t;
      }
      running += __popcll(bal);
    }
  }
}

// ---- hub rows: one workgroup per row -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
sample_pick_block_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                         const int32_t* __restrict__ rows, int n_rows, int fanout, const uint32_t* __restrict__ seed,
                         uint32_t stream, const int32_t* __restrict__ out_rowptr, int32_t* __restrict__ out_col,
                         int32_t* __restrict__ out_slot) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sh_prefix, sh_mask;
  __shared__ int sh_krem, sh_done;
  __shared__ int wave_cnt[kBlock / kWave];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  const uint32_t s0 = seed[0], s1 = seed[1];
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int g = rows[r];
    int begin;
    const int deg = row_degree(rowptr, N, g, &begin);
    if (deg <= kWaveRowSlots) continue;  // (uniform over the workgroup)
    const int obase = out_rowptr[r];
    const int keep = kept_of(deg, fanout);
    if (keep == deg) {
      for (int t = tid; t < deg; t += kBlock) {
        out_col[obase + t] = col[begin + t];
        out_slot[obase + t] = begin + t;
      }
      continue;
    }
    __syncthreads();  // the previous row's readers of the shared words are done
    if (tid == 0) {
      sh_prefix = 0;
      sh_mask = 0;
      sh_krem = keep;
      sh_done = 0;
    }
    // digits of 8 bits over the draw, most significant first (distinct draws: the last digit leaves one candidate)
    for (int sft = 56; sft >= 32; sft -= 8) {
      hist[tid] = 0;
      __syncthreads();
      const uint64_t prefix = sh_prefix, mask = sh_mask;
      for (int t = tid; t < deg; t += kBlock) {
        const uint64_t k = sample_key(s0, s1, stream, (uint32_t)g, (uint32_t)t);
        if ((k & mask) == prefix) atomicAdd(&hist[(uint32_t)(k >> sft) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {  // the digit in which the krem-th smallest candidate lies
        int krem = sh_krem;
        uint32_t d = 0;
        while (d < 255u && (uint32_t)krem > hist[d]) krem -= (int)hist[d++];
        sh_krem = krem;
        sh_mask = mask | (255ull << sft);
        uint64_t p = prefix | ((uint64_t)d << sft);
        if ((int)hist[d] == krem || sft == 32) {  // all of that digit's candidates are taken
          p |= (1ull << sft) - 1ull;
          sh_done = 1;
        }
        sh_prefix = p;
      }
      __syncthreads();
      if (sh_done) break;
    }
    const uint64_t T = sh_prefix;
    int running = 0;
    for (int base = 0; base < deg; base += kBlock) {
      const int t = base + tid;
      const bool kf = t < deg && sample_key(s0, s1, stream, (uint32_t)g, (uint32_t)t) <= T;
      const uint64_t bal = __ballot(kf);
      if (lane == 0) wave_cnt[wave] = __popcll(bal);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kBlock / kWave; ++w) {
        const int c = wave_cnt[w];
        before += w < wave ? c : 0;
        total += c;
      }
      const int pos = running + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (kf && pos < keep) {
        out_col[obase + pos] = col[begin + t];
        out_slot[obase + pos] = begin + t;
      }
      running += total;
      __syncthreads();
    }
  }
}

// ---- frontier ----------------------------------------------------------------------------------------------------------
// keys[p] = the candidate where it is not in the batch yet, else the sentinel N (sorts behind every id)
__global__ void __launch_bounds__(kBlock)
frontier_mark_kernel(const int32_t* __restrict__ cand, int64_t n, const int32_t* __restrict__ local_of, int N,
                     uint32_t* __restrict__ keys) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += (int64_t)gridDim.x * kBlock) {
    const int c = cand[p];
    keys[p] = (c >= 0 && c < N && local_of[c] < 0) ? (uint32_t)c : (uint32_t)N;
  }
}

// head[i] = 1 where sorted[i] is the first of its value and no sentinel
__global__ void __launch_bounds__(kBlock)
frontier_head_kernel(const uint32_t* __restrict__ sorted, int64_t n, int N, int32_t* __restrict__ head) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t k = sorted[i];
    head[i] = (k != (uint32_t)N && (i == 0 || sorted[i - 1] != k)) ? 1 : 0;
  }
}

// the i-th distinct new id (ascending) gets local id first_local + i
__global__ void __launch_bounds__(kBlock)
frontier_assign_kernel(const uint32_t* __restrict__ sorted, const int32_t* __restrict__ pos, int64_t n, int N,
                       int first_local, int32_t* __restrict__ local_of, int32_t* __restrict__ new_ids,
                       int32_t* __restrict__ count) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint32_t k = sorted[i];
    const bool head = k != (uint32_t)N && (i == 0 || sorted[i - 1] != k);
    const int p = pos[i];
    if (head) {
      local_of[k] = first_local + p;
      new_ids[p] = (int32_t)k;
    }
    if (i == n - 1) *count = p + (head ? 1 : 0);
  }
}

__global__ void __launch_bounds__(kBlock)
set_local_kernel(const int32_t* __restrict__ ids, int64_t n, int first_local, int32_t* __restrict__ local_of, int N) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int g = ids[i];
    if (g >= 0 && g < N) local_of[g] = first_local < 0 ? -1 : first_local + (int)i;
  }
}

// sampled edge p of row r (out_rowptr[r] <= p < out_rowptr[r + 1]): source = local id of its column, target = first_row + r,
// e_id = the input edge behind its slot
__global__ void __launch_bounds__(kBlock)
relabel_kernel(const int32_t* __restrict__ out_rowptr, int n_rows, const int32_t* __restrict__ col,
               const int32_t* __restrict__ slot, int64_t n_edges, const int32_t* __restrict__ local_of, int N,
               const int32_t* __restrict__ perm, int first_row, int64_t* __restrict__ src, int64_t* __restrict__ dst,
               int64_t* __restrict__ e_id) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n_edges; p += (int64_t)gridDim.x * kBlock) {
    int lo = 0, hi = n_rows;  // the last r with out_rowptr[r] <= p
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if ((int64_t)out_rowptr[mid] <= p) lo = mid; else hi = mid;
    }
    const int c = col[p];
    src[p] = (c >= 0 && c < N) ? (int64_t)local_of[c] : -1;
    dst[p] = (int64_t)first_row + lo;
    if (e_id) e_id[p] = perm ? (int64_t)perm[slot[p]] : (int64_t)slot[p];
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int grid_for(int64_t n) {
  int64_t g = cdiv(n > 0 ? n : 1, kBlock);
  return (int)(g < kMaxGrid ? g : kMaxGrid);
}

int id_bits(int64_t N) {  // keys lie in [0, N]
  int b = 1;
  while (b < 32 && ((uint64_t)1 << b) <= (uint64_t)N) ++b;
  return b;
}

// count: [cnt int32 (n_rows + 1)] [scan temp]
struct CountLayout {
  size_t cnt, scan_tmp, total;
};

int count_layout(int64_t n_rows, CountLayout* L) {
  const size_t m = (size_t)n_rows + 1;
  int32_t* np = nullptr;
  size_t st = 0;
  hipError_t e = rocprim::exclusive_scan(nullptr, st, np, np, (int32_t)0, m, rocprim::plus<int32_t>(), (hipStream_t) nullptr);
  if (e != hipSuccess) return hip_fail(e, "exclusive_scan(size query)");
  L->cnt = align256(m * sizeof(int32_t));
  L->scan_tmp = align256(st);
  L->total = L->cnt + L->scan_tmp;
  return RGBX_OK;
}

// frontier: [keys uint32 n] [sorted uint32 n] [head / pos int32 n] [sort or scan temp]
struct FrontierLayout {
  size_t slab, tmp, total;
};

int frontier_layout(int64_t n, int64_t N, FrontierLayout* L) {
  const size_t m = (size_t)(n > 0 ? n : 1);
  uint32_t* nk = nullptr;
  int32_t* np = nullptr;
  size_t st = 0, ct = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, st, nk, nk, m, 0, id_bits(N), (hipStream_t) nullptr);
  if (e != hipSuccess) return hip_fail(e, "radix_sort_keys(size query)");
  e = rocprim::exclusive_scan(nullptr, ct, np, np, (int32_t)0, m, rocprim::plus<int32_t>(), (hipStream_t) nullptr);
  if (e != hipSuccess) return hip_fail(e, "exclusive_scan(size query)");
  L->slab = align256(m * sizeof(uint32_t));
  L->tmp = align256(st > ct ? st : ct);
  L->total = 3 * L->slab + L->tmp;
  return RGBX_OK;
}

}  // namespace
}  // namespace rgbx

using namespace rgbx;

extern "C" int rgbx_sample_workspace_bytes(int64_t n_rows, int64_t n_cand, int64_t N, size_t* bytes) {
  if (!bytes || n_rows < 0 || n_cand < 0 || N < 0) return fail(RGBX_E_ARG, "sample_workspace_bytes: bad argument");
  if (n_rows >= INT32_MAX || n_cand >= INT32_MAX || N >= INT32_MAX)
    return fail(RGBX_E_RANGE, "sample_workspace_bytes: size exceeds int32");
  CountLayout C;
  FrontierLayout F;
  if (int rc = count_layout(n_rows, &C)) return rc;
  if (int rc = frontier_layout(n_cand, N, &F)) return rc;
  *bytes = C.total > F.total ? C.total : F.total;
  return RGBX_OK;
}

extern "C" int rgbx_sample_count(const int32_t* rowptr, int64_t N, const int32_t* rows, int64_t n_rows, int fanout,
                                 int32_t* out_rowptr, int32_t* class_rows, void* workspace, size_t workspace_bytes,
                                 rgbx_stream_t stream) {
  if (n_rows < 0 || N < 0) return fail(RGBX_E_ARG, "sample_count: negative size");
  if (fanout == 0 || fanout < -1) return fail(RGBX_E_ARG, "sample_count: fan-out %d (>= 1, or -1 for every slot)", fanout);
  if (n_rows >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "sample_count: size exceeds int32");
  if (!rowptr || !out_rowptr || !workspace || (n_rows > 0 && !rows)) return fail(RGBX_E_ARG, "sample_count: null pointer");
  CountLayout L;
  if (int rc = count_layout(n_rows, &L)) return rc;
  if (workspace_bytes < L.total) return fail(RGBX_E_WS, "sample_count: workspace %zu < %zu bytes", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  int32_t* cnt = static_cast<int32_t*>(workspace);
  void* tmp = static_cast<char*>(workspace) + L.cnt;
  if (class_rows) RGBX_HIP(hipMemsetAsync(class_rows, 0, 2 * sizeof(int32_t), s));
  sample_count_kernel<<<grid_for(n_rows + 1), kBlock, 0, s>>>(rowptr, (int)N, rows, (int)n_rows, fanout, cnt, class_rows);
  RGBX_CHECK_LAUNCH("sample_count_kernel");
  size_t st = L.scan_tmp;
  RGBX_HIP(rocprim::exclusive_scan(tmp, st, cnt, out_rowptr, (int32_t)0, (size_t)n_rows + 1, rocprim::plus<int32_t>(), s));
  return RGBX_OK;
}

extern "C" int rgbx_sample_pick(const int32_t* rowptr, const int32_t* col, int64_t N, const int32_t* rows, int64_t n_rows,
                                int fanout, const uint32_t* seed, int hop, const int32_t* out_rowptr, int32_t* out_col,
                                int32_t* out_slot, int classes, rgbx_stream_t stream) {
  if (n_rows < 0 || N < 0 || hop < 0) return fail(RGBX_E_ARG, "sample_pick: negative size or hop");
  if (fanout == 0 || fanout < -1) return fail(RGBX_E_ARG, "sample_pick: fan-out %d (>= 1, or -1 for every slot)", fanout);
  if (n_rows >= INT32_MAX || N >= INT32_MAX) return fail(RGBX_E_RANGE, "sample_pick: size exceeds int32");
  if (n_rows == 0) return RGBX_OK;
  if (!rowptr || !col || !rows || !seed || !out_rowptr || !out_col || !out_slot)
    return fail(RGBX_E_ARG, "sample_pick: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t strm = kStreamSample + (uint32_t)hop;
  if (classes & RGBX_SAMPLE_SHORT_ROWS) {
    const int64_t blocks = cdiv(n_rows, kBlock / kGroupLanes);
    sample_pick_group_kernel<<<(unsigned)blocks, kBlock, 0, s>>>(rowptr, col, (int)N, rows, (int)n_rows, fanout, seed, strm,
                                                                 out_rowptr, out_col, out_slot);
    RGBX_CHECK_LAUNCH("sample_pick_group_kernel");
  }
  if (classes & RGBX_SAMPLE_WAVE_ROWS) {
    int64_t blocks = cdiv(n_rows, kBlock / kWave);
    if (blocks > kMaxGrid) blocks = kMaxGrid;
    sample_pick_wave_kernel<<<(int)blocks, kBlock, 0, s>>>(rowptr, col, (int)N, rows, (int)n_rows, fanout, seed, strm,
                                                          out_rowptr, out_col, out_slot);
    RGBX_CHECK_LAUNCH("sample_pick_wave_kernel");
  }
  if (classes & RGBX_SAMPLE_HUB_ROWS) {
    const int64_t blocks = n_rows < 2048 ? n_rows : 2048;
    sample_pick_block_kernel<<<(int)blocks, kBlock, 0, s>>>(rowptr, col, (int)N, rows, (int)n_rows, fanout, seed, strm,
                                                           out_rowptr, out_col, out_slot);
    RGBX_CHECK_LAUNCH("sample_pick_block_kernel");
  }
  return RGBX_OK;
}

extern "C" int rgbx_sample_frontier(const int32_t* cand, int64_t n_cand, int32_t* local_of, int64_t N, int64_t first_local,
                                    int32_t* new_ids, int32_t* count, void* workspace, size_t workspace_bytes,
                                    rgbx_stream_t stream) {
  if (n_cand < 0 || N < 0 || first_local < 0) return fail(RGBX_E_ARG, "sample_frontier: negative size");
  if (n_cand >= INT32_MAX || N >= INT32_MAX || first_local >= INT32_MAX)
    return fail(RGBX_E_RANGE, "sample_frontier: size exceeds int32");
  if (!count || (n_cand > 0 && (!cand || !local_of || !new_ids || !workspace)))
    return fail(RGBX_E_ARG, "sample_frontier: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_cand == 0) {
    RGBX_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), s));
    return RGBX_OK;
  }
  FrontierLayout L;
  if (int rc = frontier_layout(n_cand, N, &L)) return rc;
  if (workspace_bytes < L.total)
    return fail(RGBX_E_WS, "sample_frontier: workspace %zu < %zu bytes", workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws);
  uint32_t* sorted = reinterpret_cast<uint32_t*>(ws + L.slab);
  int32_t* pos = reinterpret_cast<int32_t*>(ws + 2 * L.slab);
  void* tmp = ws + 3 * L.slab;
  const int grid = grid_for(n_cand);
  frontier_mark_kernel<<<grid, kBlock, 0, s>>>(cand, n_cand, local_of, (int)N, keys);
  RGBX_CHECK_LAUNCH("frontier_mark_kernel");
  size_t st = L.tmp;
  RGBX_HIP(rocprim::radix_sort_keys(tmp, st, keys, sorted, (size_t)n_cand, 0, id_bits(N), s));
  int32_t* head = reinterpret_cast<int32_t*>(keys);  // the unsorted keys are not read again
  frontier_head_kernel<<<grid, kBlock, 0, s>>>(sorted, n_cand, (int)N, head);
  RGBX_CHECK_LAUNCH("frontier_head_kernel");
  st = L.tmp;
  RGBX_HIP(rocprim::exclusive_scan(tmp, st, head, pos, (int32_t)0, (size_t)n_cand, rocprim::plus<int32_t>(), s));
  frontier_assign_kernel<<<grid, kBlock, 0, s>>>(sorted, pos, n_cand, (int)N, (int)first_local, local_of, new_ids, count);
  RGBX_CHECK_LAUNCH("frontier_assign_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_sample_set_local(const int32_t* ids, int64_t n, int64_t first_local, int32_t* local_of, int64_t N,
                                     rgbx_stream_t stream) {
  if (n < 0 || N < 0) return fail(RGBX_E_ARG, "sample_set_local: negative size");
  if (n >= INT32_MAX || N >= INT32_MAX || first_local >= INT32_MAX)
    return fail(RGBX_E_RANGE, "sample_set_local: size exceeds int32");
  if (n == 0) return RGBX_OK;
  if (!ids || !local_of) return fail(RGBX_E_ARG, "sample_set_local: null pointer");
  set_local_kernel<<<grid_for(n), kBlock, 0, (hipStream_t)stream>>>(ids, n, first_local < 0 ? -1 : (int)first_local,
                                                                   local_of, (int)N);
  RGBX_CHECK_LAUNCH("set_local_kernel");
  return RGBX_OK;
}

extern "C" int rgbx_sample_relabel(const int32_t* out_rowptr, int64_t n_rows, const int32_t* col, const int32_t* slot,
                                   int64_t n_edges, const int32_t* local_of, int64_t N, const int32_t* perm,
                                   int64_t first_row, int64_t* src, int64_t* dst, int64_t* e_id, rgbx_stream_t stream) {
  if (n_rows < 0 || n_edges < 0 || N < 0 || first_row < 0) return fail(RGBX_E_ARG, "sample_relabel: negative size");
  if (n_rows >= INT32_MAX || n_edges >= INT32_MAX || N >= INT32_MAX || first_row >= INT32_MAX)
    return fail(RGBX_E_RANGE, "sample_relabel: size exceeds int32");
  if (n_edges == 0) return RGBX_OK;
  if (n_rows == 0) return fail(RGBX_E_ARG, "sample_relabel: edges without rows");
  if (!out_rowptr || !col || !slot || !local_of || !src || !dst) return fail(RGBX_E_ARG, "sample_relabel: null pointer");
  relabel_kernel<<<grid_for(n_edges), kBlock, 0, (hipStream_t)stream>>>(out_rowptr, (int)n_rows, col, slot, n_edges, local_of,
                                                                       (int)N, perm, (int)first_row, src, dst, e_id);
  RGBX_CHECK_LAUNCH("relabel_kernel");
  return RGBX_OK;
}
