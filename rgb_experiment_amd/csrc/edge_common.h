// What the edge-message families (resgated.hip, gine.hip, cgconv.hip, film.hip, rgcn.hip, gmm.hip, softmax_aggr.hip)
// share on top of attn_common.h's lane layout and hub-row plan: the slot walk of the H = 1 row kernels, the width check
// and the row / chunk launch ladder without the training form (none of them has dropout). Everything has internal
// linkage, as in attn_common.h: each translation unit launches its own copy and the library exports nothing from here.
#pragma once
#include "attn_common.h"

namespace rgbx {
namespace {

// The slot walk of one wave over the slots [start, end) of its row (or hub-row chunk): the column indices are read 64 at
// a time, one per lane, and handed round by shuffle; a lane group takes every NG-th slot, U of them in flight, each
// with NF row fragments of VEC channels that start as zeros.
//   load(f, nb, slot)     fills the fragments f[NF][VEC] of a slot from neighbour row nb = col[slot]; called only
//                         where ok (below), so a place past the row's end keeps its zeros
//   use(f, slot, ok)      consumes them, after all U loads of the batch were issued; called for every place
// ok = this lane has channels and the slot lies before the row's end. Where zeros in f do not make a place add
// nothing, `use` must skip on !ok; slot is meaningless there.
// lane, NG, g: lane_coords' fields as plain ints. Handing the LaneCoords itself in changed the float instructions of
// resgated's VEC = 4 forms (packed adds) and their occupancy; as ints all forms keep theirs.
template <int U, int NF, int VEC, class Load, class Use>
__device__ __forceinline__ void walk_slots(const int* __restrict__ col, int start, int end, int lane, int NG, int g,
                                           bool active, Load load, Use use) {
  for (int base = start; base < end; base += kWave) {
    const int n = min(kWave, end - base);
    const int mycol = lane < n ? col[base + lane] : 0;
    for (int k = 0; k < n; k += NG * U) {
      float f[U][NF][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        const int nb = __shfl(mycol, idx & 63);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
#pragma unroll
          for (int i = 0; i < VEC; ++i) f[u][j][i] = 0.f;
        }
        if (active && idx < n) load(f[u], nb, base + idx);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = k + u * NG + g;
        use(f[u], base + idx, active && idx < n);
      }
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------

// Row widths the H = 1 layout covers (head_width_supported), in the words of a layer without heads.
int check_width(int C, const char* name) {
  if (!head_width_supported(C))
    return fail(RGBX_E_SHAPE, "%s: %d channels (any C <= 64, even C <= 128, C %% 4 == 0 up to 256)", name, C);
  return RGBX_OK;
}

int check_sizes(int64_t N, int C, const char* name) {
  if (int rc = check_common(N, 1, C, name)) return rc;
  return check_width(C, name);
}

// LAUNCH_ROW over the rows and then, with a split plan, LAUNCH_CHUNK over the hub-row chunks, each on GRID(items)
// workgroups (RGBX_ATTN_ROWS with the two kernels spelled out). The argument list is written once: in it `n_items` is
// the pass's item count and `chunk_pass` tells the two passes apart. Expects `s`, `sd` and `split` in scope.
#define RGBX_EDGE_LAUNCH(GRID, n_rows, LAUNCH_ROW, LAUNCH_CHUNK, ...)       \
  do {                                                                      \
    {                                                                       \
      const int n_items = (int)(n_rows);                                    \
      constexpr bool chunk_pass = false;                                    \
      (void)chunk_pass;                                                     \
      LAUNCH_ROW<<<GRID(n_items), 256, 0, s>>>(__VA_ARGS__);                \
    }                                                                       \
    if (sd.threshold > 0) {                                                 \
      const int n_items = split->n_chunks;                                  \
      constexpr bool chunk_pass = true;                                     \
      (void)chunk_pass;                                                     \
      LAUNCH_CHUNK<<<GRID(n_items), 256, 0, s>>>(__VA_ARGS__);              \
    }                                                                       \
  } while (0)

// The common form: KERNEL<V, CHUNK> on one wave per item, V = `vec` as a constant. Expects `vec` in scope as well.
#define RGBX_EDGE_ROWS(KERNEL, n_rows, ...) \
  RGBX_VEC_SWITCH(vec, RGBX_EDGE_LAUNCH(row_grid, n_rows, (KERNEL<V, false>), (KERNEL<V, true>), __VA_ARGS__))

// KERNEL<V, CHUNK, X...>: the further template arguments go in parentheses, RGBX_EDGE_ROWS_X(k, (true, 2), N, ...).
#define RGBX_EDGE_UNPAREN(...) __VA_ARGS__
#define RGBX_EDGE_ROWS_X(KERNEL, X, n_rows, ...)                                               \
  RGBX_VEC_SWITCH(vec, RGBX_EDGE_LAUNCH(row_grid, n_rows, (KERNEL<V, false, RGBX_EDGE_UNPAREN X>), \
                                        (KERNEL<V, true, RGBX_EDGE_UNPAREN X>), __VA_ARGS__))

}  // namespace
}  // namespace rgbx
