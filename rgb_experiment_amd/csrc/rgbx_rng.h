// Counter-based random draws shared by the kernels that recompute their random decisions in the backward pass
// (the attention families, through attn_common.h): a draw is a hash of a 64-bit seed that lives on the device, a stream
// constant of the caller and two 32-bit counters; no state, no per-edge tensor.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rgbx {

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// 32 bits that depend on (seed, stream, a, b) and on nothing else.
__device__ __forceinline__ uint32_t draw32(uint32_t s0, uint32_t s1, uint32_t stream, uint32_t a, uint32_t b) {
  return mix32(mix32(mix32(a ^ s0) + b * 0x9E3779B9u + stream) ^ s1);
}

__device__ __forceinline__ float unit24(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

}  // namespace rgbx
