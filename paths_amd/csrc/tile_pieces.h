// What the tile kernels share (tiles.hip, tile_resize.hip): 16 pixels as three 16-byte loads, the rule a table entry must keep to be
// followed, and the 16-element store of the encoder input.
#pragma once
#include "common.h"

namespace {

typedef const u32x4 __attribute__((address_space(1))) * gu4_t;
typedef const unsigned char __attribute__((address_space(1))) * gu8_t;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int grey(int r, int g, int b) { return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14; }

// 16 pixels = 48 bytes = three 16-byte loads; byte i of the piece
struct Piece {
  uint32_t w[12];
  __device__ __forceinline__ void load(const unsigned char* p) {
    const gu4_t s = reinterpret_cast<gu4_t>(reinterpret_cast<uintptr_t>(p));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const u32x4 v = s[k];
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int k = 0; k < 12; ++k) w[k] = 0;
  }
  __device__ __forceinline__ int byte(int i) const { return (int)((w[i >> 2] >> ((i & 3) * 8)) & 0xffu); }     // (i: a constant after unrolling)
  __device__ __forceinline__ int grey_of(int px) const { return grey(byte(3 * px), byte(3 * px + 1), byte(3 * px + 2)); }
};

__device__ __forceinline__ int grey_at(const unsigned char* p) {
  const gu8_t s = reinterpret_cast<gu8_t>(reinterpret_cast<uintptr_t>(p));
  return grey(s[0], s[1], s[2]);
}

__device__ __forceinline__ bool entry_ok(int64_t addr, int64_t stride, int64_t row_bytes) {
  return addr != 0 && ((addr | stride) & 15) == 0 && stride >= row_bytes;
}

// 16 consecutive elements of one output row as 16-byte stores (E: the bits of an fp16 / bf16 or an fp32 element)
template <class E>
__device__ __forceinline__ void store16(E* p, const E (&v)[16]) {
  typedef u32x4 __attribute__((address_space(1))) * gdst;
  const gdst d = reinterpret_cast<gdst>(reinterpret_cast<uintptr_t>(p));
  if constexpr (sizeof(E) == 2) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      d[q] = u32x4{(uint32_t)v[8 * q] | (uint32_t)v[8 * q + 1] << 16, (uint32_t)v[8 * q + 2] | (uint32_t)v[8 * q + 3] << 16,
                   (uint32_t)v[8 * q + 4] | (uint32_t)v[8 * q + 5] << 16, (uint32_t)v[8 * q + 6] | (uint32_t)v[8 * q + 7] << 16};
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = u32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  }
}

inline bool tile_shape_ok(int P) { return P >= 16 && P <= PATHS_TILE_MAX_P && P % 16 == 0; }

}  // namespace
