// The skeleton of the per-row kernels of the patch attributions (path_rows.hip): ONE wave per recorded row (b, r) of
// [B][rows_per_slide], ROW_WAVES rows per workgroup, 16-byte loads and stores, and on the host the argument checks and the grid size
// their entry points share.  Registers only: no LDS, no atomics, no workspace.
#pragma once
#include <initializer_list>
#include "common.h"

constexpr int ROW_WAVES = 4;        // rows per workgroup

// The row this wave owns: row = b * rows_per_slide + r of M = B * rows_per_slide.  false: beyond the launch - the caller returns (whole
// waves leave: row is uniform over a wave; nothing else is set).  padded: at or beyond num_ims[b] - not to be read, owed exact zeros.
__device__ __forceinline__ bool row_of_wave(const int64_t* __restrict__ num_ims, int rows_per_slide, int64_t M, int64_t& row, int64_t& b,
                                            int64_t& r, bool& padded) {
  row = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (row >= M) return false;
  b = row / rows_per_slide;
  r = row - b * rows_per_slide;
  padded = r >= num_ims[b];
  return true;
}

// Exact zeros in this row of all C members of out [C][M][D].
__device__ __forceinline__ void zero_row(float* out, int C, int64_t M, int64_t row, int D, int lane) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    float* o = out + ((int64_t)c * M + row) * D;
    for (int i = lane * 4; i < D; i += 256) stg_f32x4(o + i, zero);
  }
}

// Adds this lane's share of sum_d g[d] (v[d] - base[d]) to dot and of sum_d g[d]^2 to sq (base may be nullptr: zeros), columns in
// ascending order; the 64 shares meet in wave_sum (lanes.h).
__device__ __forceinline__ void row_dot_sq(const float* g, const float* v, const float* base, int D, int lane, float& dot, float& sq) {
#pragma unroll 4
  for (int i = lane * 4; i < D; i += 256) {
    const f32x4 a = ldg_f32x4(g + i);
    f32x4 t = ldg_f32x4(v + i);
    if (base != nullptr) t -= ldg_f32x4(base + i);
    dot += (a[0] * t[0] + a[1] * t[1]) + (a[2] * t[2] + a[3] * t[3]);
    sq += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
  }
}

// The checks every per-row entry point makes of its shape, its row strides and the pointers it reads or writes 16 bytes at a time
// (`aligned`: their names, for the message).  `name`: the entry point's own, which its messages start with.  PATHS_OK or the error.
inline int path_rows_check(const char* name, int D, int B, int C, int rows_per_slide, std::initializer_list<int64_t> strides,
                           std::initializer_list<const void*> ptrs, const char* aligned) {
  PATHS_REQUIRE(D > 0 && D % 128 == 0, "%s: D (%d) must be a positive multiple of 128", name, D);
  PATHS_REQUIRE(B > 0 && C > 0 && rows_per_slide > 0, "%s: B (%d), C (%d) and rows_per_slide (%d) must be positive", name, B, C,
                rows_per_slide);
  for (const int64_t ld : strides)
    PATHS_REQUIRE(ld >= D && ld % 4 == 0, "%s: row strides must be multiples of 4 and at least D (%d), got %lld", name, D, (long long)ld);
  for (const void* p : ptrs) PATHS_REQUIRE((uintptr_t)p % 16 == 0, "%s: %s must be 16-byte aligned", name, aligned);
  PATHS_REQUIRE(((int64_t)B * rows_per_slide + ROW_WAVES - 1) / ROW_WAVES <= 0x7fffffffLL, "%s: too many rows (%lld)", name,
                (long long)B * rows_per_slide);
  return PATHS_OK;
}

inline dim3 path_rows_grid(int B, int rows_per_slide) {
  return dim3((unsigned)(((int64_t)B * rows_per_slide + ROW_WAVES - 1) / ROW_WAVES));
}
