// Row staging over the host link (csrc/stage_rows.hip; tools/stage_rows_bench.hip times the other shapes of this template).
//
// A host-resident slide keeps its feature grids in pinned, device-mapped host memory.  paths_level0_batch* / paths_gather_rows*
// write the ADDRESS of every selected feature row into a table; this kernel pulls exactly those rows over the link into a compact
// HBM buffer and points the table at the copies, so every GEMM behind it reads HBM.
//
// A read over PCIe has a round trip of a microsecond or more: throughput is bytes in flight, not ALU occupancy.  One wave copies one
// row with 16-byte loads per lane (1 KiB per wave instruction), and ALL loads of a piece of up to 4 KiB are issued before the first
// store - a 4-KiB fp32 row is four loads per lane in flight, a 2-KiB fp16 row two.  No LDS.  Every source byte is read once; the
// table entry is read once, before the copy, and rewritten last.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t paths_u32x4 __attribute__((ext_vector_type(4)));

constexpr int STAGE_LOADS = 4;      // 16-byte loads per lane in flight: 4 x 64 lanes x 16 B = one 4-KiB piece

// WAVES rows per workgroup (one wave each); NT: non-temporal loads (a measurement variant).
// Entries equal to zero_row (padding, dropped rows) are never dereferenced and keep their value.
template <int WAVES, bool NT>
__global__ void __launch_bounds__(WAVES * 64)
stage_rows_kernel(int64_t* __restrict__ row_ptrs, int64_t rows, int row_bytes, unsigned char* __restrict__ stage, int64_t zero_row) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (m >= rows) return;
  const int64_t src = row_ptrs[m];
  if (src == zero_row) return;
  typedef const paths_u32x4 __attribute__((address_space(1))) * gsrc_t;
  const gsrc_t s = reinterpret_cast<gsrc_t>(static_cast<uintptr_t>(src));
  paths_u32x4* d = reinterpret_cast<paths_u32x4*>(stage + m * row_bytes);
  const int n16 = row_bytes >> 4;
  for (int c0 = 0; c0 < n16; c0 += STAGE_LOADS * 64) {
    paths_u32x4 v[STAGE_LOADS];
#pragma unroll
    for (int k = 0; k < STAGE_LOADS; ++k) {
      const int i = c0 + k * 64 + lane;
      if (i < n16) {
        if constexpr (NT) v[k] = __builtin_nontemporal_load(s + i);
        else v[k] = s[i];
      }
    }
#pragma unroll
    for (int k = 0; k < STAGE_LOADS; ++k) {
      const int i = c0 + k * 64 + lane;
      if (i < n16) d[i] = v[k];
    }
  }
  if (lane == 0) row_ptrs[m] = (int64_t)reinterpret_cast<uintptr_t>(d);
}
