// Tissue-only slide storage (paths_amd/data_utils/slide.py: DeviceSlide.pack): the device side of packing a dense [X, Y, D] grid
// into its kept rows [n, D] behind an int32 cell index [X, Y] (row number of a cell, or -1).
//
// A row is KEPT iff any of its bits is set: only rows that are all +0.0 are dropped (a -0.0 element is a set bit; a row whose elements
// cancel to a zero sum is kept - it is background to the child filter, but level 0 and the zero-children fallback still read it).
// Rows are ranked in row-major cell order (exclusive prefix sum of the flags), so the packed form is reproducible and keeps the
// dense grid's locality.  Three passes, all integer / copy work on bytes - one set of kernels serves fp32 and fp16 rows:
//   paths_pack_flags  one wave per cell, 16- (or 8-) byte loads, flag = OR of the row's words != 0
//   paths_pack_index  block partials (1024 cells per block) + every block summing the partials before it: fixed order, no atomics
//   paths_pack_rows   one wave per cell, kept rows copied 16 (or 8) bytes per lane to rows[index[cell]]
#include "common.h"

namespace {

constexpr int PACK_WAVES = 4;          // cells per workgroup of the row kernels
constexpr int SCAN_NT = 256;           // threads of a scan block
constexpr int SCAN_PER = 4;            // cells per thread
constexpr int SCAN_CELLS = SCAN_NT * SCAN_PER;

__device__ __forceinline__ unsigned any_bits(uint4 v) { return v.x | v.y | v.z | v.w; }
__device__ __forceinline__ unsigned any_bits(uint2 v) { return v.x | v.y; }

template <class V>
__global__ void __launch_bounds__(PACK_WAVES * 64)
pack_flags_kernel(const unsigned char* __restrict__ grid, int64_t cells, int row_bytes, uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int64_t cell = (int64_t)blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const V* row = reinterpret_cast<const V*>(grid + cell * row_bytes);
  unsigned m = 0;
  for (int i = lane; i < row_bytes / (int)sizeof(V); i += 64) m |= any_bits(row[i]);
  const bool any = __ballot(m != 0) != 0;
  if (lane == 0) flags[cell] = any ? 1 : 0;
}

// kept cells of the block's SCAN_CELLS cells; every thread returns the block total, `before` = kept cells in front of the thread's first
__device__ __forceinline__ int block_scan(const uint8_t* __restrict__ flags, int64_t cells, int64_t first, int f[SCAN_PER], int& before) {
  __shared__ int wave_sum[SCAN_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mine = 0;
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) {
    const int64_t c = first + e;
    f[e] = (c < cells && flags[c]) ? 1 : 0;
    mine += f[e];
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int total = 0, front = 0;
#pragma unroll
  for (int w = 0; w < SCAN_NT / 64; ++w) {
    if (w < wave) front += wave_sum[w];
    total += wave_sum[w];
  }
  before = front + incl - mine;
  return total;
}

__global__ void __launch_bounds__(SCAN_NT)
pack_partials_kernel(const uint8_t* __restrict__ flags, int64_t cells, int* __restrict__ partials) {
  int f[SCAN_PER], before;
  const int total = block_scan(flags, cells, ((int64_t)blockIdx.x * SCAN_NT + threadIdx.x) * SCAN_PER, f, before);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_NT)
pack_index_kernel(const uint8_t* __restrict__ flags, int64_t cells, const int* __restrict__ partials, int* __restrict__ index,
                  int* __restrict__ count) {
  __shared__ int part[SCAN_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // kept cells of all blocks in front of this one (integer sum: the order cannot change it)
  int s = 0;
  for (int i = threadIdx.x; i < (int)blockIdx.x; i += SCAN_NT) s += partials[i];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
  if (lane == 0) part[wave] = s;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < SCAN_NT / 64; ++w) base += part[w];
  const int64_t first = ((int64_t)blockIdx.x * SCAN_NT + threadIdx.x) * SCAN_PER;
  int f[SCAN_PER], before;
  const int total = block_scan(flags, cells, first, f, before);
  int rank = base + before;
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) {
    if (first + e < cells) index[first + e] = f[e] ? rank : -1;
    rank += f[e];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = base + total;
}

template <class V>
__global__ void __launch_bounds__(PACK_WAVES * 64)
pack_rows_kernel(const unsigned char* __restrict__ grid, int64_t cells, int row_bytes, const int* __restrict__ index, int64_t n_rows,
                 unsigned char* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int64_t cell = (int64_t)blockIdx.x * PACK_WAVES + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const int64_t r = index[cell];
  if (r < 0 || r >= n_rows) return;            // (an index that does not belong to `rows` writes nothing)
  const V* src = reinterpret_cast<const V*>(grid + cell * row_bytes);
  V* dst = reinterpret_cast<V*>(rows + r * row_bytes);
  for (int i = lane; i < row_bytes / (int)sizeof(V); i += 64) dst[i] = src[i];
}

int pack_flags(const char* what, const void* grid, int64_t cells, int row_bytes, uint8_t* flags, hipStream_t stream) {
  PATHS_REQUIRE(grid != nullptr && flags != nullptr, "%s: null pointer", what);
  PATHS_REQUIRE(cells > 0 && cells < ((int64_t)1 << 31), "%s: cells (%lld) must be in [1, 2^31)", what, (long long)cells);
  PATHS_REQUIRE(row_bytes > 0 && row_bytes % 8 == 0 && (uintptr_t)grid % 8 == 0, "%s: rows are whole 8-byte words", what);
  const dim3 g((unsigned)((cells + PACK_WAVES - 1) / PACK_WAVES)), t(PACK_WAVES * 64);
  const unsigned char* src = reinterpret_cast<const unsigned char*>(grid);
  if (row_bytes % 16 == 0 && (uintptr_t)grid % 16 == 0) hipLaunchKernelGGL(pack_flags_kernel<uint4>, g, t, 0, stream, src, cells, row_bytes, flags);
  else hipLaunchKernelGGL(pack_flags_kernel<uint2>, g, t, 0, stream, src, cells, row_bytes, flags);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

int pack_rows(const char* what, const void* grid, int64_t cells, int row_bytes, const int* index, int64_t n_rows, void* rows, hipStream_t stream) {
  PATHS_REQUIRE(grid != nullptr && index != nullptr && rows != nullptr, "%s: null pointer", what);
  PATHS_REQUIRE(cells > 0 && cells < ((int64_t)1 << 31) && n_rows > 0 && n_rows <= cells, "%s: cells (%lld) in [1, 2^31), rows (%lld) in [1, cells]", what,
                (long long)cells, (long long)n_rows);
  PATHS_REQUIRE(row_bytes > 0 && row_bytes % 8 == 0 && ((uintptr_t)grid | (uintptr_t)rows) % 8 == 0, "%s: rows are whole 8-byte words", what);
  const dim3 g((unsigned)((cells + PACK_WAVES - 1) / PACK_WAVES)), t(PACK_WAVES * 64);
  const unsigned char* src = reinterpret_cast<const unsigned char*>(grid);
  unsigned char* dst = reinterpret_cast<unsigned char*>(rows);
  if (row_bytes % 16 == 0 && ((uintptr_t)grid | (uintptr_t)rows) % 16 == 0)
    hipLaunchKernelGGL(pack_rows_kernel<uint4>, g, t, 0, stream, src, cells, row_bytes, index, n_rows, dst);
  else
    hipLaunchKernelGGL(pack_rows_kernel<uint2>, g, t, 0, stream, src, cells, row_bytes, index, n_rows, dst);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

}  // namespace

extern "C" {

int paths_pack_flags(const float* grid, int64_t cells, int D, uint8_t* flags, hipStream_t stream) {
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "pack_flags: D (%d) must be a positive multiple of 4", D);
  return pack_flags("pack_flags", grid, cells, D * 4, flags, stream);
}

int paths_pack_flags_h16(const void* grid, int64_t cells, int D, uint8_t* flags, hipStream_t stream) {
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "pack_flags_h16: D (%d) must be a positive multiple of 4", D);
  return pack_flags("pack_flags_h16", grid, cells, D * 2, flags, stream);
}

int64_t paths_pack_index_partials(int64_t cells) { return cells > 0 ? (cells + SCAN_CELLS - 1) / SCAN_CELLS : 0; }

int paths_pack_index(const uint8_t* flags, int64_t cells, int* index, int* count, int* partials, hipStream_t stream) {
  PATHS_REQUIRE(flags != nullptr && index != nullptr && count != nullptr && partials != nullptr, "pack_index: null pointer");
  PATHS_REQUIRE(cells > 0 && cells < ((int64_t)1 << 31), "pack_index: cells (%lld) must be in [1, 2^31)", (long long)cells);
  const unsigned blocks = (unsigned)paths_pack_index_partials(cells);
  hipLaunchKernelGGL(pack_partials_kernel, dim3(blocks), dim3(SCAN_NT), 0, stream, flags, cells, partials);
  PATHS_LAUNCH_CHECK("pack_index (partials)");
  hipLaunchKernelGGL(pack_index_kernel, dim3(blocks), dim3(SCAN_NT), 0, stream, flags, cells, partials, index, count);
  PATHS_LAUNCH_CHECK("pack_index");
  return PATHS_OK;
}

int paths_pack_rows(const float* grid, int64_t cells, int D, const int* index, int64_t n_rows, float* rows, hipStream_t stream) {
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "pack_rows: D (%d) must be a positive multiple of 4", D);
  return pack_rows("pack_rows", grid, cells, D * 4, index, n_rows, rows, stream);
}

int paths_pack_rows_h16(const void* grid, int64_t cells, int D, const int* index, int64_t n_rows, void* rows, hipStream_t stream) {
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "pack_rows_h16: D (%d) must be a positive multiple of 4", D);
  return pack_rows("pack_rows_h16", grid, cells, D * 2, index, n_rows, rows, stream);
}

}  // extern "C"
