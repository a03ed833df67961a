// paths_cache_probe / paths_cache_fill[_h16]: the device side of CachedOnDemandSlide (paths_amd/data_utils/slide.py) - an
// on-demand slide that keeps the rows its encoder has produced.  Per slide and level the cache is a cell index (int32 [X, Y]: the row of
// a cell in the store, or -1) and a row store [capacity, D]; the contracts are tests/cache_ref.py, byte for byte.
//
// probe: ONE workgroup per slide walks the request in chunks of PATHS_CACHE_PROBE_CHUNK cells, one cell per thread.  A cell inside its
// grid whose index entry is negative is a miss; misses are numbered in request order by a wave ballot (position inside the wave), a scan
// of the 16 wave totals in LDS (position of the wave inside the chunk) and a running carry (position of the chunk inside the request).
// fill: ONE wave per row of the batch's [B, n_max, D] buffer (the row-kernel shape of path_row.h / stage_rows.h: ROW_WAVES rows per
// workgroup, every load of a piece in flight before its first store).  A hit row moves store -> buffer, a miss row encoder -> buffer
// and, while the store has room, -> store, where one lane also names the new row in the index.  Integers and copies only: no atomics,
// no float arithmetic, no workspace; a rerun on the same inputs writes the same bytes.
//
// What keeps every access inside its buffer whatever the tables hold: n[b] is clamped to [0, n_max]; a hit is honoured only for
// src < count[b] <= capacity[b]; a miss only for j < miss_count[b] (the rows the encoder returned); a store write only for
// count[b] + j < capacity[b]; an index write only for a cell inside the grid.  Anything else reads as a zero row.
#include "common.h"
#include "path_row.h"

namespace {

constexpr int CP_THREADS = PATHS_CACHE_PROBE_CHUNK;      // one cell per thread and chunk
constexpr int CP_WAVES = CP_THREADS / 64;
static_assert(CP_THREADS % 64 == 0 && CP_THREADS <= 1024, "whole waves, one workgroup");
constexpr int CF_LOADS = 4;                              // pieces per lane in flight (stage_rows.h: a 4-KiB row is one round of 16-byte pieces)

__device__ __forceinline__ int clamp_n(int64_t n, int n_max) { return (int)max((int64_t)0, min(n, (int64_t)n_max)); }

__global__ void __launch_bounds__(CP_THREADS)
cache_probe_kernel(const int64_t* __restrict__ cells_ptrs, const int64_t* __restrict__ n, const int64_t* __restrict__ index_ptrs,
                   const int* __restrict__ gx, const int* __restrict__ gy, int n_max, int* __restrict__ src /*[B, n_max]*/,
                   int* __restrict__ miss_count /*[B]*/, int64_t* __restrict__ miss_cells /*[B, n_max, 2]*/, int* __restrict__ status /*[B]*/) {
  __shared__ int part[CP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = clamp_n(n[b], n_max);                                      // (workgroup-uniform: so are the loop and its barriers)
  const int64_t* cells = reinterpret_cast<const int64_t*>(static_cast<uintptr_t>(cells_ptrs[b]));
  const int* index = reinterpret_cast<const int*>(static_cast<uintptr_t>(index_ptrs[b]));
  const int64_t X = gx[b], Y = gy[b], row0 = (int64_t)b * n_max;
  int carry = 0, outside = 0;
  for (int c0 = 0; c0 < nb; c0 += CP_THREADS) {
    const int i = c0 + tid;
    int64_t cx = 0, cy = 0;
    int row = PATHS_CACHE_SRC_NONE;
    bool miss = false;
    if (i < nb) {
      cx = cells[2 * (int64_t)i]; cy = cells[2 * (int64_t)i + 1];
      if (cx >= 0 && cy >= 0 && cx < X && cy < Y) {
        row = index[cx * Y + cy];
        miss = row < 0;
      } else {
        outside = 1;
      }
    }
    const unsigned long long votes = __ballot(miss);
    if (lane == 0) part[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;                                              // misses of the waves in front of this one / of the chunk
#pragma unroll
    for (int w = 0; w < CP_WAVES; ++w) { const int t = part[w]; before += w < wave ? t : 0; total += t; }
    if (i < nb) {
      if (miss) {
        const int j = carry + before + __popcll(votes & ((1ull << lane) - 1ull));
        src[row0 + i] = -1 - j;
        miss_cells[2 * (row0 + j)] = cx; miss_cells[2 * (row0 + j) + 1] = cy;
      } else {
        src[row0 + i] = row;                                                // the store row, or PATHS_CACHE_SRC_NONE outside the grid
      }
    }
    carry += total;
    __syncthreads();                                                        // the totals are read before the next chunk writes them
  }
  outside = __syncthreads_or(outside);
  if (tid == 0) { miss_count[b] = carry; status[b] = outside ? 1 : 0; }
}

// one row of `pieces` V-sized pieces: from -> to (and -> also, unless null); from == null: zeros
template <class V>
__device__ __forceinline__ void copy_row(const unsigned char* from, unsigned char* to, unsigned char* also, int pieces, int lane) {
  typedef const V __attribute__((address_space(1))) * gsrc_t;
  const gsrc_t s = reinterpret_cast<gsrc_t>(reinterpret_cast<uintptr_t>(from));
  V* d = reinterpret_cast<V*>(to);
  V* e = reinterpret_cast<V*>(also);
  for (int p0 = 0; p0 < pieces; p0 += CF_LOADS * 64) {
    V v[CF_LOADS];
#pragma unroll
    for (int k = 0; k < CF_LOADS; ++k) {
      const int p = p0 + k * 64 + lane;
      v[k] = V{};
      if (from != nullptr && p < pieces) v[k] = s[p];
    }
#pragma unroll
    for (int k = 0; k < CF_LOADS; ++k) {
      const int p = p0 + k * 64 + lane;
      if (p < pieces) {
        d[p] = v[k];
        if (also != nullptr) e[p] = v[k];
      }
    }
  }
}

template <class V>
__global__ void __launch_bounds__(ROW_WAVES * 64)
cache_fill_kernel(const int64_t* __restrict__ cells_ptrs, const int64_t* __restrict__ n, const int* __restrict__ src,
                  const int* __restrict__ miss_count, const int64_t* __restrict__ enc_ptrs, const int64_t* __restrict__ store_ptrs,
                  const int64_t* __restrict__ count, const int64_t* __restrict__ capacity, const int64_t* __restrict__ index_ptrs,
                  const int* __restrict__ gx, const int* __restrict__ gy, int n_max, int64_t M /*B n_max*/, int row_bytes,
                  unsigned char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);   // (uniform over the wave)
  if (m >= M) return;
  const int64_t b = m / n_max, i = m - b * n_max;
  const int pieces = row_bytes / (int)sizeof(V);
  unsigned char* o = out + m * row_bytes;
  const unsigned char* from = nullptr;
  unsigned char* also = nullptr;
  if (i < clamp_n(n[b], n_max)) {
    const int s = src[m];
    const int64_t cnt = max((int64_t)0, count[b]);
    if (s >= 0) {
      if (s < min(cnt, capacity[b])) from = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(store_ptrs[b])) + (int64_t)s * row_bytes;
    } else if (s != PATHS_CACHE_SRC_NONE && -1 - s < miss_count[b]) {
      const int64_t j = -1 - s;
      from = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(enc_ptrs[b])) + j * row_bytes;
      if (cnt + j < capacity[b]) {
        also = reinterpret_cast<unsigned char*>(static_cast<uintptr_t>(store_ptrs[b])) + (cnt + j) * row_bytes;
        if (lane == 0) {
          const int64_t* cells = reinterpret_cast<const int64_t*>(static_cast<uintptr_t>(cells_ptrs[b]));
          const int64_t cx = cells[2 * i], cy = cells[2 * i + 1], X = gx[b], Y = gy[b];
          if (cx >= 0 && cy >= 0 && cx < X && cy < Y)
            reinterpret_cast<int*>(static_cast<uintptr_t>(index_ptrs[b]))[cx * Y + cy] = (int)(cnt + j);
        }
      }
    }
  }
  copy_row<V>(from, o, also, pieces, lane);
}

int launch_cache_fill(const char* what, int esize, const int64_t* cells_ptrs, const int64_t* n, const int* src, const int* miss_count,
                      const int64_t* enc_ptrs, const int64_t* store_ptrs, const int64_t* count, const int64_t* capacity,
                      const int64_t* index_ptrs, const int* gx, const int* gy, int B, int n_max, int D, void* out, hipStream_t stream) {
  PATHS_REQUIRE(B > 0, "%s: B (%d) must be > 0", what, B);
  PATHS_REQUIRE(n_max > 0, "%s: n_max (%d) must be > 0", what, n_max);
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "%s: D (%d) must be a positive multiple of 4", what, D);
  PATHS_REQUIRE(cells_ptrs && n && src && miss_count && enc_ptrs && store_ptrs && count && capacity && index_ptrs && gx && gy && out,
                "%s: null pointer (every argument is required)", what);
  PATHS_REQUIRE((uintptr_t)out % 16 == 0, "%s: out must be 16-byte aligned", what);
  const int64_t M = (int64_t)B * n_max, row_bytes = (int64_t)D * esize;
  PATHS_REQUIRE(row_bytes <= (1 << 30), "%s: a row of %lld bytes is too long", what, (long long)row_bytes);
  PATHS_REQUIRE((M + ROW_WAVES - 1) / ROW_WAVES <= 0x7fffffffLL, "%s: too many rows (%lld)", what, (long long)M);
  const dim3 grid((unsigned)((M + ROW_WAVES - 1) / ROW_WAVES)), block(ROW_WAVES * 64);
  unsigned char* o = reinterpret_cast<unsigned char*>(out);
  if (row_bytes % 16 == 0)
    hipLaunchKernelGGL(cache_fill_kernel<u32x4>, grid, block, 0, stream, cells_ptrs, n, src, miss_count, enc_ptrs, store_ptrs, count, capacity,
                       index_ptrs, gx, gy, n_max, M, (int)row_bytes, o);
  else      // fp16 rows of D % 8 == 4: whole 8-byte pieces
    hipLaunchKernelGGL(cache_fill_kernel<u32x2>, grid, block, 0, stream, cells_ptrs, n, src, miss_count, enc_ptrs, store_ptrs, count, capacity,
                       index_ptrs, gx, gy, n_max, M, (int)row_bytes, o);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

}  // namespace

extern "C" {

int paths_cache_probe(const int64_t* cells_ptrs, const int64_t* n, const int64_t* index_ptrs, const int* gx, const int* gy, int B, int n_max,
                      int D, int* src, int* miss_count, int64_t* miss_cells, int* status, hipStream_t stream) {
  PATHS_REQUIRE(B > 0, "cache_probe: B (%d) must be > 0", B);
  PATHS_REQUIRE(n_max > 0, "cache_probe: n_max (%d) must be > 0", n_max);
  PATHS_REQUIRE(D > 0 && D % 4 == 0, "cache_probe: D (%d) must be a positive multiple of 4", D);
  PATHS_REQUIRE(cells_ptrs && n && index_ptrs && gx && gy && src && miss_count && miss_cells && status,
                "cache_probe: null pointer (every argument is required)");
  hipLaunchKernelGGL(cache_probe_kernel, dim3(B), dim3(CP_THREADS), 0, stream, cells_ptrs, n, index_ptrs, gx, gy, n_max, src, miss_count,
                     miss_cells, status);
  PATHS_LAUNCH_CHECK("cache_probe");
  return PATHS_OK;
}

int paths_cache_fill(const int64_t* cells_ptrs, const int64_t* n, const int* src, const int* miss_count, const int64_t* enc_ptrs,
                     const int64_t* store_ptrs, const int64_t* count, const int64_t* capacity, const int64_t* index_ptrs, const int* gx,
                     const int* gy, int B, int n_max, int D, float* out, hipStream_t stream) {
  return launch_cache_fill("cache_fill", 4, cells_ptrs, n, src, miss_count, enc_ptrs, store_ptrs, count, capacity, index_ptrs, gx, gy, B, n_max,
                           D, out, stream);
}

int paths_cache_fill_h16(const int64_t* cells_ptrs, const int64_t* n, const int* src, const int* miss_count, const int64_t* enc_ptrs,
                         const int64_t* store_ptrs, const int64_t* count, const int64_t* capacity, const int64_t* index_ptrs, const int* gx,
                         const int* gy, int B, int n_max, int D, void* out, hipStream_t stream) {
  return launch_cache_fill("cache_fill_h16", 2, cells_ptrs, n, src, miss_count, enc_ptrs, store_ptrs, count, capacity, index_ptrs, gx, gy, B,
                           n_max, D, out, stream);
}

}  // extern "C"
