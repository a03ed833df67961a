// paths_rank_joint: the ranking behind the deletion and insertion curves taken along the recursion's frozen path
// (paths_amd/saliency.py:perturbation_curves).  The rows themselves are built by paths_path_mask_points (path_rows.hip).
//
// rank_joint: one rank per visited patch of a slide, jointly over the chosen levels - rank_i = #{valid j of the slide : key_j <
// key_i} on the 64-bit key of the top-K (rank_key.h; -0 read as +0, the score word inverted for `ascending`), so keys are unique and
// the ranks of a slide's valid elements are a permutation of 0 .. count - 1.  The joint length is not bounded by LDS (five levels
// at K = 2048: up to 34,816 keys, 278 KB): every workgroup owns RJ_THREADS elements, one per thread, and streams ALL keys of its
// slide through one RJ_TILE-key LDS tile (16 KiB: up to 8 workgroups per CU), every thread counting the keys below its own (key
// pairs read by 16-byte LDS broadcast).  A tile without a valid element is not compared.  Integer counts: no atomics, no workspace,
// the result does not depend on the launch.  Padded rows and rows of levels that are not chosen are never read as scores.
// Per slide: n_tot^2 64-bit compares; every workgroup builds all n_tot keys once (the valid scores are read n_tot / RJ_THREADS + 1
// times, from cache) and each of its four waves reads all of them back from LDS.  4 n_tot bytes in, 4 n_tot + 4 out, algorithmically.
//
// The removal curves on the free path (paths_amd/saliency.py:removal_curves) perturb a slide through its tissue masks, not
// its rows: a member of a curve is the slide's grids with other uint8 [X, Y] masks (DeviceSlide.with_masks).
//
// removal_masks: member (c, b)'s mask of one level = the source mask of slide b with the cell of every valid recorded row of rank <
// thr[c, b] cleared (mode 1: set).  A workgroup owns RM_CELLS cells of one member: it marks the chosen rows' cells that fall into
// its range in an LDS flag tile, then writes source-merged-with-flags in one pass of 16-byte copies (a source that is not 16-byte
// aligned and the ragged tail go byte by byte) - every output byte is written once, by one thread: no atomics, no ordering between
// workgroups.  left[c, b], the cells still set, is an integer count by the member's first workgroup alone: the source's non-zero
// bytes minus the chosen rows whose source byte is set (plus those whose byte is clear, mode 1) - two valid rows never share a
// cell - reduced over the workgroup in a fixed order.  cells in + C cells out per slide; N ranks and the chosen locations re-read
// per workgroup from cache.
//
// visited_overlap: per virtual slide v = c B + b the number of the member's valid rows whose cell is set in slide b's bitmap of
// recorded cells (a removal_masks mask in mode 1 over a NULL source).  One workgroup per v, a wave per 64-row chunk, integer wave
// sums, the four waves' partials added in wave order.
//
// level0_mask_rows: the reference loads EVERY level-0 cell, background included (a background cell is an all-zero row there);
// for a masked view the rows of cleared level-0 cells are therefore made the zero row (the copy zeroed / the row address pointed at
// the zero row) behind paths_level0_batch.
#include "common.h"
#include "lanes.h"
#include "rank_key.h"

constexpr int RJ_THREADS = 256;      // elements per workgroup
constexpr int RJ_TILE = 2048;        // keys per LDS tile
constexpr int RJ_MAX_LEVELS = 16;
static_assert(RJ_TILE % 8 == 0 && RJ_TILE % RJ_THREADS == 0, "the compare loop takes four key pairs per step");

__device__ __forceinline__ unsigned long long joint_key(float score, int idx, int ascending) {
  uint32_t u = __float_as_uint(score);
  if (u == 0x80000000u) u = 0u;                                           // -0 orders as +0
  const unsigned long long k = topk_key(__uint_as_float(u), idx);
  return ascending ? k ^ 0xFFFFFFFF00000000ull : k;                       // the score order turns, the index order does not
}

__global__ void __launch_bounds__(RJ_THREADS)
rank_joint_kernel(const float* __restrict__ scores, const int* __restrict__ seg_end, const int* __restrict__ level_on,
                  const int64_t* __restrict__ num_ims, int L, int B, int n_tot, int ascending, int* __restrict__ rank,
                  int* __restrict__ count) {
  __shared__ __attribute__((aligned(16))) unsigned long long keys[RJ_TILE];
  __shared__ int s_lo[RJ_MAX_LEVELS], s_hi[RJ_MAX_LEVELS];               // joint indices [s_lo, s_hi) of level l are valid
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    int start = 0, total = 0;
    for (int l = 0; l < L; ++l) {                                         // (the table is device data: clamped, never trusted)
      const int end = max(start, min(seg_end[l], n_tot));
      const int64_t n = num_ims[(int64_t)l * B + b];
      const int nv = level_on[l] != 0 ? (int)max((int64_t)0, min(n, (int64_t)(end - start))) : 0;
      s_lo[l] = start;
      s_hi[l] = start + nv;
      total += nv;
      start = end;
    }
    if (blockIdx.x == 0) count[b] = total;
  }
  __syncthreads();
  auto valid = [&](int j) {
    bool v = false;
    for (int l = 0; l < L; ++l) v = v || (j >= s_lo[l] && j < s_hi[l]);
    return v;
  };
  const float* s = scores + (int64_t)b * n_tot;
  int* out = rank + (int64_t)b * n_tot;
  const int i = blockIdx.x * RJ_THREADS + tid;                            // this thread's element
  const bool mine_ok = i < n_tot && valid(i);
  if (!__syncthreads_or(mine_ok)) {                                       // nothing valid here (workgroup-uniform)
    if (i < n_tot) out[i] = -1;
    return;
  }
  const unsigned long long mine = mine_ok ? joint_key(s[i], i, ascending) : 0ull;
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2* kp = reinterpret_cast<const u64x2*>(keys);
  int cnt = 0;
  for (int t0 = 0; t0 < n_tot; t0 += RJ_TILE) {
    const int len = min(RJ_TILE, n_tot - t0), np = (len + 7) & ~7;        // keys beyond len: all ones (never below a real key)
    bool any = false;
    for (int j = tid; j < np; j += RJ_THREADS) {
      const int g = t0 + j;
      const bool ok = j < len && valid(g);
      keys[j] = ok ? joint_key(s[g], g, ascending) : ~0ull;
      any = any || ok;
    }
    if (__syncthreads_or(any)) {                                          // (also the barrier between the tile's writes and reads)
      const int pairs = np >> 1;
      for (int q = 0; q < pairs; q += 4) {
        const u64x2 a = kp[q], c = kp[q + 1], d = kp[q + 2], e = kp[q + 3];
        cnt += (a[0] < mine) + (a[1] < mine) + (c[0] < mine) + (c[1] < mine) + (d[0] < mine) + (d[1] < mine) + (e[0] < mine) + (e[1] < mine);
      }
    }
    __syncthreads();                                                      // the tile is consumed before the next one is written
  }
  if (i < n_tot) out[i] = mine_ok ? cnt : -1;
}

// ---- removal masks and path overlap
constexpr int RM_THREADS = 256;
constexpr int RM_CELLS = RM_THREADS * 16;        // cells (bytes) per workgroup: one 16-byte vector per thread

// the cell index of a recorded location, -1 when it lies outside the grid (device data: never trusted)
__device__ __forceinline__ int64_t cell_of(const int64_t* __restrict__ loc, int patch_size, int X, int Y) {
  const int64_t cx = loc[0] / patch_size, cy = loc[1] / patch_size;
  return (loc[0] < 0 || loc[1] < 0 || cx >= X || cy >= Y) ? -1 : cx * Y + cy;
}

// sum over the workgroup's RM_THREADS threads, valid in thread 0: wave sums, then the waves' partials in wave order
__device__ __forceinline__ int block_sum_i(int v, int* s_part) {
  v = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < RM_THREADS / 64; ++w) t += s_part[w];
  return t;
}

__global__ void __launch_bounds__(RM_THREADS)
removal_masks_kernel(const int64_t* __restrict__ src_ptrs, const int* __restrict__ gx, const int* __restrict__ gy,
                     const int64_t* __restrict__ locs, int patch_size, const int64_t* __restrict__ num_ims, const int* __restrict__ rank,
                     int64_t ldr, const int* __restrict__ thr, int N, int B, int set, uint8_t* __restrict__ masks, int64_t ldm,
                     int* __restrict__ left) {
  __shared__ __attribute__((aligned(16))) uint8_t flag[RM_CELLS];
  __shared__ int s_part[RM_THREADS / 64];
  const int b = blockIdx.y, c = blockIdx.z, tid = threadIdx.x;
  const int X = gx[b], Y = gy[b];
  const int64_t cells = min((int64_t)X * Y, ldm);
  const int64_t c0 = (int64_t)blockIdx.x * RM_CELLS;
  if (c0 >= cells && blockIdx.x != 0) return;                              // (workgroup-uniform)
  const uint8_t* src = src_ptrs != nullptr ? reinterpret_cast<const uint8_t*>(src_ptrs[b]) : nullptr;
  uint8_t* out = masks + ((int64_t)c * B + b) * ldm;
  const int n = (int)max((int64_t)0, min(num_ims[b], (int64_t)N));
  const int t = thr != nullptr ? thr[(int64_t)c * B + b] : 0x7fffffff;
  reinterpret_cast<u32x4*>(flag)[tid] = u32x4{0u, 0u, 0u, 0u};
  __syncthreads();
  int hit = 0;                                                             // chosen rows on a set source cell (whole slide)
  int chosen = 0;
  for (int r = tid; r < n; r += RM_THREADS) {
    const int rk = rank != nullptr ? rank[b * ldr + r] : 0;
    if (rk < 0 || rk >= t) continue;
    const int64_t cell = cell_of(locs + ((int64_t)b * N + r) * 2, patch_size, X, Y);
    if (cell < 0 || cell >= cells) continue;
    if (cell >= c0 && cell < c0 + RM_CELLS) flag[cell - c0] = 0xFF;
    if (blockIdx.x == 0) {
      ++chosen;
      hit += (src != nullptr && src[cell] != 0) ? 1 : 0;
    }
  }
  __syncthreads();
  const int64_t v0 = c0 + (int64_t)tid * 16;
  const bool vec = src == nullptr || (reinterpret_cast<uintptr_t>(src) & 15) == 0;     // (uniform over the member)
  if (v0 + 16 <= cells && vec) {
    const u32x4 f = reinterpret_cast<const u32x4*>(flag)[tid];
    const u32x4 s = src != nullptr ? *reinterpret_cast<const u32x4*>(src + v0) : u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(out + v0) = set ? ((s & ~f) | (f & 0x01010101u)) : (s & ~f);
  } else {
    for (int64_t i = v0; i < min(v0 + 16, cells); ++i) {
      const uint8_t f = flag[i - c0], s = src != nullptr ? src[i] : (uint8_t)0;
      out[i] = f ? (set ? (uint8_t)1 : (uint8_t)0) : s;
    }
  }
  if (blockIdx.x != 0) return;
  int cnt = 0;                                                             // the source's non-zero bytes
  if (src != nullptr) {
    if (vec) {
      const int64_t nv = cells >> 4;
      for (int64_t q = tid; q < nv; q += RM_THREADS) {
        const u32x4 s = reinterpret_cast<const u32x4*>(src)[q];
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int k = 0; k < 4; ++k) cnt += ((s[w] >> (8 * k)) & 0xFFu) != 0u;
      }
      for (int64_t i = (nv << 4) + tid; i < cells; i += RM_THREADS) cnt += src[i] != 0;
    } else {
      for (int64_t i = tid; i < cells; i += RM_THREADS) cnt += src[i] != 0;
    }
  }
  cnt += set ? chosen - hit : -hit;
  const int total = block_sum_i(cnt, s_part);
  if (tid == 0) left[(int64_t)c * B + b] = total;
}

__global__ void __launch_bounds__(RM_THREADS)
visited_overlap_kernel(const uint8_t* __restrict__ bitmap, int64_t ldb, const int* __restrict__ gx, const int* __restrict__ gy,
                       const int64_t* __restrict__ locs_m, const int64_t* __restrict__ num_m, int patch_size, int Nm, int B,
                       int* __restrict__ overlap) {
  __shared__ int s_part[RM_THREADS / 64];
  const int v = blockIdx.x, b = v % B;
  const int X = gx[b], Y = gy[b];
  const int64_t cells = min((int64_t)X * Y, ldb);
  const uint8_t* bm = bitmap + (int64_t)b * ldb;
  const int n = (int)max((int64_t)0, min(num_m[v], (int64_t)Nm));
  int cnt = 0;
  for (int r = threadIdx.x; r < n; r += RM_THREADS) {                       // (a wave takes 64 consecutive rows per step)
    const int64_t cell = cell_of(locs_m + ((int64_t)v * Nm + r) * 2, patch_size, X, Y);
    cnt += (cell >= 0 && cell < cells && bm[cell] != 0) ? 1 : 0;
  }
  const int total = block_sum_i(cnt, s_part);
  if (threadIdx.x == 0) overlap[v] = total;
}

// one workgroup per level-0 cell (paths_level0_batch's geometry): a cleared cell's copy becomes zeros, its row address the zero row's
__global__ void __launch_bounds__(256)
level0_mask_rows_kernel(const int64_t* __restrict__ mask_ptrs, const int* __restrict__ gx, const int* __restrict__ gy, int D, int64_t n0,
                        float* __restrict__ fts, int64_t* __restrict__ row_ptrs, const float* __restrict__ zero_row) {
  const int b = blockIdx.y;
  const int64_t j = blockIdx.x;
  if (j >= (int64_t)gx[b] * gy[b]) return;
  if (reinterpret_cast<const uint8_t*>(mask_ptrs[b])[j] != 0) return;
  const int64_t o = (int64_t)b * n0 + j;
  if (fts != nullptr) {
    const f32x4 z{0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < D / 4; i += 256) stg_f32x4(fts + o * D + 4 * i, z);
  }
  if (row_ptrs != nullptr && threadIdx.x == 0) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);
}

extern "C" {

int paths_rank_joint_tile(void) { return RJ_TILE; }

int paths_rank_joint(const float* scores, const int* seg_end, const int* level_on, const int64_t* num_ims, int L, int B, int n_tot,
                     int ascending, int* rank, int* count, hipStream_t stream) {
  PATHS_REQUIRE(scores != nullptr && seg_end != nullptr && level_on != nullptr && num_ims != nullptr && rank != nullptr && count != nullptr,
                "rank_joint: null pointer (scores, seg_end, level_on, num_ims, rank and count are required)");
  PATHS_REQUIRE(L > 0 && L <= RJ_MAX_LEVELS, "rank_joint: L (%d) must be in [1, %d]", L, RJ_MAX_LEVELS);
  PATHS_REQUIRE(B > 0 && B <= 65535, "rank_joint: B (%d) must be in [1, 65535]", B);
  PATHS_REQUIRE(n_tot > 0 && n_tot <= (1 << 30), "rank_joint: n_tot (%d) must be in [1, 2^30]", n_tot);
  PATHS_REQUIRE((uintptr_t)scores % 4 == 0 && (uintptr_t)seg_end % 4 == 0 && (uintptr_t)level_on % 4 == 0 && (uintptr_t)rank % 4 == 0 &&
                    (uintptr_t)count % 4 == 0 && (uintptr_t)num_ims % 8 == 0,
                "rank_joint: scores, seg_end, level_on, rank and count must be 4-byte aligned, num_ims 8-byte aligned");
  hipLaunchKernelGGL(rank_joint_kernel, dim3((unsigned)((n_tot + RJ_THREADS - 1) / RJ_THREADS), (unsigned)B), dim3(RJ_THREADS), 0, stream,
                     scores, seg_end, level_on, num_ims, L, B, n_tot, ascending != 0 ? 1 : 0, rank, count);
  PATHS_LAUNCH_CHECK("rank_joint");
  return PATHS_OK;
}

int paths_removal_masks(const int64_t* src_ptrs, const int* gx, const int* gy, int64_t max_cells, const int64_t* locs, int patch_size,
                        const int64_t* num_ims, const int* rank, int64_t ldr, const int* thr, int N, int B, int C, int set, uint8_t* masks,
                        int64_t ldm, int* left, hipStream_t stream) {
  PATHS_REQUIRE(gx != nullptr && gy != nullptr && locs != nullptr && num_ims != nullptr && masks != nullptr && left != nullptr,
                "removal_masks: null pointer (gx, gy, locs, num_ims, masks and left are required)");
  PATHS_REQUIRE((rank == nullptr) == (thr == nullptr), "removal_masks: rank and thr come together (both NULL: every valid row is chosen)");
  PATHS_REQUIRE(N > 0 && patch_size > 0, "removal_masks: N (%d) and patch_size (%d) must be positive", N, patch_size);
  PATHS_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 65535, "removal_masks: B (%d) and C (%d) must be in [1, 65535]", B, C);
  PATHS_REQUIRE(max_cells > 0 && max_cells <= ((int64_t)1 << 31) - RM_CELLS, "removal_masks: max_cells (%lld) must be in [1, 2^31)",
                (long long)max_cells);
  PATHS_REQUIRE(ldm >= max_cells && ldm % 16 == 0, "removal_masks: mask stride (%lld) must be a multiple of 16 and at least max_cells (%lld)",
                (long long)ldm, (long long)max_cells);
  PATHS_REQUIRE(rank == nullptr || ldr >= N, "removal_masks: rank stride (%lld) must be at least N (%d)", (long long)ldr, N);
  PATHS_REQUIRE((uintptr_t)masks % 16 == 0 && (uintptr_t)left % 4 == 0 && (uintptr_t)rank % 4 == 0 && (uintptr_t)thr % 4 == 0 &&
                    (uintptr_t)gx % 4 == 0 && (uintptr_t)gy % 4 == 0 && (uintptr_t)locs % 8 == 0 && (uintptr_t)num_ims % 8 == 0 &&
                    (uintptr_t)src_ptrs % 8 == 0,
                "removal_masks: masks must be 16-byte aligned, left, rank, thr, gx and gy 4-byte, locs, num_ims and src_ptrs 8-byte");
  hipLaunchKernelGGL(removal_masks_kernel, dim3((unsigned)((max_cells + RM_CELLS - 1) / RM_CELLS), (unsigned)B, (unsigned)C), dim3(RM_THREADS), 0,
                     stream, src_ptrs, gx, gy, locs, patch_size, num_ims, rank, ldr, thr, N, B, set != 0 ? 1 : 0, masks, ldm, left);
  PATHS_LAUNCH_CHECK("removal_masks");
  return PATHS_OK;
}

int paths_visited_overlap(const uint8_t* bitmap, int64_t ldb, const int* gx, const int* gy, const int64_t* locs_m, const int64_t* num_m,
                          int patch_size, int Nm, int B, int C, int* overlap, hipStream_t stream) {
  PATHS_REQUIRE(bitmap != nullptr && gx != nullptr && gy != nullptr && locs_m != nullptr && num_m != nullptr && overlap != nullptr,
                "visited_overlap: null pointer (bitmap, gx, gy, locs_m, num_m and overlap are required)");
  PATHS_REQUIRE(Nm > 0 && patch_size > 0 && ldb > 0, "visited_overlap: Nm (%d), patch_size (%d) and the bitmap stride (%lld) must be positive", Nm,
                patch_size, (long long)ldb);
  PATHS_REQUIRE(B > 0 && C > 0 && (int64_t)B * C <= 0x7fffffff, "visited_overlap: B (%d) and C (%d) must be positive, B * C below 2^31", B, C);
  PATHS_REQUIRE((uintptr_t)gx % 4 == 0 && (uintptr_t)gy % 4 == 0 && (uintptr_t)overlap % 4 == 0 && (uintptr_t)locs_m % 8 == 0 &&
                    (uintptr_t)num_m % 8 == 0,
                "visited_overlap: gx, gy and overlap must be 4-byte aligned, locs_m and num_m 8-byte aligned");
  hipLaunchKernelGGL(visited_overlap_kernel, dim3((unsigned)(B * C)), dim3(RM_THREADS), 0, stream, bitmap, ldb, gx, gy, locs_m, num_m, patch_size,
                     Nm, B, overlap);
  PATHS_LAUNCH_CHECK("visited_overlap");
  return PATHS_OK;
}

int paths_level0_mask_rows(const int64_t* mask_ptrs, const int* gx, const int* gy, int B, int D, int64_t n0, float* fts, int64_t* row_ptrs,
                           const float* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(mask_ptrs != nullptr && gx != nullptr && gy != nullptr, "level0_mask_rows: null pointer (mask_ptrs, gx and gy are required)");
  PATHS_REQUIRE(B > 0 && B <= 65535 && n0 > 0 && n0 <= 0x7fffffff && D > 0 && D % 4 == 0, "level0_mask_rows: bad shape (B %d, n0 %lld, D %d)", B,
                (long long)n0, D);
  PATHS_REQUIRE((fts != nullptr || row_ptrs != nullptr) && (row_ptrs == nullptr || zero_row != nullptr),
                "level0_mask_rows: the rows are a copy (fts) or row pointers with the zero row");
  PATHS_REQUIRE((uintptr_t)fts % 16 == 0, "level0_mask_rows: fts must be 16-byte aligned");
  hipLaunchKernelGGL(level0_mask_rows_kernel, dim3((unsigned)n0, (unsigned)B), dim3(256), 0, stream, mask_ptrs, gx, gy, D, n0, fts, row_ptrs,
                     zero_row);
  PATHS_LAUNCH_CHECK("level0_mask_rows");
  return PATHS_OK;
}

}  // extern "C"
