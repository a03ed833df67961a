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
#include "common.h"
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

}  // extern "C"
