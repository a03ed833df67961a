// paths_topk_tiled / paths_topk_rows_tiled: the top-K of paths_topk / paths_topk_rows (select.hip) for levels of more patches than fit
// in LDS.  Same contract, byte for byte (tests/select_ref.py::topk), same 64-bit key (rank_key.h), same parameter lists; n_max and ldk
// go up to PATHS_TOPK_TILED_MAX = 65,535, the most patches the token-0 attention entries take beside the special token.  DESIGN 22.
//
// select.hip's kernel holds ALL keys of a slide in LDS (n <= 8192: 64 KiB, an LDS opt-in).  Here the keys are STREAMED, as in
// rank_joint_kernel (perturb_rows.hip), through one static TT_TILE-key tile (16 KiB: no opt-in, up to 8 workgroups per CU); the
// workgroup itself is select.hip's: it owns TT_ELEMS = 64 elements, lane l of every wave owns element 64 blockIdx.x + l, the four
// waves count over a quarter of each tile's keys (key pairs read by 16-byte LDS broadcast) and the partial counts meet in LDS once,
// after the last tile.  (One element per THREAD, rank_joint_kernel's layout, is a quarter of the workgroups: at n just past 8,192
// and 8 slides that is one workgroup, one wave per SIMD, per CU, and the LDS latency shows - 117 us against 75 us for the resident
// kernel at n = 8192)  rank_i = #{j < n : key_j < key_i}; keys are unique, so the ranks of a slide are a permutation of
// 0 .. n - 1 and element i goes to keep_idx[b, rank_i] iff rank_i < count.  Integer counts: no atomics, no workspace, a rerun is
// bit-identical.  Keys are built for j < n only (no score at or beyond num_ims[b] is read); a tile that starts at or beyond n is
// never built.  keep < 0 (keep all, original order) ranks nothing.
//
// Cost per slide: n^2 64-bit compares (a compare and an add-with-carry each); n / TT_ELEMS workgroups that each build all n keys once
// (4 n bytes of scores, from cache) and read each of them back from LDS once.  ONE launch, through PATHS_LAUNCH_STOP: the kernel's
// completion signal carries the recursion's fork, like the twins'.
#include "common.h"
#include "rank_key.h"

namespace {

constexpr int TT_THREADS = 256;
constexpr int TT_ELEMS = 64;         // elements per workgroup: one per lane, the same in all four waves
constexpr int TT_TILE = 2048;        // keys per LDS tile (rank_joint_kernel's measured size)
static_assert(TT_TILE % 8 == 0 && TT_TILE % TT_THREADS == 0 && TT_THREADS == 4 * TT_ELEMS, "four waves, a quarter of a tile's key pairs each");

__global__ void __launch_bounds__(TT_THREADS)
topk_tiled_kernel(const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ num_ims, int n_max, int keep,
                  int* __restrict__ keep_idx, int64_t ldk, int* __restrict__ keep_count,
                  const float* __restrict__ row_base, int64_t row_ld, int64_t slide_rows,         // optional: kept_rows[b, i] = address of
                  int64_t* __restrict__ kept_rows, const float* __restrict__ zero_row) {           // row_base[b, keep_idx[b, i], :] (zero_row beyond count)
  __shared__ __attribute__((aligned(16))) unsigned long long keys[TT_TILE];
  __shared__ int part[4][TT_ELEMS];                                         // partial counts of the four waves
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = (int)max((int64_t)0, min(num_ims[b], (int64_t)n_max));      // (device data: clamped before it bounds anything)
  const int count = keep < 0 ? n : min(n, keep);                            // (<= ldk: the entry points require ldk >= min(keep, n_max))
  const int i0 = blockIdx.x * TT_ELEMS, i = i0 + lane;                      // this lane's element
  if (blockIdx.x == 0 && tid == 0) keep_count[b] = count;
  auto row_addr = [&](int idx) { return (int64_t)reinterpret_cast<uintptr_t>(row_base + ((int64_t)b * slide_rows + idx) * row_ld); };
  // entries [count, ldk) of the row table point at the zero row (every workgroup covers its own TT_ELEMS positions)
  if (kept_rows && wave == 0 && i >= count && i < ldk) kept_rows[(int64_t)b * ldk + i] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);
  if (i0 >= n) return;                                                      // nothing valid here (workgroup-uniform)
  if (keep < 0) {                                                           // keep all, original order
    if (wave == 0 && i < n) {
      keep_idx[(int64_t)b * ldk + i] = i;
      if (kept_rows) kept_rows[(int64_t)b * ldk + i] = row_addr(i);
    }
    return;
  }
  const float* s = scores + (int64_t)b * ld;
  const unsigned long long mine = i < n ? topk_key(s[i], i) : 0ull;         // (0: below every key, counts nothing, is never written)
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2* kp = reinterpret_cast<const u64x2*>(keys);
  int cnt = 0;
  for (int t0 = 0; t0 < n; t0 += TT_TILE) {                                 // (n is workgroup-uniform: so are the barriers)
    const int len = min(TT_TILE, n - t0), np = (len + 7) & ~7;              // keys beyond len: all ones (never below a real key)
    for (int j = tid; j < np; j += TT_THREADS) keys[j] = j < len ? topk_key(s[t0 + j], t0 + j) : ~0ull;
    __syncthreads();
    // a quarter of the tile's key PAIRS per wave
    const int pairs = np >> 1, q0 = (pairs * wave) >> 2, q1 = (pairs * (wave + 1)) >> 2;
    int q = q0;
    for (; q + 4 <= q1; q += 4) {
      const u64x2 a = kp[q], c = kp[q + 1], d = kp[q + 2], e = kp[q + 3];
      cnt += (a[0] < mine) + (a[1] < mine) + (c[0] < mine) + (c[1] < mine) + (d[0] < mine) + (d[1] < mine) + (e[0] < mine) + (e[1] < mine);
    }
    for (; q < q1; ++q) { const u64x2 a = kp[q]; cnt += (a[0] < mine) + (a[1] < mine); }
    __syncthreads();                                                        // the tile is consumed before the next one is written
  }
  part[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && i < n) {
    const int rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    if (rank < count) {
      keep_idx[(int64_t)b * ldk + rank] = i;
      if (kept_rows) kept_rows[(int64_t)b * ldk + rank] = row_addr(i);
    }
  }
}

// the checks both entry points share (`what`: the entry point's name in messages), then the one launch
int launch_topk_tiled(const char* what, const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep, int* keep_idx,
                      int64_t ldk, int* keep_count, bool rows, const float* row_base, int64_t row_ld, int64_t slide_rows, int64_t* kept_rows,
                      const float* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0, "%s: B (%d) must be > 0", what, B);
  PATHS_REQUIRE(n_max >= 1 && n_max <= PATHS_TOPK_TILED_MAX, "%s: n_max (%d) must be in [1, %d]", what, n_max, PATHS_TOPK_TILED_MAX);
  PATHS_REQUIRE(keep == -1 || keep > 0, "%s: keep (%d) must be -1 (all) or > 0", what, keep);
  const int need = keep < 0 ? n_max : (keep < n_max ? keep : n_max);
  PATHS_REQUIRE(ldk >= need, "%s: ldk (%lld) is shorter than the %d entries a keep_idx row needs", what, (long long)ldk, need);
  PATHS_REQUIRE(ldk <= PATHS_TOPK_TILED_MAX, "%s: ldk (%lld) must be at most %d", what, (long long)ldk, PATHS_TOPK_TILED_MAX);
  PATHS_REQUIRE(ld >= n_max, "%s: ld (%lld) is shorter than n_max (%d)", what, (long long)ld, n_max);
  PATHS_REQUIRE(scores && num_ims && keep_idx && keep_count, "%s: null pointer (scores, num_ims, keep_idx and keep_count are required)", what);
  if (rows) {
    PATHS_REQUIRE(row_base && kept_rows && zero_row, "%s: null pointer among the row table arguments (row_base, kept_rows, zero_row)", what);
    PATHS_REQUIRE(row_ld > 0, "%s: row_ld (%lld) must be > 0", what, (long long)row_ld);
    PATHS_REQUIRE(slide_rows >= n_max, "%s: slide_rows (%lld) is below n_max (%d)", what, (long long)slide_rows, n_max);
  }
  // x covers every element AND every position of the kept-row table (ldk exceeds n_max only through padding)
  const int cover = (int)(ldk > n_max ? ldk : n_max);
  PATHS_LAUNCH_STOP(topk_tiled_kernel, dim3((cover + TT_ELEMS - 1) / TT_ELEMS, B), dim3(TT_THREADS), 0, stream, scores, ld, num_ims, n_max,
                    keep, keep_idx, ldk, keep_count, row_base, row_ld, slide_rows, kept_rows, zero_row);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

}  // namespace

extern "C" {

int paths_topk_tiled(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                     int* keep_idx, int64_t ldk, int* keep_count, hipStream_t stream) {
  return launch_topk_tiled("topk_tiled", scores, ld, num_ims, B, n_max, keep, keep_idx, ldk, keep_count, false, nullptr, 0, 0, nullptr, nullptr,
                           stream);
}

int paths_topk_rows_tiled(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                          int* keep_idx, int64_t ldk, int* keep_count, const float* row_base, int64_t row_ld, int64_t slide_rows,
                          int64_t* kept_rows, const float* zero_row, hipStream_t stream) {
  return launch_topk_tiled("topk_rows_tiled", scores, ld, num_ims, B, n_max, keep, keep_idx, ldk, keep_count, true, row_base, row_ld, slide_rows,
                           kept_rows, zero_row, stream);
}

}  // extern "C"
