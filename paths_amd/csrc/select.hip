// Device-resident patch selection: importance top-K, 4-child expansion, bounds/background filter, stable
// compaction and the row gathers that build the next magnification level's batch.
//
// Replaces the per-slide host loop of the reference (utils.py:248-260 -> data_utils/slide.py:277-331 and
// data_utils/dataset.py:206-235): .cpu() sync, torch.topk, torch.cat of 4 child blocks, boolean filters,
// host-RAM gather of child features, re-padding.  Nothing here synchronises with the host.
//
// All of it is HBM-bound integer / copy work: rows are 4 KB (features) and 5 KB (LSTM state) and move as
// coalesced 16-byte-per-lane copies; the per-slide bookkeeping (sort, scan) lives in LDS.
#include "common.h"
#include "rank_key.h"

namespace {

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}

// Feature grids are fp32 or fp16 (DeviceSlide dtype).  Rows are read 4 values at a time (16 or 8 bytes per lane) and widened to fp32
// exactly, so every pass below computes on an fp16 grid what it computes on an fp32 grid holding the same values.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ f32x4 load4(const T* row, int64_t i) {     // elements 4 i .. 4 i + 3 of a row
  if constexpr (sizeof(T) == 4) {
    return reinterpret_cast<const f32x4*>(row)[i];
  } else {
    const f16x4 h = reinterpret_cast<const f16x4*>(row)[i];
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
  }
}

// ------------------------------------------------------------------------------------------------
// top-K: indices of the `keep` largest scores, ordered by (score descending, index ascending).
// torch.topk (slide.py:298) leaves tie order unspecified; this rule equals it whenever scores are distinct.
//
// Selection by RANK COUNTING instead of a sort: with the 64-bit key (~monotone(score) << 32 | index) every element's output
// position is simply the number of keys below its own, rank_i = #{j : key_j < key_i} (keys are unique), and it is kept iff
// rank_i < count.  That is O(n^2) compares, but they are independent: 64 elements per workgroup x n/64 workgroups per slide put
// the whole chip on a top-K that a one-workgroup-per-slide bitonic sort (66 dependent stages at n = 2048, 21 us) ran on 8 CUs.
// Each workgroup builds all n keys of its slide in LDS (n <= 8192: 64 KiB); lane l of every wave owns element 64 blockIdx.x + l,
// the four waves count over a quarter of the keys each (key pairs read by LDS broadcast), partial counts meet in LDS.
// ------------------------------------------------------------------------------------------------
constexpr int TOPK_MAX = 8192;

__global__ void __launch_bounds__(256)
topk_rank_kernel(const float* __restrict__ scores, int64_t ld, const int64_t* __restrict__ num_ims, int keep,
                 int* __restrict__ keep_idx, int64_t ldk, int* __restrict__ keep_count,
                 const float* __restrict__ row_base, int64_t row_ld, int64_t slide_rows,        // optional: kept_rows[b, i] = address of
                 int64_t* __restrict__ kept_rows, const float* __restrict__ zero_row) {          // row_base[b, keep_idx[b, i], :] (zero_row beyond count)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = (int)num_ims[b];
  const int count = keep < 0 ? n : min(n, keep);
  const int i = blockIdx.x * 64 + lane;                 // this lane's element
  if (blockIdx.x == 0 && tid == 0) keep_count[b] = count;
  auto row_addr = [&](int idx) { return (int64_t)reinterpret_cast<uintptr_t>(row_base + ((int64_t)b * slide_rows + idx) * row_ld); };
  // entries [count, ldk) of the row table point at the zero row (every workgroup covers its own 64 positions)
  if (kept_rows && wave == 0 && i >= count && i < ldk) kept_rows[(int64_t)b * ldk + i] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);
  if (blockIdx.x * 64 >= n) return;                     // nothing valid here (workgroup-uniform)
  if (keep < 0) {                                       // keep all, original order (slide.py:294 not taken)
    if (wave == 0 && i < n) {
      keep_idx[(int64_t)b * ldk + i] = i;
      if (kept_rows) kept_rows[(int64_t)b * ldk + i] = row_addr(i);
    }
    return;
  }
  const int np = (n + 7) & ~7;                          // keys beyond n: all ones (never below a real key)
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  int* part = reinterpret_cast<int*>(smem + (size_t)((np + 1) & ~1) * 8);      // [4][64] partial counts
  const float* s = scores + (int64_t)b * ld;
  for (int j = tid; j < np; j += 256) keys[j] = j < n ? topk_key(s[j], j) : ~0ull;
  __syncthreads();
  const unsigned long long mine = i < n ? keys[i] : 0ull;
  // quarter of the key range per wave, in units of key PAIRS (16-byte broadcast reads)
  const int pairs = np >> 1, q0 = (pairs * wave) >> 2, q1 = (pairs * (wave + 1)) >> 2;
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2* kp = reinterpret_cast<const u64x2*>(keys);
  int cnt = 0;
  int q = q0;
  for (; q + 4 <= q1; q += 4) {
    const u64x2 a = kp[q], c = kp[q + 1], d = kp[q + 2], e = kp[q + 3];
    cnt += (a[0] < mine) + (a[1] < mine) + (c[0] < mine) + (c[1] < mine) + (d[0] < mine) + (d[1] < mine) + (e[0] < mine) + (e[1] < mine);
  }
  for (; q < q1; ++q) { const u64x2 a = kp[q]; cnt += (a[0] < mine) + (a[1] < mine); }
  part[wave * 64 + lane] = cnt;
  __syncthreads();
  if (wave == 0 && i < n) {
    const int rank = part[lane] + part[64 + lane] + part[128 + lane] + part[192 + lane];
    if (rank < count) {
      keep_idx[(int64_t)b * ldk + rank] = i;
      if (kept_rows) kept_rows[(int64_t)b * ldk + rank] = row_addr(i);
    }
  }
}

static int launch_topk(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep, int* keep_idx, int64_t ldk,
                       int* keep_count, const float* row_base, int64_t row_ld, int64_t slide_rows, int64_t* kept_rows,
                       const float* zero_row, hipStream_t stream) {
  const size_t lds = (size_t)(((n_max + 7) & ~7) + 2) * 8 + 4 * 64 * sizeof(int);
  PATHS_LDS_OPT_IN(topk_rank_kernel, (TOPK_MAX + 2) * 8 + 1024, "topk");
  // x covers every element AND every position of the kept-row table (ldk may exceed n_max only through padding; both <= TOPK_MAX)
  const int cover = (int)(ldk > n_max ? ldk : n_max);
  PATHS_LAUNCH_STOP(topk_rank_kernel, dim3((cover + 63) / 64, B), dim3(256), lds, stream, scores, ld, num_ims, keep, keep_idx, ldk,
                    keep_count, row_base, row_ld, slide_rows, kept_rows, zero_row);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// expansion: kept patch (x,y) -> blocks (2x,2y) | (2x,2y+1) | (2x+1,2y) | (2x+1,2y+1), each in top-K
// order (slide.py:307-315); keep child iff in bounds and tissue (slide.py:320-325); stable compaction.
//
// Two forms.  expand_kernel does all of it for resident slides.  An on-demand slide (paths_amd/data_utils/slide.py:OnDemandSlide;
// reference RawSlide.recurse, data_utils/slide.py:173-198) has no tissue mask of the next grid - whether a cell is tissue is known
// only once the caller has encoded it - so there the expansion is split around the caller: candidate_kernel is the first half
// (children, bounds, stable compaction: the cells the caller is asked for), admit_kernel the second (tissue filter over the rows the
// caller supplied, stable compaction, bookkeeping).  One workgroup per slide in all of them; the pieces are stated once, below.
// ------------------------------------------------------------------------------------------------
// threads of the one workgroup per slide.  Alone the kernel is fastest at 1024 (11.7 us against 15.1 / 23.5 at 512 / 256), but a
// 16-wave workgroup has to wait for a CU with four free wave slots per SIMD beside the aggregator's kernels: in the recursion 512
// gives 3,591-3,624 slides/s against 3,527-3,535 (sustained 3,717-3,731 against 3,609-3,616), 256 gives 3,589-3,618
constexpr int EXP_NT = 512;
// candidates per thread whose evaluation is kept in registers between the counting and the writing pass (at keep = 512 a thread owns four)
constexpr int EXP_CACHE = 4;

// cell of the child in block blk (0..3, block order of slide.py:305-315) of the patch at pixel (lx, ly); true iff inside the X x Y grid
__device__ __forceinline__ bool child_cell(int64_t lx, int64_t ly, int blk, int patch_size, int X, int Y, int& cx, int& cy) {
  const bool small = (uint64_t)(lx | ly) < 0x80000000ull;       // (pixel coordinates: a 32-bit division is a fraction of the 64-bit one)
  const int64_t px = small ? (int64_t)((int)lx / patch_size) : lx / patch_size;
  const int64_t py = small ? (int64_t)((int)ly / patch_size) : ly / patch_size;
  const int64_t x = 2 * px + (blk >> 1), y = 2 * py + (blk & 1);
  cx = (int)x; cy = (int)y;                                     // (exact for every cell inside the grid)
  return x >= 0 && y >= 0 && x < X && y < Y;
}

// exclusive prefix of `mine` over the NT threads of the workgroup; total = the sum over all of them.  Shuffles inside a wave, the
// wave totals through LDS: two barriers instead of the twenty of a Hillis-Steele scan over LDS.  Once per kernel (the LDS is its own).
template <int NT>
__device__ __forceinline__ int exp_scan(int mine, int& total) {
  constexpr int NW = NT / 64;
  __shared__ int part[2 * NW];
  const int tid = threadIdx.x;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if ((tid & 63) >= off) incl += v;
  }
  if ((tid & 63) == 63) part[tid >> 6] = incl;
  __syncthreads();
  if (tid < NW) {
    int t = part[tid];
#pragma unroll
    for (int off = 1; off < NW; off <<= 1) {
      const int v = __shfl_up(t, off);
      if (tid >= off) t += v;
    }
    part[NW + tid] = t;                                 // inclusive totals of waves 0 .. tid
  }
  __syncthreads();
  total = part[2 * NW - 1];
  return incl - mine + ((tid >> 6) ? part[NW + (tid >> 6) - 1] : 0);
}

// The candidates c = blk * count + i (i: kept slot) of one slide, in order, a contiguous run of them per thread.  A candidate is kept
// iff its cell is inside the grid and (TISSUE) its mask byte is set.  head(number kept) runs once the count is known and says whether
// to go on; then emit(c, kept, cx, cy, i, pos) runs for every candidate, pos = number of kept candidates before c.  Returns head's answer.
// kidx: the slide's kept indices, loc: the slide's locations [., 2].
//
// The first EXP_CACHE candidates of a thread are evaluated ONCE and replayed from registers in the emit pass.  Each evaluation is a
// chain of dependent loads (kept index -> its location -> the tissue byte), so they run in stages, the chains of a thread side by
// side: all kept indices, then all locations, then all cells, then all mask bytes.  Candidates beyond the cache are evaluated twice.
template <bool TISSUE, class Head, class Emit>
__device__ __forceinline__ bool for_each_child(const int* __restrict__ kidx, int count, const int64_t* __restrict__ loc, int patch_size,
                                               int X, int Y, const uint8_t* __restrict__ mask, Head head, Emit emit) {
  const int tid = threadIdx.x, total = 4 * count;
  const int per = (total + EXP_NT - 1) / EXP_NT;
  const int c0 = min(tid * per, total), c1 = min(c0 + per, total);
  auto child = [&](int c, int& cx, int& cy, int& i) -> bool {
    const int blk = c / count;
    i = c - blk * count;
    const int64_t* l = loc + 2 * (int64_t)kidx[i];
    if (!child_cell(l[0], l[1], blk, patch_size, X, Y, cx, cy)) return false;
    return !TISSUE || mask[(int64_t)cx * Y + cy] != 0;
  };

  int ccx[EXP_CACHE], ccy[EXP_CACHE], cci[EXP_CACHE];
  bool ckeep[EXP_CACHE];
  int mine = 0;
  {
    int blk[EXP_CACHE], prow[EXP_CACHE];
    bool on[EXP_CACHE];
    int64_t lx[EXP_CACHE], ly[EXP_CACHE];
#pragma unroll
    for (int u = 0; u < EXP_CACHE; ++u) {
      on[u] = c0 + u < c1;
      const int c = on[u] ? c0 + u : 0;
      blk[u] = count > 0 ? c / count : 0;
      cci[u] = c - blk[u] * count;
      prow[u] = on[u] ? kidx[cci[u]] : 0;
    }
#pragma unroll
    for (int u = 0; u < EXP_CACHE; ++u) {
      lx[u] = on[u] ? loc[2 * (int64_t)prow[u]] : 0;
      ly[u] = on[u] ? loc[2 * (int64_t)prow[u] + 1] : 0;
    }
#pragma unroll
    for (int u = 0; u < EXP_CACHE; ++u) ckeep[u] = child_cell(lx[u], ly[u], blk[u], patch_size, X, Y, ccx[u], ccy[u]) && on[u];
    if constexpr (TISSUE) {
#pragma unroll
      for (int u = 0; u < EXP_CACHE; ++u) ckeep[u] = ckeep[u] && mask[(int64_t)ccx[u] * Y + ccy[u]] != 0;
    }
#pragma unroll
    for (int u = 0; u < EXP_CACHE; ++u) mine += ckeep[u] ? 1 : 0;
  }
  for (int c = c0 + EXP_CACHE; c < c1; ++c) { int cx, cy, i; mine += child(c, cx, cy, i) ? 1 : 0; }
  int kept;
  int pos = exp_scan<EXP_NT>(mine, kept);
  if (!head(kept)) return false;
  for (int c = c0; c < c1; ++c) {
    int cx = 0, cy = 0, i = 0;
    bool keepc;
    const int u = c - c0;
    if (u < EXP_CACHE) {
      keepc = false;
#pragma unroll
      for (int v = 0; v < EXP_CACHE; ++v)
        if (v == u) { keepc = ckeep[v]; cx = ccx[v]; cy = ccy[v]; i = cci[v]; }
    } else {
      keepc = child(c, cx, cy, i);
    }
    emit(c, keepc, cx, cy, i, pos);
    pos += keepc ? 1 : 0;
  }
  return true;
}

// The bookkeeping rows of the children of slide b = base / n_next: where a child lies, which patch it descends from, and where its
// parent state (src_row) and its features (src_cell) are read.  hp_row (child -> row of the kept-parent table) is optional.
struct ChildRows {
  int64_t* locs_out; int64_t* parent_out; int* src_row; int* src_cell; int* hp_row;
  int64_t base;
  __device__ __forceinline__ void put(int pos, int64_t cx, int64_t cy, int patch_size, int64_t parent, int srow, int scell, int hp) const {
    const int64_t o = base + pos;
    locs_out[2 * o] = cx * patch_size;
    locs_out[2 * o + 1] = cy * patch_size;
    parent_out[o] = parent;
    src_row[o] = srow;
    src_cell[o] = scell;
    if (hp_row) hp_row[o] = hp;
  }
  // padding tail [n_out, n_next): zero rows like collate_fn's zero padding (dataset.py:216-218)
  __device__ __forceinline__ void pad(int n_out, int64_t n_next) const {
    for (int j = n_out + threadIdx.x; j < n_next; j += EXP_NT) put(j, 0, 0, 0, 0, -1, -1, -1);
  }
};

// thread 0 publishes the number of children of its slide; false = over capacity: the workgroup writes nothing else
__device__ __forceinline__ bool publish_count(int n_out, int64_t n_next, int64_t* __restrict__ num_out_b, int* __restrict__ status) {
  if (threadIdx.x == 0) {
    *num_out_b = n_out;
    if (n_out == 0) atomicOr(status, 1);               // no tissue among the children: the reference falls back to "all cells" (slide.py:336-352)
    if (n_out > n_next) atomicOr(status, 2);
  }
  return n_out <= n_next;
}

__global__ void __launch_bounds__(EXP_NT)
expand_kernel(const int* __restrict__ keep_idx, int64_t ldk, const int* __restrict__ keep_count,
              const int64_t* __restrict__ locs, int64_t n_cur, int patch_size,
              const int* __restrict__ next_x, const int* __restrict__ next_y,          // [B] next-level grid dims
              const int64_t* __restrict__ mask_ptrs,                                     // [B] -> uint8 [X*Y], 1 = tissue
              int64_t n_next,
              int64_t* __restrict__ num_out, int64_t* __restrict__ locs_out, int64_t* __restrict__ parent_out,
              int* __restrict__ src_row, int* __restrict__ src_cell, int* __restrict__ status,
              int* __restrict__ child_pos /*[B, 4*ldk] or null: output row of every candidate child, -1 if dropped*/,
              int* __restrict__ hp_row /*[B, n_next] or null: row of the kept-parent table (b*ldk + i) of every child*/) {
  const int b = blockIdx.x;
  const int count = max(0, min(keep_count[b], (int)ldk));      // (keep_idx holds ldk entries per slide, child_pos 4 * ldk)
  const int Y = next_y[b];
  const int* kidx = keep_idx + (int64_t)b * ldk;
  const ChildRows rows{locs_out, parent_out, src_row, src_cell, hp_row, (int64_t)b * n_next};
  int n_out = 0;
  const bool fits = for_each_child<true>(
      kidx, count, locs + (int64_t)b * n_cur * 2, patch_size, next_x[b], Y, reinterpret_cast<const uint8_t*>(mask_ptrs[b]),
      [&](int kept) { n_out = kept; return publish_count(kept, n_next, num_out + b, status); },
      [&](int c, bool keepc, int cx, int cy, int i, int pos) {
        if (child_pos) child_pos[(int64_t)b * 4 * ldk + c] = keepc ? pos : -1;
        if (keepc) rows.put(pos, cx, cy, patch_size, i, kidx[i], cx * Y + cy, (int)((int64_t)b * ldk + i));
      });
  if (fits) rows.pad(n_out, n_next);
}

__global__ void __launch_bounds__(EXP_NT)
candidate_kernel(const int* __restrict__ keep_idx, int64_t ldk, const int* __restrict__ keep_count,
                 const int64_t* __restrict__ locs, int64_t n_cur, int patch_size,
                 const int* __restrict__ next_x, const int* __restrict__ next_y,
                 int* __restrict__ cand_count, int64_t* __restrict__ cand_cells /*[B, 4*ldk, 2]*/, int* __restrict__ cand_slot /*[B, 4*ldk]*/) {
  const int b = blockIdx.x;
  const int count = max(0, min(keep_count[b], (int)ldk));      // (the tables hold 4 * ldk entries per slide)
  const int64_t row = (int64_t)b * 4 * ldk;
  int n_cand = 0;
  for_each_child<false>(
      keep_idx + (int64_t)b * ldk, count, locs + (int64_t)b * n_cur * 2, patch_size, next_x[b], next_y[b], nullptr,
      [&](int kept) { n_cand = kept; if (threadIdx.x == 0) cand_count[b] = kept; return true; },
      [&](int, bool keepc, int cx, int cy, int i, int pos) {
        if (keepc) { cand_cells[2 * (row + pos)] = cx; cand_cells[2 * (row + pos) + 1] = cy; cand_slot[row + pos] = i; }
      });
  // padding: no cell, no slot
  for (int64_t j = n_cand + threadIdx.x; j < 4 * ldk; j += EXP_NT) {
    cand_cells[2 * (row + j)] = -1; cand_cells[2 * (row + j) + 1] = -1; cand_slot[row + j] = -1;
  }
}

__global__ void __launch_bounds__(EXP_NT)
admit_kernel(const int* __restrict__ cand_count, const int64_t* __restrict__ cand_cells, const int* __restrict__ cand_slot,
             const uint8_t* __restrict__ cand_mask /*[B, 4*ldk]: 1 = the supplied row is tissue*/,
             const int* __restrict__ keep_idx, int64_t ldk, const int* __restrict__ keep_count, int patch_size, int64_t n_next,
             int64_t* __restrict__ num_out, int64_t* __restrict__ locs_out, int64_t* __restrict__ parent_out,
             int* __restrict__ src_row, int* __restrict__ src_cell, int* __restrict__ status,
             int* __restrict__ child_pos /*[B, 4*ldk] or null*/, int* __restrict__ hp_row /*[B, n_next] or null*/) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t row = (int64_t)b * 4 * ldk;
  const int n_cand = (int)max((int64_t)0, min((int64_t)cand_count[b], 4 * ldk));
  const int per = (n_cand + EXP_NT - 1) / EXP_NT;
  const int j0 = min(tid * per, n_cand), j1 = min(j0 + per, n_cand);
  const int count = max(0, min(keep_count[b], (int)ldk));
  // admitted: tissue, and the slot names a kept parent (a table that does not can make nothing below write out of bounds)
  auto admitted = [&](int j) { return cand_mask[row + j] != 0 && (unsigned)cand_slot[row + j] < (unsigned)count; };
  int mine = 0;
  for (int j = j0; j < j1; ++j) mine += admitted(j) ? 1 : 0;
  int n_out;
  int pos = exp_scan<EXP_NT>(mine, n_out);
  if (!publish_count(n_out, n_next, num_out + b, status)) return;
  if (child_pos) {
    // expand_kernel's table is indexed by the candidate BEFORE the bounds filter, c = blk * count + slot: every entry starts as
    // "dropped", the admitted ones are written behind the barrier (blk is the parity of the cell)
    for (int c = tid; c < 4 * count; c += EXP_NT) child_pos[row + c] = -1;
    __syncthreads();
  }
  const ChildRows rows{locs_out, parent_out, src_row, src_cell, hp_row, (int64_t)b * n_next};
  for (int j = j0; j < j1; ++j) {
    if (!admitted(j)) continue;
    const int64_t cx = cand_cells[2 * (row + j)], cy = cand_cells[2 * (row + j) + 1];
    const int i = cand_slot[row + j];
    // (src_cell: the row's index in the slide's candidate buffer)
    rows.put(pos, cx, cy, patch_size, i, keep_idx[(int64_t)b * ldk + i], j, (int)((int64_t)b * ldk + i));
    if (child_pos) child_pos[row + (int)(((cx & 1) << 1) | (cy & 1)) * count + i] = pos;
    ++pos;
  }
  rows.pad(n_out, n_next);
}

// Rare fallback (reference data_utils/slide.py:336-352): a slide whose kept patches have NO tissue children
// continues with every tissue cell of the next grid (or every cell if the grid has no tissue at all), zero patch
// context, parent_inds = cell index.  Only slides with num_out[b] == 0 are touched.
__global__ void __launch_bounds__(1024)
fallback_all_cells_kernel(const int* __restrict__ next_x, const int* __restrict__ next_y, const int64_t* __restrict__ mask_ptrs,
                          int patch_size, int64_t n_next, int64_t* __restrict__ num_out, int64_t* __restrict__ locs_out,
                          int64_t* __restrict__ parent_out, int* __restrict__ src_row, int* __restrict__ src_cell,
                          int* __restrict__ status, int* __restrict__ hp_row) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (num_out[b] != 0) return;
  const int X = next_x[b], Y = next_y[b];
  const int total = X * Y;
  const uint8_t* mask = reinterpret_cast<const uint8_t*>(mask_ptrs[b]);
  const int per = (total + 1023) / 1024;
  const int c0 = min(tid * per, total), c1 = min(c0 + per, total);
  int mine = 0;
  for (int c = c0; c < c1; ++c) mine += mask[c] != 0;
  int tissue;
  const int before = exp_scan<1024>(mine, tissue);
  const bool all = tissue == 0;                       // "hope that there will be tissue later" (slide.py:344-347)
  const int n_out = all ? total : tissue;
  int pos = all ? c0 : before;
  if (tid == 0) {
    num_out[b] = n_out;
    if (n_out > n_next) atomicOr(status, 2);
  }
  if (n_out > n_next) return;
  const ChildRows rows{locs_out, parent_out, src_row, src_cell, hp_row, (int64_t)b * n_next};
  for (int c = c0; c < c1; ++c)
    if (all || mask[c]) rows.put(pos++, c / Y, c % Y, patch_size, c, -1, c, -1);
}

// One WAVE per output row (four rows per workgroup): features from the next-level grid, LSTM state (h|c) from the kept parent.
// (One 256-thread workgroup per row was 16,384 workgroups for 16 MB in the default path - only the 1-KiB memory-cell part of the
// state is copied there, 64 of the 256 threads had anything to do: 14.6 us.)
//
// PACKED (tissue-only slides, pack_rows.hip): grid_ptrs[b] is the slide's first PACKED row and index_ptrs[b] its int32 [X*Y] cell
// index - the row number of a cell, or -1 for a cell whose row was all +0.0 and is not stored.  Such a cell reads as what it was:
// zero_row in the address table, zeros in the copy.  src_cell stays the cell of the dense grid.
constexpr int GATHER_ROWS = 4;
template <class T, bool PACKED = false>
__global__ void __launch_bounds__(256)
gather_kernel(const int64_t* __restrict__ grid_ptrs, const int* __restrict__ src_cell, int D,
              const float* __restrict__ state_cur /*already offset to the first copied column*/, int64_t n_cur, int64_t ld_state_cur,
              const int* __restrict__ src_row, int Dp /*columns copied*/, const int64_t* __restrict__ num_out, int64_t n_next,
              float* __restrict__ fts_out, float* __restrict__ state_out, int zero_pad,
              int64_t* __restrict__ row_ptrs, const float* __restrict__ zero_row, const int64_t* __restrict__ index_ptrs = nullptr) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * GATHER_ROWS + (threadIdx.x >> 6);
  if (j >= n_next) return;
  const int64_t o = (int64_t)b * n_next + j;
  f32x4* fo = fts_out ? reinterpret_cast<f32x4*>(fts_out + o * D) : nullptr;
  f32x4* so = state_out ? reinterpret_cast<f32x4*>(state_out + o * Dp) : nullptr;
  if (j < num_out[b]) {
    int64_t row = src_cell[o];
    if constexpr (PACKED) row = reinterpret_cast<const int*>(index_ptrs[b])[row];           // (-1: a dropped all-zero row)
    const T* fi = reinterpret_cast<const T*>(grid_ptrs[b]) + row * D;
    if (!PACKED || row >= 0) {
      if (row_ptrs && lane == 0) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(fi);   // consumers read the row where it lives
      if (fo) for (int i = lane; i < D / 4; i += 64) fo[i] = load4(fi, i);                  // (gathered copies are fp32)
    } else {
      const f32x4 z{0.f, 0.f, 0.f, 0.f};
      if (row_ptrs && lane == 0) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);
      if (fo) for (int i = lane; i < D / 4; i += 64) fo[i] = z;
    }
    if (so) {
      const int sr = src_row[o];
      if (sr >= 0) {
        const f32x4* si = reinterpret_cast<const f32x4*>(state_cur + ((int64_t)b * n_cur + sr) * ld_state_cur);
        for (int i = lane; i < Dp / 4; i += 64) so[i] = si[i];
      } else {                                   // fallback rows (slide.py:338): fresh zero context
        const f32x4 z{0.f, 0.f, 0.f, 0.f};
        for (int i = lane; i < Dp / 4; i += 64) so[i] = z;
      }
    }
  } else {
    if (row_ptrs && lane == 0) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);   // padding rows: a row of zeros
    if (zero_pad) {
      const f32x4 z{0.f, 0.f, 0.f, 0.f};
      if (fo) for (int i = lane; i < D / 4; i += 64) fo[i] = z;
      if (so) for (int i = lane; i < Dp / 4; i += 64) so[i] = z;
    }
  }
}



// Kept parents' h rows -> compact table [B*ldk, D] (rows beyond keep_count are zero): the A operand of the
// once-per-parent half of the next level's LSTM gate GEMM.
__global__ void __launch_bounds__(256)
gather_kept_rows_kernel(const float* __restrict__ src, int64_t n_cur, int64_t ld_src, const int* __restrict__ keep_idx, int64_t ldk,
                        const int* __restrict__ keep_count, int D, float* __restrict__ out) {
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  f32x4* o = reinterpret_cast<f32x4*>(out + ((int64_t)b * ldk + i) * D);
  if (i < keep_count[b]) {
    const f32x4* r = reinterpret_cast<const f32x4*>(src + ((int64_t)b * n_cur + keep_idx[(int64_t)b * ldk + i]) * ld_src);
    for (int c = tid; c < D / 4; c += 256) o[c] = r[c];
  } else {
    const f32x4 z{0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < D / 4; c += 256) o[c] = z;
  }
}

// Backward of the parent-state gather (reference data_utils/slide.py:318 `ctx_patch = cat((ctx_patch,)*4)` + filter):
// a kept parent receives the sum of the gradients of its (up to 4) surviving children, in block order (deterministic).
__global__ void __launch_bounds__(256)
gather_bwd_kernel(const int* __restrict__ keep_idx, int64_t ldk, const int* __restrict__ keep_count,
                  const int* __restrict__ child_pos, const float* __restrict__ d_next, int64_t n_next, int Dp,
                  float* __restrict__ d_cur, int64_t n_cur) {
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  const int count = keep_count[b];
  if (i >= count) return;
  const int row = keep_idx[(int64_t)b * ldk + i];
  int pos[4];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) pos[blk] = child_pos[(int64_t)b * 4 * ldk + blk * count + i];
  f32x4* out = reinterpret_cast<f32x4*>(d_cur + ((int64_t)b * n_cur + row) * Dp);
  for (int c = tid; c < Dp / 4; c += 256) {
    f32x4 s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
      if (pos[blk] >= 0) s += reinterpret_cast<const f32x4*>(d_next + ((int64_t)b * n_next + pos[blk]) * Dp)[c];
    out[c] = s;
  }
}

// The same sum with separate row strides, an optional compact destination (keep_idx == nullptr: kept slot i -> row i) and a column
// window: dst[b, row(i), 0:width] (+)= sum over the surviving children of kept parent i of src[b, child, 0:width].  The training
// step's once-per-parent form: dHP = sum of the children's gate-pre-activation gradients (compact table), dc_parent = sum of dc0.
__global__ void __launch_bounds__(256)
sibling_sum_kernel(const int* __restrict__ keep_idx, int64_t ldk, const int* __restrict__ keep_count, const int* __restrict__ child_pos,
                   const float* __restrict__ src, int64_t n_src, int64_t ld_src, int width, float* __restrict__ dst, int64_t n_dst,
                   int64_t ld_dst) {
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  const int count = keep_count[b];
  if (i >= count) return;
  const int row = keep_idx ? keep_idx[(int64_t)b * ldk + i] : i;
  int pos[4];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) pos[blk] = child_pos[(int64_t)b * 4 * ldk + blk * count + i];
  f32x4* out = reinterpret_cast<f32x4*>(dst + ((int64_t)b * n_dst + row) * ld_dst);
  for (int c = tid; c < width / 4; c += 256) {
    f32x4 s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
      if (pos[blk] >= 0) s += reinterpret_cast<const f32x4*>(src + ((int64_t)b * n_src + pos[blk]) * ld_src)[c];
    out[c] = s;
  }
}

// dst[b, keep_idx[b, i], 0:width] = src[b, i, 0:width] for i < keep_count[b] (the kept parents' h gradient back into the level's state gradient)
__global__ void __launch_bounds__(256)
scatter_kept_rows_kernel(const float* __restrict__ src, int64_t ldk, int64_t ld_src, const int* __restrict__ keep_idx,
                         const int* __restrict__ keep_count, float* __restrict__ dst, int64_t n_dst, int64_t ld_dst, int width) {
  const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
  if (i >= keep_count[b]) return;
  const int row = keep_idx[(int64_t)b * ldk + i];
  const f32x4* in = reinterpret_cast<const f32x4*>(src + ((int64_t)b * ldk + i) * ld_src);
  f32x4* out = reinterpret_cast<f32x4*>(dst + ((int64_t)b * n_dst + row) * ld_dst);
  for (int c = tid; c < width / 4; c += 256) out[c] = in[c];
}

// Level 0: every grid cell, row-major, no background filter (slide.py:257-269).  PACKED: as in gather_kernel.
template <class T, bool PACKED = false>
__global__ void __launch_bounds__(256)
level0_kernel(const int64_t* __restrict__ grid_ptrs, const int* __restrict__ gx, const int* __restrict__ gy, int D,
              int patch_size, int64_t n0, float* __restrict__ fts, int64_t* __restrict__ locs,
              int64_t* __restrict__ parent, int64_t* __restrict__ num_ims, int zero_pad,
              int64_t* __restrict__ row_ptrs, const float* __restrict__ zero_row, const int64_t* __restrict__ index_ptrs = nullptr) {
  const int b = blockIdx.y;
  const int64_t j = blockIdx.x;
  const int X = gx[b], Y = gy[b];
  const int64_t n = (int64_t)X * Y;
  const int64_t o = (int64_t)b * n0 + j;
  const int tid = threadIdx.x;
  f32x4* fo = fts ? reinterpret_cast<f32x4*>(fts + o * D) : nullptr;
  if (j == 0 && tid == 0) num_ims[b] = n;
  if (j < n) {
    int64_t row = j;
    if constexpr (PACKED) row = reinterpret_cast<const int*>(index_ptrs[b])[j];
    const bool stored = !PACKED || row >= 0;
    const T* fi = reinterpret_cast<const T*>(grid_ptrs[b]) + row * D;
    if (fo) {
      if (stored) { for (int i = tid; i < D / 4; i += 256) fo[i] = load4(fi, i); }
      else { const f32x4 z{0.f, 0.f, 0.f, 0.f}; for (int i = tid; i < D / 4; i += 256) fo[i] = z; }
    }
    if (tid == 0) {
      locs[2 * o] = (j / Y) * patch_size; locs[2 * o + 1] = (j % Y) * patch_size; parent[o] = j;
      if (row_ptrs) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(stored ? reinterpret_cast<const void*>(fi) : reinterpret_cast<const void*>(zero_row));
    }
  } else {
    if (fo && zero_pad) { const f32x4 z{0.f, 0.f, 0.f, 0.f}; for (int i = tid; i < D / 4; i += 256) fo[i] = z; }
    if (tid == 0) {
      locs[2 * o] = 0; locs[2 * o + 1] = 0; parent[o] = 0;
      if (row_ptrs) row_ptrs[o] = (int64_t)reinterpret_cast<uintptr_t>(zero_row);
    }
  }
}

// tissue mask: 1 iff the row's fp32 sum != 0 (slide.py:324 `fts[...].sum(dim=1) != 0`); one wave per cell.
// With absmax_bits (optional) also max|x| of the whole grid (fp16-split range contract of the default GEMM mode: |x| * a_scale must stay a finite
// fp16).  absmax_bits holds the fp32 BIT PATTERN of the running maximum: non-negative floats order like their bit patterns and a
// NaN's pattern is above +inf's, so a NaN anywhere reads back as "not finite".  The atomic is only issued by waves that beat the
// value they last saw, i.e. a handful of times per grid.
template <class T>
__global__ void __launch_bounds__(256)
tissue_mask_absmax_kernel(const T* __restrict__ grid, int64_t cells, int D, uint8_t* __restrict__ mask, unsigned* __restrict__ absmax_bits) {
  const int lane = threadIdx.x & 63;
  const int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= cells) return;
  const T* row = grid + cell * D;
  float s = 0.f;
  unsigned m = 0;
  for (int i = lane; i < D / 4; i += 64) {
    const f32x4 v = load4(row, i);
    s += (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int e = 0; e < 4; ++e) m = max(m, __float_as_uint(v[e]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { s += __shfl_xor(s, o); m = max(m, (unsigned)__shfl_xor((int)m, o)); }
  if (lane == 0) {
    if (mask) mask[cell] = s != 0.f ? 1 : 0;
    if (absmax_bits && m > __hip_atomic_load(absmax_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(absmax_bits, m);
  }
}

// Z[row] = alpha[row] * X[row] (+ H[row] on valid rows): the non-LSTM hierarchical-context update
// (reference model/paths.py:96-109: Z = Y * alpha; Z += apply_to_non_padded(hctx_mlp, prev Z)).
__global__ void __launch_bounds__(256)
scale_add_rows_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ h,
                      const int64_t* __restrict__ num_ims, int rows_per_slide, int D, int64_t M, int use_alpha,
                      float* __restrict__ z) {
  const int64_t row = blockIdx.x;
  if (row >= M) return;
  const int b = (int)(row / rows_per_slide), idx = (int)(row % rows_per_slide);
  const bool valid = idx < (int)num_ims[b];
  const float a = use_alpha ? alpha[row] : 1.0f;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + row * D);
  const f32x4* hr = h ? reinterpret_cast<const f32x4*>(h + row * D) : nullptr;
  f32x4* zr = reinterpret_cast<f32x4*>(z + row * D);
  for (int i = threadIdx.x; i < D / 4; i += 256) {
    f32x4 v = xr[i] * a;
    if (hr && valid) v += hr[i];
    zr[i] = v;
  }
}

// Synthetic grid (paths_amd/synthetic.py): one thread per 4 channels.  fp16 grids: the fp32 values rounded to nearest even.
template <class T>
__global__ void __launch_bounds__(256)
synth_grid_kernel(T* __restrict__ grid, int X, int Y, int D, uint32_t k2, int level, unsigned long long bg_thr) {
  const int64_t cell = blockIdx.x;
  const int x = (int)(cell / Y), y = (int)(cell % Y);
  const uint32_t k3 = fmix32(k2 + (uint32_t)x * 0xC2B2AE3Du);
  const uint32_t ck = fmix32(k3 + (uint32_t)y * 0x27D4EB2Fu);
  const bool bg = level >= 1 && (unsigned long long)fmix32(ck ^ 0xB6B6B6B6u) < bg_thr;
  for (int c4 = threadIdx.x; c4 < D / 4; c4 += 256) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t u = fmix32(ck + (uint32_t)(4 * c4 + e) * 0x165667B1u + 0x9E3779B9u);
      const float f = ((float)(u >> 8) * 0x1p-23f - 1.0f) * 1.7320508075688772f;
      v[e] = bg ? 0.f : f;
    }
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4*>(grid + cell * D + 4 * c4) = v;
    } else {
      // round the fp32 VALUES (the host replica's double step): without the barrier the last multiply and the conversion fuse into
      // one mixed-precision FMA that rounds the exact product to fp16 once - 1 ulp apart from fp32-then-fp16 in rare cases
      asm volatile("" : "+v"(v));
      *reinterpret_cast<f16x4*>(grid + cell * D + 4 * c4) = f16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
    }
  }
}

// THE host launchers of the two address-forming kernels, behind paths_gather_rows[_packed][_h16] / paths_level0_batch[_packed][_h16]
// (`what`: the entry point's name in messages).  PACKED: grid_ptrs[b] = the slide's first packed row, index_ptrs[b] -> int32 [X*Y] (row
// of a cell or -1); a cell without a stored row gives zero_row in row_ptrs and zeros in the copy.  Dense: index_ptrs is null.
template <class T, bool PACKED>
int launch_gather(const char* what, const int64_t* grid_ptrs, const int64_t* index_ptrs, const int* src_cell, int D, const float* state_cur,
                  int64_t n_cur, int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                  float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_next > 0 && D % 4 == 0 && Dp % 4 == 0 && ld_state_cur % 4 == 0, "%s: bad shape", what);
  PATHS_REQUIRE(grid_ptrs != nullptr && (!PACKED || index_ptrs != nullptr) && src_cell != nullptr && num_out != nullptr, "%s: null pointer", what);
  PATHS_REQUIRE(fts_out != nullptr || row_ptrs != nullptr, "%s: features must go somewhere (a copy or row pointers)", what);
  PATHS_REQUIRE(row_ptrs == nullptr || zero_row != nullptr, "%s: row_ptrs needs a zero row for padding and dropped rows", what);
  PATHS_REQUIRE((state_cur == nullptr) == (state_out == nullptr), "%s: state in/out must both be given or null", what);
  hipLaunchKernelGGL((gather_kernel<T, PACKED>), dim3((unsigned)((n_next + GATHER_ROWS - 1) / GATHER_ROWS), B), dim3(256), 0, stream, grid_ptrs, src_cell, D,
                     state_cur, n_cur, ld_state_cur, src_row, Dp, num_out, n_next, fts_out, state_out, zero_pad, row_ptrs, zero_row, index_ptrs);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

template <class T, bool PACKED>
int launch_level0(const char* what, const int64_t* grid_ptrs, const int64_t* index_ptrs, const int* gx, const int* gy, int B, int D, int patch_size,
                  int64_t n0, float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                  const float* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n0 > 0 && D % 4 == 0, "%s: bad shape", what);
  PATHS_REQUIRE(grid_ptrs != nullptr && (!PACKED || index_ptrs != nullptr) && gx != nullptr && gy != nullptr, "%s: null pointer", what);
  PATHS_REQUIRE((fts != nullptr || row_ptrs != nullptr) && (row_ptrs == nullptr || zero_row != nullptr), "%s: features need a destination (copy or row pointers + zero row)", what);
  hipLaunchKernelGGL((level0_kernel<T, PACKED>), dim3((unsigned)n0, B), dim3(256), 0, stream, grid_ptrs, gx, gy, D, patch_size, n0,
                     fts, locs, parent, num_ims, zero_pad, row_ptrs, zero_row, index_ptrs);
  PATHS_LAUNCH_CHECK(what);
  return PATHS_OK;
}

}  // namespace

extern "C" {

int paths_topk(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
               int* keep_idx, int64_t ldk, int* keep_count, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_max > 0 && n_max <= TOPK_MAX, "topk: n_max (%d) must be in [1, %d]", n_max, TOPK_MAX);
  PATHS_REQUIRE(keep == -1 || keep > 0, "topk: keep must be -1 (all) or > 0");
  PATHS_REQUIRE(ldk >= (keep < 0 ? n_max : (keep < n_max ? keep : n_max)), "topk: keep_idx row too short");
  PATHS_REQUIRE(ldk <= TOPK_MAX, "topk: keep_idx row longer than %d", TOPK_MAX);
  launch_topk(scores, ld, num_ims, B, n_max, keep, keep_idx, ldk, keep_count, nullptr, 0, 0, nullptr, nullptr, stream);
  PATHS_LAUNCH_CHECK("topk");
  return PATHS_OK;
}

// paths_topk + the ADDRESS of every kept row of a row-major [B, slide_rows, row_ld] table (kept_rows [B, ldk]; entries beyond a
// slide's keep_count point at zero_row): the once-per-parent GEMM reads the kept parents' h rows through them, in place.
int paths_topk_rows(const float* scores, int64_t ld, const int64_t* num_ims, int B, int n_max, int keep,
                    int* keep_idx, int64_t ldk, int* keep_count, const float* row_base, int64_t row_ld, int64_t slide_rows,
                    int64_t* kept_rows, const float* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_max > 0 && n_max <= TOPK_MAX, "topk_rows: n_max (%d) must be in [1, %d]", n_max, TOPK_MAX);
  PATHS_REQUIRE(keep == -1 || keep > 0, "topk_rows: keep must be -1 (all) or > 0");
  PATHS_REQUIRE(ldk >= (keep < 0 ? n_max : (keep < n_max ? keep : n_max)), "topk_rows: keep_idx row too short");
  PATHS_REQUIRE(row_base && kept_rows && zero_row && row_ld > 0 && slide_rows >= n_max, "topk_rows: row table arguments");
  PATHS_REQUIRE(ldk <= TOPK_MAX, "topk_rows: keep_idx row longer than %d", TOPK_MAX);
  launch_topk(scores, ld, num_ims, B, n_max, keep, keep_idx, ldk, keep_count, row_base, row_ld, slide_rows, kept_rows, zero_row, stream);
  PATHS_LAUNCH_CHECK("topk_rows");
  return PATHS_OK;
}

int paths_expand_children(const int* keep_idx, int64_t ldk, const int* keep_count, const int64_t* locs, int64_t n_cur,
                          int patch_size, const int* next_x, const int* next_y, const int64_t* mask_ptrs, int B,
                          int64_t n_next, int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row,
                          int* src_cell, int* status, int* child_pos, int* hp_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_cur > 0 && n_next > 0 && patch_size > 0 && ldk > 0, "expand_children: bad shape");
  PATHS_REQUIRE(4 * ldk <= (int64_t)1 << 30, "expand_children: too many candidates");
  PATHS_REQUIRE(keep_idx && keep_count && locs && next_x && next_y && mask_ptrs && num_out && locs_out && parent_out && src_row &&
                src_cell && status, "expand_children: null pointer");
  hipLaunchKernelGGL(expand_kernel, dim3(B), dim3(EXP_NT), 0, stream, keep_idx, ldk, keep_count, locs, n_cur, patch_size,
                     next_x, next_y, mask_ptrs, n_next, num_out, locs_out, parent_out, src_row, src_cell, status, child_pos, hp_row);
  PATHS_LAUNCH_CHECK("expand_children");
  return PATHS_OK;
}

int paths_candidate_children(const int* keep_idx, int64_t ldk, const int* keep_count, const int64_t* locs, int64_t n_cur,
                             int patch_size, const int* next_x, const int* next_y, int B, int* cand_count, int64_t* cand_cells,
                             int* cand_slot, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_cur > 0 && patch_size > 0 && ldk > 0, "candidate_children: bad shape");
  PATHS_REQUIRE(4 * ldk <= (int64_t)1 << 30, "candidate_children: too many candidates");
  PATHS_REQUIRE(keep_idx && keep_count && locs && next_x && next_y && cand_count && cand_cells && cand_slot, "candidate_children: null pointer");
  hipLaunchKernelGGL(candidate_kernel, dim3(B), dim3(EXP_NT), 0, stream, keep_idx, ldk, keep_count, locs, n_cur, patch_size, next_x,
                     next_y, cand_count, cand_cells, cand_slot);
  PATHS_LAUNCH_CHECK("candidate_children");
  return PATHS_OK;
}

int paths_admit_children(const int* cand_count, const int64_t* cand_cells, const int* cand_slot, const uint8_t* cand_mask,
                         const int* keep_idx, int64_t ldk, const int* keep_count, int patch_size, int B, int64_t n_next,
                         int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row, int* src_cell, int* status,
                         int* child_pos, int* hp_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_next > 0 && patch_size > 0 && ldk > 0, "admit_children: bad shape");
  PATHS_REQUIRE(4 * ldk <= (int64_t)1 << 30, "admit_children: too many candidates");
  PATHS_REQUIRE(cand_count && cand_cells && cand_slot && cand_mask && keep_idx && keep_count && num_out && locs_out && parent_out &&
                src_row && src_cell && status, "admit_children: null pointer");
  hipLaunchKernelGGL(admit_kernel, dim3(B), dim3(EXP_NT), 0, stream, cand_count, cand_cells, cand_slot, cand_mask, keep_idx, ldk,
                     keep_count, patch_size, n_next, num_out, locs_out, parent_out, src_row, src_cell, status, child_pos, hp_row);
  PATHS_LAUNCH_CHECK("admit_children");
  return PATHS_OK;
}

int paths_fallback_all_cells(const int* next_x, const int* next_y, const int64_t* mask_ptrs, int patch_size, int B,
                             int64_t n_next, int64_t* num_out, int64_t* locs_out, int64_t* parent_out, int* src_row,
                             int* src_cell, int* status, int* hp_row, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && n_next > 0 && patch_size > 0, "fallback_all_cells: bad shape");
  PATHS_REQUIRE(next_x && next_y && mask_ptrs && num_out && locs_out && parent_out && src_row && src_cell && status,
                "fallback_all_cells: null pointer");
  hipLaunchKernelGGL(fallback_all_cells_kernel, dim3(B), dim3(1024), 0, stream, next_x, next_y, mask_ptrs, patch_size, n_next,
                     num_out, locs_out, parent_out, src_row, src_cell, status, hp_row);
  PATHS_LAUNCH_CHECK("fallback_all_cells");
  return PATHS_OK;
}

int paths_gather_rows(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                      int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                      float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                      hipStream_t stream) {
  return launch_gather<float, false>("gather_rows", grid_ptrs, nullptr, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp, num_out, B, n_next,
                                     fts_out, state_out, zero_pad, row_ptrs, zero_row, stream);
}

// paths_gather_rows over FP16 grids: row_ptrs address fp16 rows, fts_out (if given) receives fp32 copies.  zero_row: D floats of zero
// (valid padding for either row width).
int paths_gather_rows_h16(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                          int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                          float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                          hipStream_t stream) {
  return launch_gather<_Float16, false>("gather_rows_h16", grid_ptrs, nullptr, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp, num_out, B,
                                        n_next, fts_out, state_out, zero_pad, row_ptrs, zero_row, stream);
}

// paths_gather_rows[_h16] over PACKED slides (tissue-only storage, pack_rows.hip): index_ptrs, the cell-index table, in front of the stream
int paths_gather_rows_packed(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                             int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                             float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                             const int64_t* index_ptrs, hipStream_t stream) {
  return launch_gather<float, true>("gather_rows_packed", grid_ptrs, index_ptrs, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp, num_out,
                                    B, n_next, fts_out, state_out, zero_pad, row_ptrs, zero_row, stream);
}

int paths_gather_rows_packed_h16(const int64_t* grid_ptrs, const int* src_cell, int D, const float* state_cur, int64_t n_cur,
                                 int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                                 float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row,
                                 const int64_t* index_ptrs, hipStream_t stream) {
  return launch_gather<_Float16, true>("gather_rows_packed_h16", grid_ptrs, index_ptrs, src_cell, D, state_cur, n_cur, ld_state_cur, src_row, Dp,
                                       num_out, B, n_next, fts_out, state_out, zero_pad, row_ptrs, zero_row, stream);
}

// d_cur [B, n_cur, Dp] must be zero-initialised (rows that were not kept receive no gradient).
int paths_gather_kept_rows(const float* src, int64_t n_cur, int64_t ld_src, const int* keep_idx, int64_t ldk, const int* keep_count,
                           int D, int B, float* out, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && ldk > 0 && D % 4 == 0 && ld_src % 4 == 0 && src && keep_idx && keep_count && out, "gather_kept_rows: bad arguments");
  hipLaunchKernelGGL(gather_kept_rows_kernel, dim3((unsigned)ldk, B), dim3(256), 0, stream, src, n_cur, ld_src, keep_idx, ldk, keep_count, D, out);
  PATHS_LAUNCH_CHECK("gather_kept_rows");
  return PATHS_OK;
}

int paths_gather_rows_bwd(const int* keep_idx, int64_t ldk, const int* keep_count, const int* child_pos, const float* d_next,
                          int64_t n_next, int Dp, float* d_cur, int64_t n_cur, int B, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && ldk > 0 && Dp % 4 == 0 && keep_idx && keep_count && child_pos && d_next && d_cur, "gather_rows_bwd: bad arguments");
  hipLaunchKernelGGL(gather_bwd_kernel, dim3((unsigned)ldk, B), dim3(256), 0, stream, keep_idx, ldk, keep_count, child_pos, d_next, n_next, Dp, d_cur, n_cur);
  PATHS_LAUNCH_CHECK("gather_rows_bwd");
  return PATHS_OK;
}

int paths_sibling_sum(const int* keep_idx, int64_t ldk, const int* keep_count, const int* child_pos, const float* src, int64_t n_src,
                      int64_t ld_src, int width, float* dst, int64_t n_dst, int64_t ld_dst, int B, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && ldk > 0 && width > 0 && width % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && keep_count && child_pos && src && dst,
                "sibling_sum: bad arguments");
  PATHS_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "sibling_sum: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(sibling_sum_kernel, dim3((unsigned)ldk, B), dim3(256), 0, stream, keep_idx, ldk, keep_count, child_pos, src, n_src, ld_src,
                     width, dst, n_dst, ld_dst);
  PATHS_LAUNCH_CHECK("sibling_sum");
  return PATHS_OK;
}

int paths_scatter_kept_rows(const float* src, int64_t ldk, int64_t ld_src, const int* keep_idx, const int* keep_count, float* dst,
                            int64_t n_dst, int64_t ld_dst, int width, int B, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && ldk > 0 && width > 0 && width % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 && keep_idx && keep_count && src && dst,
                "scatter_kept_rows: bad arguments");
  PATHS_REQUIRE(((uintptr_t)src | (uintptr_t)dst) % 16 == 0, "scatter_kept_rows: buffers must be 16-byte aligned");
  hipLaunchKernelGGL(scatter_kept_rows_kernel, dim3((unsigned)ldk, B), dim3(256), 0, stream, src, ldk, ld_src, keep_idx, keep_count, dst, n_dst,
                     ld_dst, width);
  PATHS_LAUNCH_CHECK("scatter_kept_rows");
  return PATHS_OK;
}

int paths_level0_batch(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                       float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                       const float* zero_row, hipStream_t stream) {
  return launch_level0<float, false>("level0_batch", grid_ptrs, nullptr, gx, gy, B, D, patch_size, n0, fts, locs, parent, num_ims, zero_pad, row_ptrs,
                                     zero_row, stream);
}

// paths_level0_batch over FP16 grids (row_ptrs address fp16 rows; fts receives fp32 copies)
int paths_level0_batch_h16(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                           float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                           const float* zero_row, hipStream_t stream) {
  return launch_level0<_Float16, false>("level0_batch_h16", grid_ptrs, nullptr, gx, gy, B, D, patch_size, n0, fts, locs, parent, num_ims, zero_pad,
                                        row_ptrs, zero_row, stream);
}

// paths_level0_batch[_h16] over PACKED slides: index_ptrs in front of the stream
int paths_level0_batch_packed(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                              float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                              const float* zero_row, const int64_t* index_ptrs, hipStream_t stream) {
  return launch_level0<float, true>("level0_batch_packed", grid_ptrs, index_ptrs, gx, gy, B, D, patch_size, n0, fts, locs, parent, num_ims, zero_pad,
                                    row_ptrs, zero_row, stream);
}

int paths_level0_batch_packed_h16(const int64_t* grid_ptrs, const int* gx, const int* gy, int B, int D, int patch_size, int64_t n0,
                                  float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad, int64_t* row_ptrs,
                                  const float* zero_row, const int64_t* index_ptrs, hipStream_t stream) {
  return launch_level0<_Float16, true>("level0_batch_packed_h16", grid_ptrs, index_ptrs, gx, gy, B, D, patch_size, n0, fts, locs, parent, num_ims,
                                       zero_pad, row_ptrs, zero_row, stream);
}

int paths_scale_add_rows(const float* x, const float* alpha, const float* h, const int64_t* num_ims, int rows_per_slide,
                         int D, int64_t M, int use_alpha, float* z, hipStream_t stream) {
  PATHS_REQUIRE(M > 0 && D % 4 == 0 && rows_per_slide > 0 && num_ims && x && z && (alpha || !use_alpha), "scale_add_rows: bad arguments");
  hipLaunchKernelGGL(scale_add_rows_kernel, dim3((unsigned)M), dim3(256), 0, stream, x, alpha, h, num_ims, rows_per_slide, D, M, use_alpha, z);
  PATHS_LAUNCH_CHECK("scale_add_rows");
  return PATHS_OK;
}

int paths_tissue_mask(const float* grid, int64_t cells, int D, uint8_t* mask, hipStream_t stream) {
  PATHS_REQUIRE(cells > 0 && D % 4 == 0, "tissue_mask: bad shape");
  hipLaunchKernelGGL(tissue_mask_absmax_kernel<float>, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, stream, grid, cells, D, mask,
                     (unsigned*)nullptr);
  PATHS_LAUNCH_CHECK("tissue_mask");
  return PATHS_OK;
}

int paths_tissue_mask_absmax(const float* grid, int64_t cells, int D, uint8_t* mask, uint32_t* absmax_bits, hipStream_t stream) {
  PATHS_REQUIRE(cells > 0 && D % 4 == 0 && absmax_bits != nullptr, "tissue_mask_absmax: bad arguments");
  hipLaunchKernelGGL(tissue_mask_absmax_kernel<float>, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, stream, grid, cells, D, mask, absmax_bits);
  PATHS_LAUNCH_CHECK("tissue_mask_absmax");
  return PATHS_OK;
}

// the same pass over an FP16 grid (grid: [cells, D] fp16; sums and max|x| in fp32, identical to the fp32 grid of the same values)
int paths_tissue_mask_absmax_h16(const void* grid, int64_t cells, int D, uint8_t* mask, uint32_t* absmax_bits, hipStream_t stream) {
  PATHS_REQUIRE(cells > 0 && D % 4 == 0 && absmax_bits != nullptr, "tissue_mask_absmax_h16: bad arguments");
  hipLaunchKernelGGL(tissue_mask_absmax_kernel<_Float16>, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, stream,
                     reinterpret_cast<const _Float16*>(grid), cells, D, mask, absmax_bits);
  PATHS_LAUNCH_CHECK("tissue_mask_absmax_h16");
  return PATHS_OK;
}

int paths_synth_grid(float* grid, int X, int Y, int D, uint32_t slide_level_key, int level, uint64_t bg_threshold, hipStream_t stream) {
  PATHS_REQUIRE(X > 0 && Y > 0 && D % 4 == 0 && (int64_t)X * Y < ((int64_t)1 << 31), "synth_grid: bad shape");
  hipLaunchKernelGGL(synth_grid_kernel<float>, dim3((unsigned)((int64_t)X * Y)), dim3(256), 0, stream, grid, X, Y, D, slide_level_key, level, (unsigned long long)bg_threshold);
  PATHS_LAUNCH_CHECK("synth_grid");
  return PATHS_OK;
}

// paths_synth_grid into an FP16 grid: the same values rounded to nearest even (synthetic.SyntheticSlide feature_dtype "float16")
int paths_synth_grid_h16(void* grid, int X, int Y, int D, uint32_t slide_level_key, int level, uint64_t bg_threshold, hipStream_t stream) {
  PATHS_REQUIRE(X > 0 && Y > 0 && D % 4 == 0 && (int64_t)X * Y < ((int64_t)1 << 31), "synth_grid_h16: bad shape");
  hipLaunchKernelGGL(synth_grid_kernel<_Float16>, dim3((unsigned)((int64_t)X * Y)), dim3(256), 0, stream, reinterpret_cast<_Float16*>(grid), X, Y, D,
                     slide_level_key, level, (unsigned long long)bg_threshold);
  PATHS_LAUNCH_CHECK("synth_grid_h16");
  return PATHS_OK;
}

}  // extern "C"
