// From decoded pixels to encoder input and back to feature rows (paths_amd/pixels.py; include/paths_hip.h: paths_grey_histogram,
// paths_tile_tissue, paths_tile_compact, paths_tiles_to_input, paths_scatter_rows; contract tests/tiles_ref.py, bit for bit).
// Everything here is integer or table work at memory rate: the grey value is an integer dot product, the tissue decision compares
// integers, the encoder input is a 768-entry table lookup (the table is built on the host with torch, so the kernel is torch's result
// by construction) and the scatter copies rows with at most one cast.  No global atomics, no float arithmetic: reruns are bit-identical.
//
// Images and tiles are named by device tables of addresses.  What keeps every access inside its buffer whatever a table holds is the
// caller's table; what the kernels add is that an entry breaking the stated rules (address or stride not a multiple of 16, a stride
// shorter than the row) is never followed, and that an index read from `order` or `slot` is used only inside its range.
#include "common.h"
#include "tile_pieces.h"

namespace {

constexpr int TT = 256;                       // threads of the histogram, tissue and input workgroups
constexpr int TW = TT / 64;
constexpr int CT = 1024;                      // threads of the one compaction workgroup
constexpr int IN_ROUNDS = 4;                  // 16-pixel pieces per thread of the input kernel, all loaded before the first store
static_assert(PATHS_TILES_MAX % CT == 0 && PATHS_TILES_MAX / CT <= 64, "a thread of the compaction owns at most 64 flags");

// ---- histogram: workgroup (x, img) counts rows x, x + PATHS_HIST_BLOCKS, .. of image img, one count table per wave in LDS
__global__ void __launch_bounds__(TT)
grey_hist_kernel(const int64_t* __restrict__ images, int n_images, uint32_t* __restrict__ partials) {
  __shared__ unsigned int h[TW][256];
  const int tid = threadIdx.x, wave = tid >> 6, img = blockIdx.y;
  for (int i = tid; i < TW * 256; i += TT) (&h[0][0])[i] = 0;
  __syncthreads();
  const int64_t addr = images[4 * img], stride = images[4 * img + 1], rows = images[4 * img + 2], cols = images[4 * img + 3];
  const bool ok = rows > 0 && cols > 0 && rows * cols < (1ll << 31) && entry_ok(addr, stride, 3 * cols);     // (uniform over the workgroup)
  if (blockIdx.x == 0 && tid == 0) partials[(int64_t)n_images * PATHS_HIST_BLOCKS * 256 + img] = ok ? 0u : 1u;   // a refused entry: reported
  if (ok) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(addr));
    const int64_t pieces = (cols + 15) / 16;
    unsigned int* mine = h[wave];
    for (int64_t row = blockIdx.x; row < rows; row += PATHS_HIST_BLOCKS) {
      const unsigned char* r = base + row * stride;
      for (int64_t pc = tid; pc < pieces; pc += TT) {
        const int64_t c0 = pc * 16;
        if (c0 + 16 <= cols) {
          Piece p;
          p.load(r + 3 * c0);
          int prev = p.grey_of(0), run = 1;                       // equal neighbours (background) share one LDS add
#pragma unroll
          for (int px = 1; px < 16; ++px) {
            const int g = p.grey_of(px);
            if (g == prev) { ++run; } else { atomicAdd(mine + prev, (unsigned int)run); prev = g; run = 1; }
          }
          atomicAdd(mine + prev, (unsigned int)run);
        } else {                                                  // the ragged end of a row: byte loads, nothing behind cols * 3
          for (int64_t c = c0; c < cols; ++c) atomicAdd(mine + grey_at(r + 3 * c), 1u);
        }
      }
    }
  }
  __syncthreads();
  unsigned int s = 0;
#pragma unroll
  for (int w = 0; w < TW; ++w) s += h[w][tid];
  partials[((int64_t)img * PATHS_HIST_BLOCKS + blockIdx.x) * 256 + tid] = s;
}

__global__ void __launch_bounds__(256)
grey_hist_sum_kernel(const uint32_t* __restrict__ partials, int n_images, int64_t* __restrict__ counts, int* __restrict__ status) {
  const int parts = n_images * PATHS_HIST_BLOCKS;
  int64_t s = 0;
  for (int p = 0; p < parts; ++p) s += partials[(int64_t)p * 256 + threadIdx.x];
  counts[threadIdx.x] = s;
  if (threadIdx.x == 0) {
    unsigned int refused = 0;
    for (int i = 0; i < n_images; ++i) refused |= partials[(int64_t)parts * 256 + i];
    status[0] = refused ? 1 : 0;
  }
}

// ---- tissue: one workgroup per tile.  S > 0: the stride divides 16, a thread takes the 16 / S lattice pixels of a 16-pixel piece of a
// lattice row from three 16-byte loads; S = 0: any other stride, one lattice pixel per thread and step from byte loads.
template <int S>
__global__ void __launch_bounds__(TT)
tile_tissue_kernel(const int64_t* __restrict__ tiles, int P, int stride, int threshold, int pass_count, int* __restrict__ counts,
                   uint8_t* __restrict__ flags) {
  __shared__ int part[TW];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int64_t addr = tiles[2 * (int64_t)k], rs = tiles[2 * (int64_t)k + 1];
  if (!entry_ok(addr, rs, 3 * (int64_t)P)) {                       // (uniform) a refused entry is never followed
    if (tid == 0) { counts[k] = -1; flags[k] = 0; }
    return;
  }
  const unsigned char* base = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(addr));
  const int L = P / stride, half = stride / 2;
  int c = 0;
  if constexpr (S > 0) {
    const int pieces = P / 16, items = L * pieces;
    for (int it = tid; it < items; it += TT) {
      const int i = it / pieces, j = it - i * pieces;
      Piece p;
      p.load(base + (int64_t)(i * S + S / 2) * rs + 48 * j);
#pragma unroll
      for (int q = 0; q < 16 / S; ++q) c += p.grey_of(q * S + S / 2) < threshold ? 1 : 0;
    }
  } else {
    const int items = L * L;
    for (int it = tid; it < items; it += TT) {
      const int i = it / L, j = it - i * L;
      c += grey_at(base + (int64_t)(i * stride + half) * rs + 3 * (j * stride + half)) < threshold ? 1 : 0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  if ((tid & 63) == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < TW; ++w) total += part[w];
    counts[k] = total;
    flags[k] = total >= pass_count ? 1 : 0;
  }
}

// ---- compaction: one workgroup, a contiguous run of flags per thread, positions by an exclusive scan (wave scan by shuffles, then a
// scan of the wave totals: the shape of select.hip:exp_scan)
__global__ void __launch_bounds__(CT)
tile_compact_kernel(const uint8_t* __restrict__ flags, const int* __restrict__ counts, int n, int* __restrict__ order, int* __restrict__ m,
                    int* __restrict__ slot, int* __restrict__ status) {
  constexpr int NW = CT / 64;
  __shared__ int part[2 * NW];
  const int tid = threadIdx.x, per = (n + CT - 1) / CT;
  const int k0 = min(n, tid * per), k1 = min(n, k0 + per);
  int mine = 0, refused = 0;
  for (int k = k0; k < k1; ++k) { mine += flags[k] ? 1 : 0; refused |= counts[k] < 0 ? 1 : 0; }
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off);
    if ((tid & 63) >= off) incl += v;
  }
  if ((tid & 63) == 63) part[tid >> 6] = incl;
  refused = __syncthreads_or(refused);
  if (tid < NW) {
    int t = part[tid];
#pragma unroll
    for (int off = 1; off < NW; off <<= 1) {
      const int v = __shfl_up(t, off);
      if (tid >= off) t += v;
    }
    part[NW + tid] = t;                                            // inclusive totals of waves 0 .. tid
  }
  __syncthreads();
  int pos = incl - mine + ((tid >> 6) ? part[NW + (tid >> 6) - 1] : 0);
  for (int k = k0; k < k1; ++k) {
    if (flags[k]) { order[pos] = k; slot[k] = pos; ++pos; } else { slot[k] = -1; }
  }
  if (tid == 0) { m[0] = part[2 * NW - 1]; status[0] = refused ? 1 : 0; }
}

// ---- encoder input: workgroup (i, y) writes pieces [y * IN_ROUNDS * TT, ..) of tile order[first + i]; piece = (row, 16 pixels)
template <class E>
__global__ void __launch_bounds__(TT)
tiles_to_input_kernel(const int64_t* __restrict__ tiles, int n, const int* __restrict__ order, int first, int P, const E* __restrict__ table,
                      E* __restrict__ out) {
  __shared__ E lut[768];
  const int tid = threadIdx.x;
  for (int i = tid; i < 768; i += TT) lut[i] = table[i];
  __syncthreads();
  const int t = order[first + (int64_t)blockIdx.x];
  int64_t addr = 0, rs = 0;
  if (t >= 0 && t < n) { addr = tiles[2 * (int64_t)t]; rs = tiles[2 * (int64_t)t + 1]; }
  const bool valid = entry_ok(addr, rs, 3 * (int64_t)P);           // (uniform) otherwise the tile reads as zero bytes
  const unsigned char* base = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(addr));
  const int pieces = P / 16, items = P * pieces;
  const int64_t plane = (int64_t)P * P;
  E* o = out + (int64_t)blockIdx.x * 3 * plane;
  const int it0 = blockIdx.y * IN_ROUNDS * TT + tid;
  Piece p[IN_ROUNDS];
#pragma unroll
  for (int r = 0; r < IN_ROUNDS; ++r) {
    const int it = it0 + r * TT;
    p[r].zero();
    if (valid && it < items) {
      const int row = it / pieces, j = it - row * pieces;
      p[r].load(base + (int64_t)row * rs + 48 * j);
    }
  }
#pragma unroll
  for (int r = 0; r < IN_ROUNDS; ++r) {
    const int it = it0 + r * TT;
    if (it >= items) break;
    const int row = it / pieces, j = it - row * pieces;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      E v[16];
#pragma unroll
      for (int px = 0; px < 16; ++px) v[px] = lut[c * 256 + p[r].byte(3 * px + c)];
      store16<E>(o + c * plane + (int64_t)row * P + 16 * j, v);
    }
  }
}

// ---- rows: a unit is four consecutive elements of a row (dim % 4 == 0: never across rows).  fp32 output: one unit = one 16-byte store
// per thread; fp16 output: two units (which may lie in two rows) = one 16-byte store, the odd last unit 8 bytes.
template <bool IN16>
__device__ __forceinline__ f32x4 load_unit(const void* enc, const int* __restrict__ slot, int m, int64_t u, int upr, int dim) {
  const int64_t k = u / upr;
  const int col = (int)(u - k * upr) * 4;
  const int s = slot[k];
  if (s < 0 || s >= m) return f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (IN16) {
    typedef const f16x4 __attribute__((address_space(1))) * gsrc;
    const f16x4 h = *reinterpret_cast<gsrc>(reinterpret_cast<uintptr_t>(reinterpret_cast<const _Float16*>(enc) + (int64_t)s * dim + col));
    return f32x4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
  } else {
    return ldg_f32x4(reinterpret_cast<const float*>(enc) + (int64_t)s * dim + col);
  }
}

__device__ __forceinline__ u32x2 to_half4(f32x4 v) {               // round to nearest even, what a torch / NumPy cast does
  return __builtin_bit_cast(u32x2, f16x4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w});
}

template <bool IN16, bool OUT16>
__global__ void __launch_bounds__(256)
scatter_rows_kernel(const void* __restrict__ enc, int m, const int* __restrict__ slot, int64_t units, int dim, void* __restrict__ out) {
  const int upr = dim / 4;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if constexpr (!OUT16) {
    if (g >= units) return;
    stg_f32x4(reinterpret_cast<float*>(out) + 4 * g, load_unit<IN16>(enc, slot, m, g, upr, dim));
  } else {
    const int64_t u = 2 * g;
    if (u >= units) return;
    const u32x2 a = to_half4(load_unit<IN16>(enc, slot, m, u, upr, dim));
    if (u + 1 < units) {
      const u32x2 b = to_half4(load_unit<IN16>(enc, slot, m, u + 1, upr, dim));
      typedef u32x4 __attribute__((address_space(1))) * gdst;
      *reinterpret_cast<gdst>(reinterpret_cast<uintptr_t>(reinterpret_cast<_Float16*>(out) + 4 * u)) = u32x4{a.x, a.y, b.x, b.y};
    } else {
      typedef u32x2 __attribute__((address_space(1))) * gdst;
      *reinterpret_cast<gdst>(reinterpret_cast<uintptr_t>(reinterpret_cast<_Float16*>(out) + 4 * u)) = a;
    }
  }
}

}  // namespace

extern "C" {

int64_t paths_grey_histogram_workspace(int n_images) {
  return n_images < 1 ? 0 : ((int64_t)n_images * PATHS_HIST_BLOCKS * 256 + n_images) * (int64_t)sizeof(uint32_t);
}

int paths_grey_histogram(const int64_t* images, int n_images, uint32_t* partials, int64_t* counts, int* status, hipStream_t stream) {
  PATHS_REQUIRE(n_images >= 1 && n_images <= PATHS_HIST_MAX_IMAGES, "grey_histogram: n_images = %d is outside [1, %d]", n_images,
                PATHS_HIST_MAX_IMAGES);
  PATHS_REQUIRE(images && partials && counts && status, "grey_histogram: null pointer (every argument is required)");
  PATHS_REQUIRE((uintptr_t)images % 8 == 0 && (uintptr_t)partials % 4 == 0 && (uintptr_t)counts % 8 == 0 && (uintptr_t)status % 4 == 0,
                "grey_histogram: alignment of a table");
  hipLaunchKernelGGL(grey_hist_kernel, dim3(PATHS_HIST_BLOCKS, n_images), dim3(TT), 0, stream, images, n_images, partials);
  PATHS_LAUNCH_CHECK("grey_histogram");
  hipLaunchKernelGGL(grey_hist_sum_kernel, dim3(1), dim3(256), 0, stream, partials, n_images, counts, status);
  PATHS_LAUNCH_CHECK("grey_histogram (sum)");
  return PATHS_OK;
}

int paths_tile_tissue(const int64_t* tiles, int n, int P, int stride, int threshold, int pass_count, int* counts, uint8_t* flags,
                      hipStream_t stream) {
  PATHS_REQUIRE(n >= 1 && n <= PATHS_TILES_MAX, "tile_tissue: n = %d is outside [1, %d]", n, PATHS_TILES_MAX);
  PATHS_REQUIRE(tile_shape_ok(P), "tile_tissue: P = %d must be a multiple of 16 in [16, %d]", P, PATHS_TILE_MAX_P);
  PATHS_REQUIRE(stride >= 1 && stride <= P && P % stride == 0, "tile_tissue: stride = %d must divide P = %d", stride, P);
  PATHS_REQUIRE(threshold >= 0 && threshold <= 256, "tile_tissue: threshold = %d is outside [0, 256]", threshold);
  const int64_t size = (int64_t)(P / stride) * (P / stride);
  PATHS_REQUIRE(pass_count >= 0 && pass_count <= size + 1, "tile_tissue: pass_count = %d is outside [0, %lld]", pass_count, (long long)(size + 1));
  PATHS_REQUIRE(tiles && counts && flags, "tile_tissue: null pointer (every argument is required)");
  PATHS_REQUIRE((uintptr_t)tiles % 8 == 0 && (uintptr_t)counts % 4 == 0, "tile_tissue: alignment of a table");
  const dim3 grid(n), block(TT);
#define PATHS_TISSUE_CASE(S) \
  hipLaunchKernelGGL(tile_tissue_kernel<S>, grid, block, 0, stream, tiles, P, stride, threshold, pass_count, counts, flags)
  switch (stride) {
    case 1: PATHS_TISSUE_CASE(1); break;
    case 2: PATHS_TISSUE_CASE(2); break;
    case 4: PATHS_TISSUE_CASE(4); break;
    case 8: PATHS_TISSUE_CASE(8); break;
    case 16: PATHS_TISSUE_CASE(16); break;
    default: PATHS_TISSUE_CASE(0); break;
  }
#undef PATHS_TISSUE_CASE
  PATHS_LAUNCH_CHECK("tile_tissue");
  return PATHS_OK;
}

int paths_tile_compact(const uint8_t* flags, const int* counts, int n, int* order, int* m, int* slot, int* status, hipStream_t stream) {
  PATHS_REQUIRE(n >= 1 && n <= PATHS_TILES_MAX, "tile_compact: n = %d is outside [1, %d]", n, PATHS_TILES_MAX);
  PATHS_REQUIRE(flags && counts && order && m && slot && status, "tile_compact: null pointer (every argument is required)");
  PATHS_REQUIRE((uintptr_t)counts % 4 == 0 && (uintptr_t)order % 4 == 0 && (uintptr_t)m % 4 == 0 && (uintptr_t)slot % 4 == 0 &&
                (uintptr_t)status % 4 == 0, "tile_compact: alignment of a table");
  hipLaunchKernelGGL(tile_compact_kernel, dim3(1), dim3(CT), 0, stream, flags, counts, n, order, m, slot, status);
  PATHS_LAUNCH_CHECK("tile_compact");
  return PATHS_OK;
}

int paths_tiles_to_input(const int64_t* tiles, int n, const int* order, int first, int count, int P, const void* table, int elem_bytes,
                         void* out, hipStream_t stream) {
  PATHS_REQUIRE(n >= 1 && n <= PATHS_TILES_MAX, "tiles_to_input: n = %d is outside [1, %d]", n, PATHS_TILES_MAX);
  PATHS_REQUIRE(tile_shape_ok(P), "tiles_to_input: P = %d must be a multiple of 16 in [16, %d]", P, PATHS_TILE_MAX_P);
  PATHS_REQUIRE(first >= 0 && count >= 1 && (int64_t)first + count <= n, "tiles_to_input: [first, first + count) = [%d, %lld) is outside [0, %d]",
                first, (long long)first + count, n);
  PATHS_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "tiles_to_input: elem_bytes = %d is neither 2 nor 4", elem_bytes);
  PATHS_REQUIRE(tiles && order && table && out, "tiles_to_input: null pointer (every argument is required)");
  PATHS_REQUIRE((uintptr_t)tiles % 8 == 0 && (uintptr_t)order % 4 == 0 && (uintptr_t)table % elem_bytes == 0 && (uintptr_t)out % 16 == 0,
                "tiles_to_input: alignment (out: 16 bytes)");
  const int items = P * (P / 16);
  const dim3 grid(count, (items + IN_ROUNDS * TT - 1) / (IN_ROUNDS * TT)), block(TT);
  if (elem_bytes == 2)
    hipLaunchKernelGGL(tiles_to_input_kernel<uint16_t>, grid, block, 0, stream, tiles, n, order, first, P,
                       reinterpret_cast<const uint16_t*>(table), reinterpret_cast<uint16_t*>(out));
  else
    hipLaunchKernelGGL(tiles_to_input_kernel<uint32_t>, grid, block, 0, stream, tiles, n, order, first, P,
                       reinterpret_cast<const uint32_t*>(table), reinterpret_cast<uint32_t*>(out));
  PATHS_LAUNCH_CHECK("tiles_to_input");
  return PATHS_OK;
}

int paths_scatter_rows(const void* enc, int enc_f16, int m, const int* slot, int n, int dim, int out_f16, void* out, hipStream_t stream) {
  PATHS_REQUIRE(n >= 1 && n <= PATHS_TILES_MAX, "scatter_rows: n = %d is outside [1, %d]", n, PATHS_TILES_MAX);
  PATHS_REQUIRE(m >= 0 && m <= n, "scatter_rows: m = %d is outside [0, n = %d]", m, n);
  PATHS_REQUIRE(dim >= 4 && dim % 4 == 0 && dim <= (1 << 20), "scatter_rows: dim = %d must be a positive multiple of 4", dim);
  PATHS_REQUIRE(slot && out && (enc || m == 0), "scatter_rows: null pointer (enc may be null only when m = 0)");
  PATHS_REQUIRE((uintptr_t)enc % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)slot % 4 == 0, "scatter_rows: alignment (enc, out: 16 bytes)");
  const int64_t units = (int64_t)n * (dim / 4), threads = out_f16 ? (units + 1) / 2 : units;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
#define PATHS_SCATTER_CASE(I, O) hipLaunchKernelGGL((scatter_rows_kernel<I, O>), grid, block, 0, stream, enc, m, slot, units, dim, out)
  if (enc_f16) { if (out_f16) PATHS_SCATTER_CASE(true, true); else PATHS_SCATTER_CASE(true, false); }
  else         { if (out_f16) PATHS_SCATTER_CASE(false, true); else PATHS_SCATTER_CASE(false, false); }
#undef PATHS_SCATTER_CASE
  PATHS_LAUNCH_CHECK("scatter_rows");
  return PATHS_OK;
}

}  // extern "C"
