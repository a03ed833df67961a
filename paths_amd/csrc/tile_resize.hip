// Resize and centre crop in front of the encoder (paths_amd/pixels.py: encoder_input(resize=...); include/paths_hip.h:
// paths_tiles_resize_to_input; contract tests/resize_ref.py, bit for bit): Pillow's antialiased 8-bit resample - integer
// coefficients of 22 fractional bits, the horizontal pass into a BYTE image, then the vertical pass - of a P x P tile to S x S, the
// C x C centre of it through the [3][256] table.  Integers and a table: no float arithmetic, no atomics, reruns are bit-identical.
//
// A workgroup takes one tile and a band of R output rows:
//   1. the table, the coefficient rows of the C cropped columns and of the band's rows -> LDS;
//   2. the input rows the band needs (rows lo[first row] .. lo[last row] + cnt - 1) and of them the 16-pixel pieces the cropped columns
//      need: three 16-byte loads per piece, de-interleaved into one byte plane per channel in LDS (16-byte LDS stores);
//   3. horizontal pass: a thread owns (channel, cropped column, 8 staged rows): one coefficient read and 8 byte reads per tap,
//      8 bytes written to the plane [rows][C] of horizontal results;
//   4. vertical pass: a thread owns (channel, output row, 8 columns): one 8-byte LDS read and one coefficient (a broadcast) per tap,
//      8 table lookups, 16-byte stores - consecutive lanes write consecutive pieces of out[., c, r, .], whose rows are contiguous.
// The products are 24-bit multiplies (a byte times a coefficient below 2^23 in magnitude: the host checks its tables).
//
// The coefficient tables are device memory the host cannot inspect: cnt is clamped into [0, taps], every source row and column
// into the staged window, the window into the tile and into the LDS the launch sized.  Whatever the tables hold, the kernel reads
// only bytes of the tile's P x 3P window and LDS it wrote.
#include "common.h"
#include "tile_pieces.h"

namespace {

constexpr int RT = 256;                       // threads of a workgroup
constexpr int HROWS = 8;                      // staged rows per thread of the horizontal pass
constexpr int VCOLS = 8;                      // columns per thread of the vertical pass (one 8-byte LDS read per tap)
constexpr int HALF = 1 << 21, BITS = 22;      // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int64_t LDS_TWO_PER_CU = 64 * 1024, LDS_ONE_PER_CU = 160 * 1024;

__host__ __device__ inline int align4(int ints) { return (ints + 3) & ~3; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int to_byte(uint32_t acc) { return clampi((int)acc >> BITS, 0, 255); }      // (>> of an int: arithmetic)
__device__ __forceinline__ uint32_t mac(uint32_t acc, int byte, int k) { return acc + (uint32_t)__mul24(byte, k); }

template <class E>
__global__ void __launch_bounds__(RT)
tiles_resize_kernel(const int64_t* __restrict__ tiles, int n, const int* __restrict__ order, int first, int P, int S, int C, int off, int R,
                    int rows_cap, const int* __restrict__ bounds, const int* __restrict__ coef, int taps, const E* __restrict__ table,
                    E* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  E* lut = reinterpret_cast<E*>(smem);                                        // [3][256]
  int* hb = reinterpret_cast<int*>(smem + 768 * sizeof(E));                   // [C][2]     lo, cnt of the cropped columns
  int* hk = hb + 2 * C;                                                       // [C][taps]
  int* vb = hk + C * taps;                                                    // [R][2]     lo, cnt of the band's rows
  int* vk = vb + align4(2 * R);                                               // [R][taps]
  unsigned char* raw = reinterpret_cast<unsigned char*>(vk + align4(R * taps));   // [3][rows_cap][P]   the staged input rows, planar
  unsigned char* hp = raw + 3 * rows_cap * P;                                 // [3][rows_cap][C]   their horizontal results
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * R, Rb = min(R, C - i0);

  // 1. tables
  for (int i = tid; i < 768; i += RT) lut[i] = table[i];
  for (int i = tid; i < 2 * C; i += RT) hb[i] = bounds[2 * off + i];
  for (int i = tid; i < C * taps; i += RT) hk[i] = coef[off * taps + i];
  for (int i = tid; i < 2 * Rb; i += RT) vb[i] = bounds[2 * (off + i0) + i];
  for (int i = tid; i < Rb * taps; i += RT) vk[i] = coef[(off + i0) * taps + i];

  // the staged window (uniform): rows [r_lo, r_lo + nrows) of the tile, columns [x0, x1) in whole 16-pixel pieces
  const int last_r = off + i0 + Rb - 1, last_c = off + C - 1;
  const int r_lo = clampi(bounds[2 * (off + i0)], 0, P - 1);
  const int nrows = min(clampi(bounds[2 * last_r] + clampi(bounds[2 * last_r + 1], 0, taps), r_lo + 1, P) - r_lo, rows_cap);
  const int c_lo = clampi(bounds[2 * off], 0, P - 1);
  const int c_hi = clampi(bounds[2 * last_c] + clampi(bounds[2 * last_c + 1], 0, taps), c_lo + 1, P);
  const int p0 = c_lo >> 4, np = ((c_hi + 15) >> 4) - p0, x0 = 16 * p0, x1 = x0 + 16 * np;

  // 2. stage
  const int t = order[first + (int64_t)blockIdx.x];
  int64_t addr = 0, rs = 0;
  if (t >= 0 && t < n) { addr = tiles[2 * (int64_t)t]; rs = tiles[2 * (int64_t)t + 1]; }
  const bool valid = entry_ok(addr, rs, 3 * (int64_t)P);            // (uniform) otherwise the tile reads as zero bytes
  const unsigned char* base = reinterpret_cast<const unsigned char*>(static_cast<uintptr_t>(addr));
  for (int it = tid; it < nrows * np; it += RT) {
    const int row = it / np, pj = p0 + it - row * np;
    Piece p;
    if (valid) p.load(base + (int64_t)(r_lo + row) * rs + 48 * pj); else p.zero();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      u32x4 d;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        d[q] = (uint32_t)p.byte(12 * q + c) | (uint32_t)p.byte(12 * q + 3 + c) << 8 | (uint32_t)p.byte(12 * q + 6 + c) << 16 |
               (uint32_t)p.byte(12 * q + 9 + c) << 24;
      *reinterpret_cast<u32x4*>(raw + (c * rows_cap + row) * P + 16 * pj) = d;
    }
  }
  __syncthreads();

  // 3. horizontal pass over the staged rows, cropped columns only
  const int chunks = (nrows + HROWS - 1) / HROWS;
  for (int it = tid; it < 3 * chunks * C; it += RT) {
    const int q = it / C, jj = it - q * C, c = q / chunks, row0 = (q - c * chunks) * HROWS;
    const int lo = hb[2 * jj], cnt = clampi(hb[2 * jj + 1], 0, taps);
    const unsigned char* plane = raw + c * rows_cap * P;
    int at[HROWS];
    uint32_t acc[HROWS];
#pragma unroll
    for (int r = 0; r < HROWS; ++r) { at[r] = min(row0 + r, nrows - 1) * P; acc[r] = HALF; }
    for (int k = 0; k < cnt; ++k) {
      const int x = clampi(lo + k, x0, x1 - 1), w = hk[jj * taps + k];
#pragma unroll
      for (int r = 0; r < HROWS; ++r) acc[r] = mac(acc[r], plane[at[r] + x], w);
    }
    unsigned char* o = hp + (c * rows_cap + row0) * C + jj;
#pragma unroll
    for (int r = 0; r < HROWS; ++r)
      if (row0 + r < nrows) o[r * C] = (unsigned char)to_byte(acc[r]);
  }
  __syncthreads();

  // 4. vertical pass, table, store
  const int groups = C / VCOLS;
  E* o_tile = out + (int64_t)blockIdx.x * 3 * C * C;
  for (int it = tid; it < 3 * Rb * groups; it += RT) {
    const int q = it / groups, g = it - q * groups, c = q / Rb, r = q - c * Rb;
    const int lo = vb[2 * r] - r_lo, cnt = clampi(vb[2 * r + 1], 0, taps);
    const unsigned char* plane = hp + c * rows_cap * C + VCOLS * g;
    uint32_t acc[VCOLS];
#pragma unroll
    for (int x = 0; x < VCOLS; ++x) acc[x] = HALF;
    for (int k = 0; k < cnt; ++k) {
      const int row = clampi(lo + k, 0, nrows - 1), w = vk[r * taps + k];
      const u32x2 d = *reinterpret_cast<const u32x2*>(plane + row * C);
#pragma unroll
      for (int x = 0; x < VCOLS; ++x) acc[x] = mac(acc[x], (int)((d[x >> 2] >> (8 * (x & 3))) & 0xffu), w);
    }
    E v[VCOLS];
#pragma unroll
    for (int x = 0; x < VCOLS; ++x) v[x] = lut[c * 256 + to_byte(acc[x])];
    typedef u32x4 __attribute__((address_space(1))) * gdst;
    const gdst d = reinterpret_cast<gdst>(reinterpret_cast<uintptr_t>(o_tile + ((int64_t)c * C + i0 + r) * C + VCOLS * g));
    if constexpr (sizeof(E) == 2) {
      d[0] = u32x4{(uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16, (uint32_t)v[4] | (uint32_t)v[5] << 16,
                   (uint32_t)v[6] | (uint32_t)v[7] << 16};
    } else {
      d[0] = u32x4{v[0], v[1], v[2], v[3]};
      d[1] = u32x4{v[4], v[5], v[6], v[7]};
    }
  }
}

// taps of Pillow's precompute_coeffs for a filter of support fsup (1: bilinear, 2: bicubic): ceil(fsup * max(P / S, 1)) * 2 + 1
int taps_of(int fsup, int P, int S) { return (P > S ? (fsup * P + S - 1) / S : fsup) * 2 + 1; }

// torchvision's CenterCrop: int(round((S - C) / 2.0)), half to even
int crop_offset(int S, int C) {
  const int d = S - C, m = d / 2;
  return (d & 1) ? m + (m & 1) : m;
}

// input rows a band of R output rows can need: hi(last) - lo(first) <= (R - 1) P / S + 2 support + 1 <= (R - 1) P / S + taps
int band_rows(int R, int P, int S, int taps) {
  const int64_t rows = (int64_t)(R - 1) * P / S + taps + 1;
  return rows < P ? (int)rows : P;
}

int64_t lds_bytes(int R, int P, int S, int C, int taps, int elem_bytes) {
  return 768 * (int64_t)elem_bytes + 4 * ((int64_t)C * (taps + 2) + align4(2 * R) + align4(R * taps)) +
         3 * (int64_t)band_rows(R, P, S, taps) * (P + C);
}

// the largest band that fits `budget`, then the same number of bands in equal parts; 0: not even one row fits
int band_for(int64_t budget, int P, int S, int C, int taps, int elem_bytes) {
  int R = C;
  while (R >= 1 && lds_bytes(R, P, S, C, taps, elem_bytes) > budget) --R;
  if (R < 1) return 0;
  const int bands = (C + R - 1) / R;
  return (C + bands - 1) / bands;
}

template <class E>
int launch(const int64_t* tiles, int n, const int* order, int first, int count, int P, int S, int C, int R, const int* bounds, const int* coef,
           int taps, const void* table, void* out, hipStream_t stream) {
  const int64_t lds = lds_bytes(R, P, S, C, taps, (int)sizeof(E));
  if (lds > LDS_TWO_PER_CU) PATHS_LDS_OPT_IN(tiles_resize_kernel<E>, LDS_ONE_PER_CU, "tiles_resize_to_input");
  hipLaunchKernelGGL(tiles_resize_kernel<E>, dim3(count, (C + R - 1) / R), dim3(RT), (size_t)lds, stream, tiles, n, order, first, P, S, C,
                     crop_offset(S, C), R, band_rows(R, P, S, taps), bounds, coef, taps, reinterpret_cast<const E*>(table),
                     reinterpret_cast<E*>(out));
  PATHS_LAUNCH_CHECK("tiles_resize_to_input");
  return PATHS_OK;
}

}  // namespace

extern "C" {

int paths_tiles_resize_to_input(const int64_t* tiles, int n, const int* order, int first, int count, int P, int S, int C, const int* bounds,
                                const int* coef, int taps, const void* table, int elem_bytes, void* out, hipStream_t stream) {
  PATHS_REQUIRE(n >= 1 && n <= PATHS_TILES_MAX, "tiles_resize_to_input: n = %d is outside [1, %d]", n, PATHS_TILES_MAX);
  PATHS_REQUIRE(tile_shape_ok(P), "tiles_resize_to_input: P = %d must be a multiple of 16 in [16, %d]", P, PATHS_TILE_MAX_P);
  PATHS_REQUIRE(first >= 0 && count >= 1 && (int64_t)first + count <= n,
                "tiles_resize_to_input: [first, first + count) = [%d, %lld) is outside [0, %d]", first, (long long)first + count, n);
  PATHS_REQUIRE(C >= 16 && C <= S && S <= PATHS_RESIZE_MAX, "tiles_resize_to_input: S = %d, C = %d: 16 <= C <= S <= %d", S, C, PATHS_RESIZE_MAX);
  PATHS_REQUIRE(C % 16 == 0, "tiles_resize_to_input: C = %d must be a multiple of 16", C);
  PATHS_REQUIRE(P <= 4 * S, "tiles_resize_to_input: P = %d is more than 4 S = %d (at most %d taps)", P, 4 * S, PATHS_RESIZE_MAX_TAPS);
  PATHS_REQUIRE(taps >= 3 && taps <= PATHS_RESIZE_MAX_TAPS && (taps == taps_of(1, P, S) || taps == taps_of(2, P, S)),
                "tiles_resize_to_input: taps = %d; P = %d to S = %d takes %d (bilinear) or %d (bicubic)", taps, P, S, taps_of(1, P, S),
                taps_of(2, P, S));
  PATHS_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "tiles_resize_to_input: elem_bytes = %d is neither 2 nor 4", elem_bytes);
  PATHS_REQUIRE(tiles && order && bounds && coef && table && out, "tiles_resize_to_input: null pointer (every argument is required)");
  PATHS_REQUIRE((uintptr_t)tiles % 8 == 0 && (uintptr_t)order % 4 == 0 && (uintptr_t)bounds % 4 == 0 && (uintptr_t)coef % 4 == 0 &&
                (uintptr_t)table % elem_bytes == 0 && (uintptr_t)out % 16 == 0, "tiles_resize_to_input: alignment (out: 16 bytes)");
  int R = band_for(LDS_TWO_PER_CU, P, S, C, taps, elem_bytes);
  if (R == 0) R = band_for(LDS_ONE_PER_CU, P, S, C, taps, elem_bytes);
  PATHS_REQUIRE(R >= 1, "tiles_resize_to_input: a band of one output row takes %lld bytes of LDS, more than %lld (P = %d, S = %d, C = %d, taps = %d)",
                (long long)lds_bytes(1, P, S, C, taps, elem_bytes), (long long)LDS_ONE_PER_CU, P, S, C, taps);
  if (elem_bytes == 2) return launch<uint16_t>(tiles, n, order, first, count, P, S, C, R, bounds, coef, taps, table, out, stream);
  return launch<uint32_t>(tiles, n, order, first, count, P, S, C, R, bounds, coef, taps, table, out, stream);
}

}  // extern "C"
