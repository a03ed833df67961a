// Heat-map rasters on the device (paths_amd/heatmap.py:rasterize; include/paths_hip.h: paths_raster_index / paths_raster_maps).
// Painting a patch over its footprint is a gather seen from the raster: every finest cell looks up, per level, the patch that
// covers it.  paths_raster_index turns one level's recorded locations into a cell -> row grid; paths_raster_maps then writes all
// levels and slides of a call in one launch, four consecutive finest cells (16 or 32 bytes of output) per thread.  The kernel is
// bound by the bytes it stores: a patch of level l is read by up to 4^(L-1-l) cells, so index and value reads come from cache.
#include "common.h"

namespace {

constexpr int RASTER_MAX_LEVELS = 8;
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clamp_extent(int g, int G) { return min(max(g, 0), G); }

// one thread per recorded row; rows at or beyond num_ims[b] return before any address is formed from them
__global__ void __launch_bounds__(256)
raster_index_kernel(const int64_t* __restrict__ locs, const int64_t* __restrict__ num_ims, const int* __restrict__ gx,
                    const int* __restrict__ gy, int level, int patch_size, int N, int GX, int GY, int* __restrict__ index, int64_t ldi,
                    int* __restrict__ status) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t n = num_ims[b];
  if (i >= N || i >= n) return;
  const int64_t* p = locs + ((int64_t)b * N + i) * 2;
  const int64_t px = p[0], py = p[1];
  const int64_t ex = (int64_t)clamp_extent(gx[b], GX) << level, ey = (int64_t)clamp_extent(gy[b], GY) << level;
  const int64_t cx = px / patch_size, cy = py / patch_size;
  if (px < 0 || py < 0 || cx >= ex || cy >= ey) {          // outside the slide's own grid: reported, never written
    atomicOr(status, 1 << level);
    return;
  }
  atomicMax(index + ((int64_t)b * ((int64_t)GX << level) + cx) * ldi + cy, i);
}

template <typename O>
__device__ __forceinline__ void store4(O* p, const double (&v)[4]);
template <>
__device__ __forceinline__ void store4<float>(float* p, const double (&v)[4]) {
  stg_f32x4(p, f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]});
}
template <>
__device__ __forceinline__ void store4<double>(double* p, const double (&v)[4]) {
  typedef f64x2 __attribute__((address_space(1))) * gptr;
  gptr g = reinterpret_cast<gptr>(reinterpret_cast<uintptr_t>(p));
  g[0] = f64x2{v[0], v[1]};
  g[1] = f64x2{v[2], v[3]};
}

// V: value type, O: output type.  Thread t of slide b owns cells (x, y0 .. y0 + 3), x = t / n4, y0 = 4 (t % n4), n4 = ldo / 4.
// Levels run from the finest to level 0, so the fold needs one running value per cell.
template <typename V, typename O, bool FOLD>
__global__ void __launch_bounds__(256)
raster_maps_kernel(const int64_t* __restrict__ table, const int* __restrict__ gx, const int* __restrict__ gy, int L, int GX, int GY, int n4,
                   const double* __restrict__ offset_w, O* __restrict__ out, int64_t ldo) {
#pragma clang fp contract(off)
  const int Xf = GX << (L - 1);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Xf * n4) return;
  const int b = blockIdx.y;
  const int x = t / n4, y0 = (t - x * n4) * 4;
  const V off = (V)offset_w[0];
  const double w = offset_w[1];
  // a row or a group of four cells wholly outside the slide's own extent holds nothing: zeros without a load
  const bool inside = x < (clamp_extent(gx[b], GX) << (L - 1)) && y0 < (clamp_extent(gy[b], GY) << (L - 1));
  O* orow = out + ((int64_t)b * (FOLD ? 1 : L) * Xf + x) * ldo + y0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int l = L - 1; l >= 0; --l) {
    const int s = L - 1 - l;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (inside) {
      // (addresses read from a table are "generic" to the compiler: typed as global, the loads are global_load, not flat_load)
      typedef const int __attribute__((address_space(1))) * gint;
      typedef const V __attribute__((address_space(1))) * gval;
      typedef const i32x4 __attribute__((address_space(1))) * gint4;
      const int64_t ld = table[4 * l + 1];
      const gval vals = reinterpret_cast<gval>(static_cast<uintptr_t>(table[4 * l + 2])) + (int64_t)b * table[4 * l + 3];
      const int GYl = GY << l;
      const gint row = reinterpret_cast<gint>(static_cast<uintptr_t>(table[4 * l])) + ((int64_t)b * (Xf >> s) + (x >> s)) * ld;
      int id[4];
      if (s >= 2) {                                   // y0 is a multiple of 4: one cell of this level covers all four
        const int c = y0 >> s;
        id[0] = id[1] = id[2] = id[3] = c < GYl ? row[c] : -1;
      } else if (s == 1) {
        const int c = y0 >> 1;
        id[0] = id[1] = c < GYl ? row[c] : -1;
        id[2] = id[3] = c + 1 < GYl ? row[c + 1] : -1;
      } else if (y0 + 3 < GYl && ((reinterpret_cast<uintptr_t>(row + y0) & 15) == 0)) {
        const i32x4 q = *reinterpret_cast<gint4>(row + y0);
        id[0] = q.x, id[1] = q.y, id[2] = q.z, id[3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = y0 + j < GYl ? row[y0 + j] : -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j > 0 && id[j] == id[j - 1]) v[j] = v[j - 1];
        else if (id[j] >= 0) v[j] = (double)(V)(vals[id[j]] + off);
      }
    }
    if (FOLD) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (acc[j] != 0.0) v[j] = v[j] + acc[j] * w;
        acc[j] = v[j];
      }
    } else {
      store4<O>(orow + (int64_t)l * Xf * ldo, v);
    }
  }
  if (FOLD) store4<O>(orow, acc);
}

template <typename V, typename O>
void launch_maps(bool fold, dim3 grid, hipStream_t stream, const int64_t* table, const int* gx, const int* gy, int L, int GX, int GY, int n4,
                 const double* offset_w, void* out, int64_t ldo) {
  if (fold) hipLaunchKernelGGL((raster_maps_kernel<V, O, true>), grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, n4, offset_w, (O*)out, ldo);
  else hipLaunchKernelGGL((raster_maps_kernel<V, O, false>), grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, n4, offset_w, (O*)out, ldo);
}

// ---- overlays: the raster above as pixels (paths_amd/heatmap.py:render; paths_render_range / paths_render_rgb) ------------

constexpr int RENDER_PARTS = 64;       // partial (min, max) blocks per slide: the launch shape of the range does not depend on the data
constexpr int RENDER_RUN = 16;         // pixels per thread: 48 bytes, three 16-byte stores

struct Cell {
  int bits;        // bit l: level l's index grid names a row on the cell of level l that covers this finest cell (levels of `mask` only)
  int first;       // bit l: this finest cell lies in the first column of that cell,
  int last;        //        in its last column
};

// finest cell (x, y) of slide b, inside the slide's own extent (so every index address is inside its grid)
__device__ __forceinline__ Cell lookup_cell(const int64_t* __restrict__ table, int b, int L, int Xf, int x, int y, int mask) {
  typedef const int __attribute__((address_space(1))) * gint;
  Cell c = {0, 0, 0};
  for (int l = 0; l < L; ++l) {
    if (!(mask >> l & 1)) continue;
    const int s = L - 1 - l, m = (1 << s) - 1;
    const gint row = reinterpret_cast<gint>(static_cast<uintptr_t>(table[4 * l])) + ((int64_t)b * (Xf >> s) + (x >> s)) * table[4 * l + 1];
    if (row[y >> s] < 0) continue;
    c.bits |= 1 << l;
    if ((y & m) == 0) c.first |= 1 << l;
    if ((y & m) == m) c.last |= 1 << l;
  }
  return c;
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }     // (false for NaN)

// stage 1 of the range: block p of slide b folds cells p * 256 + t, + RENDER_PARTS * 256, ... of the slide's own extent into one
// (min, max, non-finite seen); min and max of finite values do not depend on the order they are taken in
template <typename V>
__global__ void __launch_bounds__(256)
render_range_partial_kernel(const int64_t* __restrict__ table, const int* __restrict__ gx, const int* __restrict__ gy, int L, int GX, int GY,
                            int drawn, const V* __restrict__ raster, int64_t slide_stride, int64_t ldo, double* __restrict__ partial) {
  __shared__ double s_lo[256], s_hi[256];
  __shared__ int s_bad[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int Xf = GX << (L - 1);
  const int ex = clamp_extent(gx[b], GX) << (L - 1), ey = clamp_extent(gy[b], GY) << (L - 1);
  const int64_t n = (int64_t)ex * ey;
  double lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)RENDER_PARTS * 256) {
    const int x = (int)(i / ey), y = (int)(i - (int64_t)x * ey);
    if (lookup_cell(table, b, L, Xf, x, y, drawn).bits == 0) continue;
    const double v = (double)raster[(int64_t)b * slide_stride + (int64_t)x * ldo + y];
    if (!finite64(v)) bad = 1;
    else {
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  s_lo[tid] = lo, s_hi[tid] = hi, s_bad[tid] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      s_lo[tid] = s_lo[tid + w] < s_lo[tid] ? s_lo[tid + w] : s_lo[tid];
      s_hi[tid] = s_hi[tid + w] > s_hi[tid] ? s_hi[tid + w] : s_hi[tid];
      s_bad[tid] |= s_bad[tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* p = partial + ((int64_t)b * RENDER_PARTS + blockIdx.x) * 3;
    p[0] = s_lo[0], p[1] = s_hi[0], p[2] = (double)s_bad[0];
  }
}

// stage 2: one thread per slide.  "+ 0.0" turns a -0 extreme into +0, whichever zero the comparisons kept.
__global__ void __launch_bounds__(64)
render_range_finish_kernel(const double* __restrict__ partial, const double* __restrict__ center, int B, double* __restrict__ range,
                           int* __restrict__ status) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double lo = INFINITY, hi = -INFINITY, bad = 0.0;
  for (int p = 0; p < RENDER_PARTS; ++p) {
    const double* q = partial + ((int64_t)b * RENDER_PARTS + p) * 3;
    lo = q[0] < lo ? q[0] : lo;
    hi = q[1] > hi ? q[1] : hi;
    bad = q[2] != 0.0 ? 1.0 : bad;
  }
  double vmin = 0.0, vmax = 0.0;
  if (lo <= hi) {
    if (center != nullptr) {                    // rounding is monotonic: max |v - z| is taken at one of the two extremes
      const double z = center[0];
      const double m = fmax(fabs(lo - z), fabs(hi - z));
      vmin = z - m, vmax = z + m;
    } else {
      vmin = lo + 0.0, vmax = hi + 0.0;
    }
  }
  range[2 * b] = vmin, range[2 * b + 1] = vmax;
  status[b] = bad != 0.0;
}

__device__ __forceinline__ uint32_t blend_rgb(uint32_t colour, uint32_t under, uint32_t a) {
  uint32_t px = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t cc = colour >> (8 * ch) & 255u, uu = under >> (8 * ch) & 255u;
    px |= ((a * cc + (255u - a) * uu + 127u) / 255u) << (8 * ch);
  }
  return px;
}

// Thread t of slide b owns pixels (u, 16 r .. 16 r + 15) = bytes [48 r, 48 r + 48) of image row u: u = t / runs, r = t % runs.  A pixel
// is r | g << 8 | b << 16 here; the sixteen of them are packed into twelve words and leave as three 16-byte stores.
template <typename V, bool THUMB>
__global__ void __launch_bounds__(256)
render_rgb_kernel(const int64_t* __restrict__ table, const int* __restrict__ gx, const int* __restrict__ gy, int L, int GX, int GY, int drawn,
                  int outlined, const V* __restrict__ raster, int64_t slide_stride, int64_t ldo, const double* __restrict__ range,
                  const uint32_t* __restrict__ colours, const int64_t* __restrict__ thumbs, int c, uint32_t a, uint32_t outline_rgb,
                  uint32_t background, uint8_t* __restrict__ out, int64_t ldp, int runs) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int Xf = GX << (L - 1);
  const int64_t rows = (int64_t)Xf * c;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * runs) return;
  const int u = (int)(t / runs), r = (int)(t - (int64_t)u * runs);
  const int ex = clamp_extent(gx[b], GX) << (L - 1), ey = clamp_extent(gy[b], GY) << (L - 1);
  const int x = u / c, pu = u - x * c;
  const int v0 = r * RENDER_RUN;
  const int64_t eyc = (int64_t)ey * c;
  const bool inside = x < ex && v0 < eyc;
  uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (inside) {
    uint32_t tw[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (THUMB) {
      typedef const uint8_t __attribute__((address_space(1))) * gbyte;
      typedef const u32x4 __attribute__((address_space(1))) * gquad;
      const uintptr_t at = static_cast<uintptr_t>(thumbs[2 * b]) + (uintptr_t)((int64_t)u * thumbs[2 * b + 1]) + (uintptr_t)v0 * 3;
      const int64_t left = (eyc - v0) * 3;                        // bytes of this row from the run's first one
      if (left >= 48 && (at & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const u32x4 q = reinterpret_cast<gquad>(at)[k];
          tw[4 * k] = q.x, tw[4 * k + 1] = q.y, tw[4 * k + 2] = q.z, tw[4 * k + 3] = q.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 48; ++k)
          if (k < left) tw[k / 4] |= (uint32_t) reinterpret_cast<gbyte>(at)[k] << (8 * (k % 4));
      }
    }
    // which levels put an outline on this image row: first or last pixel row of the level's cell
    int edge_row = 0;
    for (int l = 0; l < L; ++l) {
      const int s = L - 1 - l, q = (x & ((1 << s) - 1)) * c + pu;
      if (q == 0 || q == (c << s) - 1) edge_row |= 1 << l;
    }
    const double vmin = range[2 * b], vmax = range[2 * b + 1];
    const double span = vmax - vmin;
    int y = v0 / c, pv = v0 - y * c;
    bool fresh = true, vis = false;
    Cell cell = {0, 0, 0};
    uint32_t colour = 0, flat = 0;
#pragma unroll
    for (int j = 0; j < RENDER_RUN; ++j) {
      if (v0 + j < eyc) {
        if (fresh) {
          fresh = false;
          cell = lookup_cell(table, b, L, Xf, x, y, drawn | outlined);
          vis = false;
          if (cell.bits & drawn) {
            const double v = (double)raster[(int64_t)b * slide_stride + (int64_t)x * ldo + y];
            if (finite64(v)) {
              vis = true;
              int k = 0;
              if (vmax != vmin) {
                const double t256 = (v - vmin) / span * 256.0;
                k = t256 >= 255.0 ? 255 : (t256 > 0.0 ? (int)t256 : 0);
              }
              colour = colours[k];
              if (!THUMB) flat = blend_rgb(colour, background, a);
            }
          }
        }
        uint32_t under = background;
        if (THUMB) {
          const int bit = 24 * j, lo = bit / 32, sh = bit % 32;
          under = tw[lo] >> sh;
          if (sh > 8) under |= tw[lo + 1] << (32 - sh);
          under &= 0xFFFFFFu;
        }
        uint32_t px = under;
        if (vis) px = THUMB ? blend_rgb(colour, under, a) : flat;
        const int lv = cell.bits & outlined;
        if ((lv & edge_row) || (pv == 0 && (lv & cell.first)) || (pv == c - 1 && (lv & cell.last))) px = outline_rgb;
        const int bit = 24 * j, lo = bit / 32, sh = bit % 32;
        w[lo] |= px << sh;
        if (sh > 8) w[lo + 1] |= px >> (32 - sh);
      }
      if (++pv == c) pv = 0, ++y, fresh = true;
    }
  }
  uint8_t* dst = out + ((int64_t)b * rows + u) * ldp + (int64_t)r * 48;
  typedef u32x4 __attribute__((address_space(1))) * gquad_w;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if ((int64_t)r * 48 + 16 * k < ldp) reinterpret_cast<gquad_w>(reinterpret_cast<uintptr_t>(dst))[k] = u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
}

template <typename V>
void launch_rgb(bool thumb, dim3 grid, hipStream_t stream, const int64_t* table, const int* gx, const int* gy, int L, int GX, int GY, int drawn,
                       int outlined, const V* raster, int64_t slide_stride, int64_t ldo, const double* range, const uint32_t* colours,
                       const int64_t* thumbs, int c, uint32_t a, uint32_t outline_rgb, uint32_t background, uint8_t* out, int64_t ldp, int runs) {
  if (thumb)
    hipLaunchKernelGGL((render_rgb_kernel<V, true>), grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, drawn, outlined, raster, slide_stride,
                       ldo, range, colours, thumbs, c, a, outline_rgb, background, out, ldp, runs);
  else
    hipLaunchKernelGGL((render_rgb_kernel<V, false>), grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, drawn, outlined, raster, slide_stride,
                       ldo, range, colours, thumbs, c, a, outline_rgb, background, out, ldp, runs);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int paths_raster_index(const int64_t* locs, const int64_t* num_ims, const int* gx, const int* gy, int level, int patch_size, int N, int B,
                       int GX, int GY, int* index, int64_t ldi, int* status, hipStream_t stream) {
  PATHS_REQUIRE(locs && num_ims && gx && gy && index && status, "paths_raster_index: null pointer");
  PATHS_REQUIRE(B >= 1 && B <= 65535, "paths_raster_index: B = %d not in [1, 65535]", B);
  PATHS_REQUIRE(N >= 1, "paths_raster_index: N = %d must be positive", N);
  PATHS_REQUIRE(patch_size >= 1, "paths_raster_index: patch_size = %d must be positive", patch_size);
  PATHS_REQUIRE(level >= 0 && level < RASTER_MAX_LEVELS, "paths_raster_index: level = %d not in [0, %d)", level, RASTER_MAX_LEVELS);
  PATHS_REQUIRE(GX >= 1 && GY >= 1 && GX <= (1 << 20) && GY <= (1 << 20), "paths_raster_index: extent GX = %d, GY = %d not in [1, 2^20]", GX, GY);
  PATHS_REQUIRE(ldi >= ((int64_t)GY << level), "paths_raster_index: stride ldi = %lld below GY << level = %lld", (long long)ldi,
                (long long)((int64_t)GY << level));
  PATHS_REQUIRE(aligned(locs, 8) && aligned(num_ims, 8) && aligned(gx, 4) && aligned(gy, 4) && aligned(index, 4) && aligned(status, 4),
                "paths_raster_index: alignment (int64 tables 8 bytes, int32 tables 4 bytes)");
  hipLaunchKernelGGL(raster_index_kernel, dim3((N + 255) / 256, B), dim3(256), 0, stream, locs, num_ims, gx, gy, level, patch_size, N, GX, GY,
                     index, ldi, status);
  PATHS_LAUNCH_CHECK("paths_raster_index");
  return PATHS_OK;
}

int paths_raster_maps(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int value_f64, int out_f64, int fold,
                      const double* offset_w, void* out, int64_t ldo, hipStream_t stream) {
  PATHS_REQUIRE(table && gx && gy && offset_w && out, "paths_raster_maps: null pointer");
  PATHS_REQUIRE(B >= 1 && B <= 65535, "paths_raster_maps: B = %d not in [1, 65535]", B);
  PATHS_REQUIRE(L >= 1 && L <= RASTER_MAX_LEVELS, "paths_raster_maps: L = %d not in [1, %d]", L, RASTER_MAX_LEVELS);
  PATHS_REQUIRE(GX >= 1 && GY >= 1 && GX <= (1 << 20) && GY <= (1 << 20), "paths_raster_maps: extent GX = %d, GY = %d not in [1, 2^20]", GX, GY);
  const int64_t Xf = (int64_t)GX << (L - 1), Yf = (int64_t)GY << (L - 1);
  PATHS_REQUIRE(ldo >= Yf && ldo % 4 == 0, "paths_raster_maps: stride ldo = %lld must be a multiple of 4 and at least GY << (L-1) = %lld",
                (long long)ldo, (long long)Yf);
  PATHS_REQUIRE(Xf * (ldo / 4) < ((int64_t)1 << 31) - 256, "paths_raster_maps: raster of %lld x %lld cells per slide is too large", (long long)Xf,
                (long long)ldo);
  PATHS_REQUIRE(aligned(out, 16) && aligned(table, 8) && aligned(offset_w, 8) && aligned(gx, 4) && aligned(gy, 4),
                "paths_raster_maps: alignment (out 16 bytes, table and offset_w 8 bytes, int32 tables 4 bytes)");
  const int n4 = (int)(ldo / 4);
  const dim3 grid((unsigned)((Xf * n4 + 255) / 256), B);
  if (value_f64) {
    if (out_f64) launch_maps<double, double>(fold != 0, grid, stream, table, gx, gy, L, GX, GY, n4, offset_w, out, ldo);
    else launch_maps<double, float>(fold != 0, grid, stream, table, gx, gy, L, GX, GY, n4, offset_w, out, ldo);
  } else {
    if (out_f64) launch_maps<float, double>(fold != 0, grid, stream, table, gx, gy, L, GX, GY, n4, offset_w, out, ldo);
    else launch_maps<float, float>(fold != 0, grid, stream, table, gx, gy, L, GX, GY, n4, offset_w, out, ldo);
  }
  PATHS_LAUNCH_CHECK("paths_raster_maps");
  return PATHS_OK;
}

#define RENDER_REQUIRE_COMMON(name)                                                                                                        \
  PATHS_REQUIRE(B >= 1 && B <= 65535, name ": B = %d not in [1, 65535]", B);                                                               \
  PATHS_REQUIRE(L >= 1 && L <= RASTER_MAX_LEVELS, name ": L = %d not in [1, %d]", L, RASTER_MAX_LEVELS);                                   \
  PATHS_REQUIRE(level >= -1 && level < L, name ": level = %d not in [-1, L = %d)", level, L);                                             \
  PATHS_REQUIRE(GX >= 1 && GY >= 1 && GX <= (1 << 20) && GY <= (1 << 20), name ": extent GX = %d, GY = %d not in [1, 2^20]", GX, GY);      \
  PATHS_REQUIRE(ldo >= ((int64_t)GY << (L - 1)), name ": stride ldo = %lld below GY << (L-1) = %lld", (long long)ldo,                      \
                (long long)((int64_t)GY << (L - 1)))

int paths_render_range(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int level, const void* raster,
                       int raster_f64, int64_t ldo, const double* center, double* partial, double* range, int* status, hipStream_t stream) {
  PATHS_REQUIRE(table && gx && gy && raster && partial && range && status, "paths_render_range: null pointer");
  RENDER_REQUIRE_COMMON("paths_render_range");
  PATHS_REQUIRE(aligned(table, 8) && aligned(raster, raster_f64 ? 8 : 4) && aligned(center, 8) && aligned(partial, 8) && aligned(range, 8) &&
                aligned(gx, 4) && aligned(gy, 4) && aligned(status, 4),
                "paths_render_range: alignment (fp64 and int64 tables 8 bytes, fp32 and int32 tables 4 bytes)");
  const int64_t Xf = (int64_t)GX << (L - 1);
  const int64_t slide_stride = (level < 0 ? 1 : L) * Xf * ldo, plane = level < 0 ? 0 : level * Xf * ldo;
  const int drawn = level < 0 ? (1 << L) - 1 : 1 << level;
  const dim3 grid(RENDER_PARTS, B);
  if (raster_f64)
    hipLaunchKernelGGL(render_range_partial_kernel<double>, grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, drawn,
                       (const double*)raster + plane, slide_stride, ldo, partial);
  else
    hipLaunchKernelGGL(render_range_partial_kernel<float>, grid, dim3(256), 0, stream, table, gx, gy, L, GX, GY, drawn,
                       (const float*)raster + plane, slide_stride, ldo, partial);
  hipLaunchKernelGGL(render_range_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, partial, center, B, range, status);
  PATHS_LAUNCH_CHECK("paths_render_range");
  return PATHS_OK;
}

int paths_render_rgb(const int64_t* table, const int* gx, const int* gy, int L, int B, int GX, int GY, int level, const void* raster,
                     int raster_f64, int64_t ldo, const double* range, const uint32_t* colours, const int64_t* thumbs, int cell_px, int alpha255,
                     int outline_levels, uint32_t outline_rgb, uint32_t background, uint8_t* out, int64_t ldp, hipStream_t stream) {
  PATHS_REQUIRE(table && gx && gy && raster && range && colours && out, "paths_render_rgb: null pointer");
  RENDER_REQUIRE_COMMON("paths_render_rgb");
  PATHS_REQUIRE(cell_px >= 1 && cell_px <= 64, "paths_render_rgb: cell_px = %d not in [1, 64]", cell_px);
  PATHS_REQUIRE(alpha255 >= 0 && alpha255 <= 255, "paths_render_rgb: alpha255 = %d not in [0, 255]", alpha255);
  PATHS_REQUIRE(outline_levels >= 0 && outline_levels < (1 << L), "paths_render_rgb: outline_levels = %d names a level beyond L = %d",
                outline_levels, L);
  const int64_t rows = ((int64_t)GX << (L - 1)) * cell_px, row_bytes = ((int64_t)GY << (L - 1)) * cell_px * 3;
  PATHS_REQUIRE(ldp >= row_bytes && ldp % 16 == 0, "paths_render_rgb: stride ldp = %lld must be a multiple of 16 and at least %lld bytes",
                (long long)ldp, (long long)row_bytes);
  const int64_t runs = (ldp + 3 * RENDER_RUN - 1) / (3 * RENDER_RUN);
  PATHS_REQUIRE(rows * runs < ((int64_t)1 << 31) - 256 && ldp < ((int64_t)1 << 31), "paths_render_rgb: image of %lld rows x %lld bytes per slide is too large",
                (long long)rows, (long long)ldp);
  PATHS_REQUIRE(aligned(out, 16) && aligned(table, 8) && aligned(raster, raster_f64 ? 8 : 4) && aligned(range, 8) && aligned(thumbs, 8) &&
                aligned(colours, 4) && aligned(gx, 4) && aligned(gy, 4),
                "paths_render_rgb: alignment (out 16 bytes, fp64 and int64 tables 8 bytes, fp32 and 32-bit tables 4 bytes)");
  const int64_t Xf = (int64_t)GX << (L - 1);
  const int64_t slide_stride = (level < 0 ? 1 : L) * Xf * ldo, plane = level < 0 ? 0 : level * Xf * ldo;
  const int drawn = level < 0 ? (1 << L) - 1 : 1 << level;
  const dim3 grid((unsigned)((rows * runs + 255) / 256), B);
  if (raster_f64)
    launch_rgb<double>(thumbs != nullptr, grid, stream, table, gx, gy, L, GX, GY, drawn, outline_levels, (const double*)raster + plane, slide_stride,
                       ldo, range, colours, thumbs, cell_px, (uint32_t)alpha255, outline_rgb & 0xFFFFFFu, background & 0xFFFFFFu, out, ldp, (int)runs);
  else
    launch_rgb<float>(thumbs != nullptr, grid, stream, table, gx, gy, L, GX, GY, drawn, outline_levels, (const float*)raster + plane, slide_stride,
                      ldo, range, colours, thumbs, cell_px, (uint32_t)alpha255, outline_rgb & 0xFFFFFFu, background & 0xFFFFFFu, out, ldp, (int)runs);
  PATHS_LAUNCH_CHECK("paths_render_rgb");
  return PATHS_OK;
}

}  // extern "C"
