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

}  // extern "C"
