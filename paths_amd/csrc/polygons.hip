// Annotation polygons on the device (paths_amd/annotations.py; include/paths_hip.h: paths_polygon_cover / paths_polygon_outline;
// DESIGN 27).  Coordinates are int32 with 16 fractional bits per finest cell, every predicate is exact integer arithmetic (the header
// derives the 2^61 bound), so the kernels equal tests/polygon_ref.py bit for bit.
//
// Coverage: a workgroup of 256 threads owns 16 x 16 finest cells, one cell per thread, and streams its slide's edges through one LDS
// tile of 256 edges, polygon by polygon: 256 edges are loaded (one per thread), those that can change a sample of the tile are
// compacted into LDS through wave ballots (no atomics), then every thread walks the kept edges - all lanes read the same LDS address, a
// broadcast.  A cell keeps one parity bit per sample (s * s <= 256 bits) and ORs it into its union mask at the end of each polygon.
// What an edge costs a cell: nothing when its rows miss the cell's sample rows or it lies wholly on the near side of the cell's first
// sample column; a row test per sample row when it lies wholly beyond the last one; else one 64-bit product pair per crossed sample
// row and a 64-bit add and compare per sample (t is linear in the sample column).  A 64-bit product of two int32 values is a
// v_mul_lo / v_mul_hi pair, the slow integer instructions of the VALU, so products are what the per-cell classification avoids.
#include "common.h"

namespace {

constexpr int COVER_TILE = 16;         // cells per side of a workgroup's tile
constexpr int COVER_EDGES = 256;       // edges per LDS tile = threads per workgroup
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int S>
__global__ void __launch_bounds__(COVER_EDGES)
polygon_cover_kernel(const int* __restrict__ verts, int V, const int* __restrict__ poly_off, int P, const int* __restrict__ slide_poly,
                     const int* __restrict__ gx, const int* __restrict__ gy, int X, int Y, int* __restrict__ out, int64_t ld) {
  constexpr int WORDS = (S * S + 31) / 32;
  constexpr int STEP = 65536 / S;                 // distance of two sample points
  constexpr int FIRST = STEP / 2;                 // ((2 * 0 + 1) << 15) >> log2 S
  __shared__ i32x4 s_edge[COVER_EDGES];           // (a.r, a.c, b.r, b.c)
  __shared__ int s_count[COVER_EDGES / 64];
  const int b = blockIdx.z, tid = threadIdx.x;
  const int x = blockIdx.y * COVER_TILE + tid / COVER_TILE, y = blockIdx.x * COVER_TILE + tid % COVER_TILE;
  const int ex = clampi(gx[b], 0, X), ey = clampi(gy[b], 0, Y);
  const bool mine = x < ex && y < ey;             // this thread's cell lies inside the slide
  uint32_t inside[WORDS], parity[WORDS];
#pragma unroll
  for (int w = 0; w < WORDS; ++w) inside[w] = parity[w] = 0;

  // a tile wholly outside the slide's extent holds zeros: no edge is loaded (uniform over the workgroup)
  if (blockIdx.y * COVER_TILE < ex && blockIdx.x * COVER_TILE < ey) {
    // the tile's sample rows and columns that lie inside the slide
    const int tr_lo = ((blockIdx.y * COVER_TILE) << 16) + FIRST;
    const int tr_hi = ((min((int)(blockIdx.y + 1) * COVER_TILE, ex) - 1) << 16) + FIRST + (S - 1) * STEP;
    const int tc_lo = ((blockIdx.x * COVER_TILE) << 16) + FIRST;
    const int pr0 = (x << 16) + FIRST, pr_last = pr0 + (S - 1) * STEP;
    const int pc0 = (y << 16) + FIRST, pc_last = pc0 + (S - 1) * STEP;
    const int p0 = clampi(slide_poly[b], 0, P), p1 = clampi(slide_poly[b + 1], p0, P);
    const int lane = tid & 63, wave = tid >> 6;
    for (int k = p0; k < p1; ++k) {
      const int v0 = clampi(poly_off[k], 0, V), v1 = clampi(poly_off[k + 1], v0, V);
      for (int e0 = v0; e0 < v1; e0 += COVER_EDGES) {
        // load one edge per thread; keep it when it can flip a sample of this tile
        const int e = e0 + tid;
        i32x4 edge = {0, 0, 0, 0};
        bool keep = false;
        if (e < v1) {
          const i32x2 a = *reinterpret_cast<const i32x2*>(verts + 2 * (int64_t)e);
          const i32x2 c = *reinterpret_cast<const i32x2*>(verts + 2 * (int64_t)(e + 1 < v1 ? e + 1 : v0));
          edge = i32x4{a.x, a.y, c.x, c.y};
          // a sample row p.r counts when min(a.r, b.r) <= p.r < max(a.r, b.r); a crossing lies within [min c, max c]
          keep = a.x != c.x && min(a.x, c.x) <= tr_hi && max(a.x, c.x) > tr_lo && max(a.y, c.y) > tc_lo;
        }
        const unsigned long long vote = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(vote);
        __syncthreads();
        int at = __popcll(vote & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
        for (int w = 0; w < COVER_EDGES / 64; ++w) {
          if (w < wave) at += s_count[w];
          kept += s_count[w];
        }
        if (keep) s_edge[at] = edge;
        __syncthreads();
        if (mine) {
          for (int i = 0; i < kept; ++i) {
            const i32x4 q = s_edge[i];
            const int ar = q.x, ac = q.y, br = q.z, bc = q.w;
            if (max(ar, br) <= pr0 || min(ar, br) > pr_last || max(ac, bc) <= pc0) continue;
            if (min(ac, bc) > pc_last) {            // wholly beyond this cell's samples: the row test decides a whole sample row
#pragma unroll
              for (int r = 0; r < S; ++r) {
                const int pr = pr0 + r * STEP;
                if ((ar > pr) != (br > pr)) parity[(r * S) / 32] ^= ((1u << S) - 1u) << ((r * S) % 32);
              }
              continue;
            }
            // t' = sign(d) t: the crossing lies beyond p.c when t' < 0; t' grows by STEP |d| per sample column
            const int d = br - ar;
            const int64_t ad = d < 0 ? -(int64_t)d : (int64_t)d;
            const int64_t sdc = d < 0 ? -(int64_t)(bc - ac) : (int64_t)(bc - ac);
            const int64_t t_c0 = (int64_t)(pc0 - ac) * ad, dt = (int64_t)STEP * ad;
#pragma unroll
            for (int r = 0; r < S; ++r) {
              const int pr = pr0 + r * STEP;
              if ((ar > pr) != (br > pr)) {
                int64_t t = t_c0 - (int64_t)(pr - ar) * sdc;
                uint32_t row = 0;
#pragma unroll
                for (int j = 0; j < S; ++j) {
                  row |= (uint32_t)(t < 0) << j;
                  t += dt;
                }
                parity[(r * S) / 32] ^= row << ((r * S) % 32);
              }
            }
          }
        }
        __syncthreads();                             // the tile is free for the next 256 edges
      }
#pragma unroll
      for (int w = 0; w < WORDS; ++w) inside[w] |= parity[w], parity[w] = 0;
    }
  }
  int n = 0;
#pragma unroll
  for (int w = 0; w < WORDS; ++w) n += __popc(inside[w]);
  if (x < X && y < ld) out[((int64_t)b * X + x) * ld + y] = mine ? n : 0;
}

// floor(a / m), m > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t m) {
  const int64_t q = a / m;
  return (a % m < 0) ? q - 1 : q;
}

// the last index i of [0, n) with table[i] <= t, table ascending from table[0] <= t (any table: the result stays in [0, n))
__device__ __forceinline__ int last_at_or_below(const int* __restrict__ table, int n, int64_t t) {
  int lo = 0, hi = n;                  // table[lo] <= t < table[hi] (hi = n: beyond the table)
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if ((int64_t)table[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256)
polygon_outline_kernel(const int* __restrict__ verts, int V, const int* __restrict__ poly_off, int P, const int* __restrict__ slide_poly,
                       const int* __restrict__ gx, const int* __restrict__ gy, int B, const int* __restrict__ cum, int64_t steps,
                       const int64_t* __restrict__ images, int c, int width, uint32_t rgb) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= steps) return;
  const int e = last_at_or_below(cum, V, t);                 // the edge that starts at vertex e
  const int k = last_at_or_below(poly_off, P, e);            // its polygon
  const int b = last_at_or_below(slide_poly, B, k);          // its slide
  const int v0 = clampi(poly_off[k], 0, V), v1 = clampi(poly_off[k + 1], v0, V);
  if (e < v0 || e >= v1) return;                             // (tables that do not belong together)
  const i32x2 a = *reinterpret_cast<const i32x2*>(verts + 2 * (int64_t)e);
  const i32x2 q = *reinterpret_cast<const i32x2*>(verts + 2 * (int64_t)(e + 1 < v1 ? e + 1 : v0));
  const int64_t u0 = ((int64_t)a.x * c) >> 16, w0 = ((int64_t)a.y * c) >> 16;
  const int64_t du = (((int64_t)q.x * c) >> 16) - u0, dv = (((int64_t)q.y * c) >> 16) - w0;
  const int64_t n = max(du < 0 ? -du : du, dv < 0 ? -dv : dv);
  const int64_t step = t - cum[e];
  if (step < 0 || step > n) return;
  int64_t u = u0, w = w0;
  if (n > 0) {
    u += floor_div(2 * step * du + n, 2 * n);
    w += floor_div(2 * step * dv + n, 2 * n);
  }
  const int64_t eu = (int64_t)clampi(gx[b], 0, 8192) * c, ew = (int64_t)clampi(gy[b], 0, 8192) * c;
  typedef uint8_t __attribute__((address_space(1))) * gbyte;
  const uintptr_t base = static_cast<uintptr_t>(images[2 * b]);
  const int64_t stride = images[2 * b + 1];
  const uint8_t r8 = rgb & 255u, g8 = rgb >> 8 & 255u, b8 = rgb >> 16 & 255u;
  const int half = width / 2;
  for (int i = 0; i < width; ++i) {
    const int64_t pu = u - half + i;
    if (pu < 0 || pu >= eu) continue;
    for (int j = 0; j < width; ++j) {
      const int64_t pw = w - half + j;
      if (pw < 0 || pw >= ew) continue;
      gbyte px = reinterpret_cast<gbyte>(base + (uintptr_t)(pu * stride + pw * 3));
      px[0] = r8, px[1] = g8, px[2] = b8;
    }
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

#define POLYGON_REQUIRE_COMMON(name)                                                                                                        \
  PATHS_REQUIRE(verts && poly_off && slide_poly && gx && gy, name ": null pointer");                                                       \
  PATHS_REQUIRE(B >= 1 && B <= 65535, name ": B = %d not in [1, 65535]", B);                                                               \
  PATHS_REQUIRE(V >= 0 && V <= (1 << 20), name ": V = %d not in [0, 2^20]", V);                                                            \
  PATHS_REQUIRE(P >= 0 && P <= V / 3, name ": P = %d polygons of at least 3 vertices do not fit V = %d", P, V);                            \
  PATHS_REQUIRE(aligned(verts, 8) && aligned(poly_off, 4) && aligned(slide_poly, 4) && aligned(gx, 4) && aligned(gy, 4),                   \
                name ": alignment (verts 8 bytes, int32 tables 4 bytes)")

int paths_polygon_cover(const int* verts, int V, const int* poly_off, int P, const int* slide_poly, const int* gx, const int* gy, int B, int X,
                        int Y, int samples, int* out, int64_t ld, hipStream_t stream) {
  POLYGON_REQUIRE_COMMON("paths_polygon_cover");
  PATHS_REQUIRE(out != nullptr && aligned(out, 4), "paths_polygon_cover: out is null or not 4-byte aligned");
  PATHS_REQUIRE(X >= 1 && Y >= 1 && X <= 8192 && Y <= 8192, "paths_polygon_cover: extent X = %d, Y = %d not in [1, 8192]", X, Y);
  PATHS_REQUIRE(ld >= Y && ld <= 8192 + 16, "paths_polygon_cover: stride ld = %lld not in [Y = %d, 8208]", (long long)ld, Y);
  const dim3 grid((unsigned)((ld + COVER_TILE - 1) / COVER_TILE), (unsigned)((X + COVER_TILE - 1) / COVER_TILE), (unsigned)B);
#define COVER_LAUNCH(S)                                                                                                             \
  hipLaunchKernelGGL(polygon_cover_kernel<S>, grid, dim3(COVER_EDGES), 0, stream, verts, V, poly_off, P, slide_poly, gx, gy, X, Y, out, ld)
  switch (samples) {
    case 1: COVER_LAUNCH(1); break;
    case 2: COVER_LAUNCH(2); break;
    case 4: COVER_LAUNCH(4); break;
    case 8: COVER_LAUNCH(8); break;
    case 16: COVER_LAUNCH(16); break;
    default: return paths_set_error(PATHS_EINVAL, "paths_polygon_cover: samples = %d is none of 1, 2, 4, 8, 16", samples);
  }
#undef COVER_LAUNCH
  PATHS_LAUNCH_CHECK("paths_polygon_cover");
  return PATHS_OK;
}

int paths_polygon_outline(const int* verts, int V, const int* poly_off, int P, const int* slide_poly, const int* gx, const int* gy, int B,
                          const int* cum, int64_t steps, const int64_t* images, int cell_px, int width, uint32_t rgb, hipStream_t stream) {
  POLYGON_REQUIRE_COMMON("paths_polygon_outline");
  PATHS_REQUIRE(cum && images && aligned(cum, 4) && aligned(images, 8), "paths_polygon_outline: cum or images is null or misaligned");
  PATHS_REQUIRE(V >= 3 && P >= 1, "paths_polygon_outline: no polygon to draw (V = %d, P = %d)", V, P);
  PATHS_REQUIRE(cell_px >= 1 && cell_px <= 64, "paths_polygon_outline: cell_px = %d not in [1, 64]", cell_px);
  PATHS_REQUIRE(width >= 1 && width <= 7, "paths_polygon_outline: width = %d not in [1, 7]", width);
  PATHS_REQUIRE(steps >= 1 && steps < ((int64_t)1 << 31) - 256, "paths_polygon_outline: steps = %lld not in [1, 2^31 - 256)", (long long)steps);
  hipLaunchKernelGGL(polygon_outline_kernel, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, stream, verts, V, poly_off, P, slide_poly, gx,
                     gy, B, cum, steps, images, cell_px, width, rgb & 0xFFFFFFu);
  PATHS_LAUNCH_CHECK("paths_polygon_outline");
  return PATHS_OK;
}

}  // extern "C"
