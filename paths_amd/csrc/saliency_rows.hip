// paths_saliency_rows: per-patch reductions of the feature gradient (paths_amd/saliency.py:input_gradients).
//   gxi[r] = sum_d dX[r,d] X[r,d]  (gradient x input)     gnorm[r] = sqrt(sum_d dX[r,d]^2)  (gradient norm)
// One wave per row, 16-byte loads, four rows per workgroup.  Every lane sums its columns in ascending order and the 64 partial sums
// meet in a fixed butterfly (in registers, no LDS, no atomics): the result of a row does not depend on the launch or on its neighbours.
// Rows at or beyond num_ims[b] are not read (the training path computes padded rows: their dX means nothing) and get exact zeros.
// HBM-bound: 2 M D 4 bytes in, 8 M bytes out.
#include "common.h"
#include "lanes.h"

constexpr int SAL_WAVES = 4;        // rows per workgroup

__global__ void __launch_bounds__(SAL_WAVES * 64)
saliency_rows_kernel(const float* __restrict__ dx, int64_t ldd, const float* __restrict__ x, int64_t ldx,
                     const int64_t* __restrict__ num_ims, int rows_per_slide, int D, int64_t M, float* __restrict__ gxi,
                     float* __restrict__ gnorm) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * SAL_WAVES + (threadIdx.x >> 6);
  if (row >= M) return;                                            // (whole waves leave: row is uniform over a wave)
  const int64_t b = row / rows_per_slide;
  const bool valid = row - b * rows_per_slide < num_ims[b];
  float dot = 0.f, sq = 0.f;
  if (valid) {
    const float* g = dx + row * ldd;
    const float* v = x + row * ldx;
#pragma unroll 4
    for (int i = lane * 4; i < D; i += 256) {
      const f32x4 a = ldg_f32x4(g + i), c = ldg_f32x4(v + i);
      dot += (a[0] * c[0] + a[1] * c[1]) + (a[2] * c[2] + a[3] * c[3]);
      sq += (a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3]);
    }
    dot = wave_sum(dot);
    sq = wave_sum(sq);
  }
  if (lane == 0) {
    gxi[row] = dot;
    gnorm[row] = sqrtf(sq);
  }
}

extern "C" {

int paths_saliency_rows(const float* dx, int64_t ldd, const float* x, int64_t ldx, const int64_t* num_ims, int rows_per_slide, int D,
                        int B, float* gxi, float* gnorm, hipStream_t stream) {
  PATHS_REQUIRE(dx != nullptr && x != nullptr && num_ims != nullptr && gxi != nullptr && gnorm != nullptr,
                "saliency_rows: null pointer (dx, x, num_ims, gxi and gnorm are required)");
  PATHS_REQUIRE(D > 0 && D % 128 == 0, "saliency_rows: D (%d) must be a positive multiple of 128", D);
  PATHS_REQUIRE(B > 0 && rows_per_slide > 0, "saliency_rows: B (%d) and rows_per_slide (%d) must be positive", B, rows_per_slide);
  PATHS_REQUIRE(ldd >= D && ldx >= D && ldd % 4 == 0 && ldx % 4 == 0,
                "saliency_rows: row strides (%lld, %lld) must be multiples of 4 and at least D (%d)", (long long)ldd, (long long)ldx, D);
  PATHS_REQUIRE((uintptr_t)dx % 16 == 0 && (uintptr_t)x % 16 == 0, "saliency_rows: dx and x must be 16-byte aligned");
  const int64_t M = (int64_t)B * rows_per_slide;
  PATHS_REQUIRE((M + SAL_WAVES - 1) / SAL_WAVES <= 0x7fffffffLL, "saliency_rows: too many rows (%lld)", (long long)M);
  hipLaunchKernelGGL(saliency_rows_kernel, dim3((unsigned)((M + SAL_WAVES - 1) / SAL_WAVES)), dim3(SAL_WAVES * 64), 0, stream, dx, ldd,
                     x, ldx, num_ims, rows_per_slide, D, M, gxi, gnorm);
  PATHS_LAUNCH_CHECK("saliency_rows");
  return PATHS_OK;
}

}  // extern "C"
