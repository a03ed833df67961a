// The per-row kernels of the patch attributions (paths_amd/saliency.py), all on the skeleton of path_row.h: ONE wave per recorded row
// (b, r), four rows per workgroup, 16-byte loads and stores.  Every lane sums its columns in ascending order and the 64 partial sums
// meet in a fixed butterfly (registers only: no LDS, no atomics, no workspace): a row's result does not depend on the launch, on its
// neighbours or on how the members were cut into chunks.  Rows at or beyond num_ims[b] are not read (the training path computes
// padded rows: their dX means nothing); they get exact zeros.  All HBM-bound.
//
// paths_saliency_rows (input_gradients): per-patch reductions of the feature gradient.  2 M D 4 bytes in, 8 M bytes out.
//   gxi[r] = sum_d dX[r,d] X[r,d]  (gradient x input)     gnorm[r] = sqrt(sum_d dX[r,d]^2)  (gradient norm)
//
// paths_path_points / paths_path_accumulate (integrated_gradients, smooth_grad): C chunk members of B slides run as B * C
// virtual slides (virtual slide v = c * B + b); a wave loops over the members of its row in ascending c.
//   points:     out[v,r,:] = fmaf(alpha[c], x[b,r,:] - base, base) + sigma[c] * rms(x[b,r,:]) * z(keys[v], r * D + d)
//   accumulate: acc_gxi[b,r] (+)= sum_c w[c] sum_d dx[v,r,d] (x[b,r,d] - base[d]),  acc_sq[b,r] (+)= sum_c w[c] sum_d dx[v,r,d]^2,
//               acc_dx[b,r,:] (+)= sum_c w[c] dx[v,r,:]
// The Gaussian draw is a function of (key, element) alone.  Padded rows - points: always zeros; accumulate: with init, else they are
// left alone.  points: M D 4 bytes in (x; re-read per member from cache), C M D 4 bytes out.  accumulate: (C + 1) M D 4 bytes in,
// 8 M bytes out (+ 8 M in without init); with acc_dx M D 4 more out (and in without init; dx is re-read from cache).
//
// paths_path_mask_points (perturbation_curves): the sibling of paths_path_points with the same layout.  A member's row is
// the recorded row or the baseline, chosen by the row's rank against the member's threshold: a copy, no arithmetic on the values.
// M D 4 bytes in (re-read per member from cache), C M D 4 bytes out.
#include "path_row.h"
#include "dropout.h"
#include "lanes.h"

__global__ void __launch_bounds__(ROW_WAVES * 64)
saliency_rows_kernel(const float* __restrict__ dx, int64_t ldd, const float* __restrict__ x, int64_t ldx,
                     const int64_t* __restrict__ num_ims, int rows_per_slide, int D, int64_t M, float* __restrict__ gxi,
                     float* __restrict__ gnorm) {
  const int lane = threadIdx.x & 63;
  int64_t row, b, r;
  bool padded;
  if (!row_of_wave(num_ims, rows_per_slide, M, row, b, r, padded)) return;
  float dot = 0.f, sq = 0.f;
  if (!padded) {
    const float* g = dx + row * ldd;
    const float* v = x + row * ldx;
#pragma unroll 4
    for (int i = lane * 4; i < D; i += 256) {        // (row_dot_sq's loop, written out: inlined from there it compiles to other code)
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

// The Box-Muller pair of elements (e, e + 1), e even:  u1 = ((h0 >> 8) + 0.5) 2^-24 in (0, 1),  u2 = (h1 >> 8) 2^-24 in [0, 1),
// (z0, z1) = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2).  k + 0.5 has 25 significant bits for k >= 2^23: there ln u1 is taken as
// log1p(-(1 - u1)) with 1 - u1 = ((2^24 - k) - 0.5) 2^-24 exact, so the radius keeps its relative accuracy where u1 -> 1 (a rounded
// u1 = 1 would give radius 0 for 2.4e-4).  The angle is formed as pi * (2 u2) (2 u2 is exact): no rounding of 2 pi u2.
__device__ __forceinline__ void gauss_pair(uint64_t e_even, uint32_t key_lo, uint32_t key_hi, float& z0, float& z1) {
  const uint32_t k = drop_hash(e_even, key_lo, key_hi) >> 8;
  const uint32_t j = drop_hash(e_even | 1ull, key_lo, key_hi) >> 8;
  const float ln_u1 = k < (1u << 23) ? logf(((float)k + 0.5f) * 0x1p-24f) : log1pf(-(((float)((1u << 24) - k) - 0.5f) * 0x1p-24f));
  const float rad = sqrtf(-2.0f * ln_u1);
  float s, c;
  sincospif((float)j * 0x1p-23f, &s, &c);
  z0 = rad * c;
  z1 = rad * s;
}

__global__ void __launch_bounds__(ROW_WAVES * 64)
path_points_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ base, const float* __restrict__ alpha,
                   const float* __restrict__ sigma, const uint64_t* __restrict__ keys, const int64_t* __restrict__ num_ims,
                   int rows_per_slide, int D, int B, int C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t M = (int64_t)B * rows_per_slide;
  int64_t row, b, r;
  bool padded;
  if (!row_of_wave(num_ims, rows_per_slide, M, row, b, r, padded)) return;
  if (padded) {
    zero_row(out, C, M, row, D, lane);
    return;
  }
  const float* v = x + row * ldx;
  bool noisy = false;
  for (int c = 0; c < C; ++c) noisy = noisy || sigma[c] != 0.f;
  float rms = 0.f;
  if (noisy) {
    float dot = 0.f, sq = 0.f;
    row_dot_sq(v, v, nullptr, D, lane, dot, sq);
    rms = sqrtf(wave_sum(sq) / (float)D);
  }
  for (int c = 0; c < C; ++c) {
    const float al = alpha[c], sg = sigma[c] * rms;
    const bool noise = sigma[c] != 0.f;
    const uint64_t key = keys != nullptr ? keys[(int64_t)c * B + b] : 0ull;
    const uint32_t key_lo = (uint32_t)key, key_hi = (uint32_t)(key >> 32);
    float* o = out + ((int64_t)c * M + row) * D;
    for (int i = lane * 4; i < D; i += 256) {
      const f32x4 a = ldg_f32x4(v + i);
      f32x4 p;
      if (base != nullptr) {
        const f32x4 bs = ldg_f32x4(base + i);
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = fmaf(al, a[q] - bs[q], bs[q]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = al * a[q];
      }
      if (noise) {
        const uint64_t e = (uint64_t)r * (uint64_t)D + (uint64_t)i;        // even: D and i are multiples of 4
        float z0, z1, z2, z3;
        gauss_pair(e, key_lo, key_hi, z0, z1);
        gauss_pair(e + 2, key_lo, key_hi, z2, z3);
        p[0] = fmaf(sg, z0, p[0]);
        p[1] = fmaf(sg, z1, p[1]);
        p[2] = fmaf(sg, z2, p[2]);
        p[3] = fmaf(sg, z3, p[3]);
      }
      stg_f32x4(o + i, p);
    }
  }
}

__global__ void __launch_bounds__(ROW_WAVES * 64)
path_accumulate_kernel(const float* __restrict__ dx, int64_t ldd, const float* __restrict__ x, int64_t ldx,
                       const float* __restrict__ base, const float* __restrict__ w, const int64_t* __restrict__ num_ims,
                       int rows_per_slide, int D, int B, int C, int init, float* __restrict__ acc_gxi, float* __restrict__ acc_sq,
                       float* __restrict__ acc_dx) {
  const int lane = threadIdx.x & 63;
  const int64_t M = (int64_t)B * rows_per_slide;
  int64_t row, b, r;
  bool padded;
  if (!row_of_wave(num_ims, rows_per_slide, M, row, b, r, padded)) return;
  if (padded) {
    if (init) {
      if (lane == 0) {
        acc_gxi[row] = 0.f;
        acc_sq[row] = 0.f;
      }
      if (acc_dx != nullptr) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int i = lane * 4; i < D; i += 256) stg_f32x4(acc_dx + row * D + i, zero);
      }
    }
    return;
  }
  const float* v = x + row * ldx;
  float gxi = init ? 0.f : acc_gxi[row];
  float sqs = init ? 0.f : acc_sq[row];
  for (int c = 0; c < C; ++c) {
    float dot = 0.f, sq = 0.f;
    row_dot_sq(dx + ((int64_t)c * M + row) * ldd, v, base, D, lane, dot, sq);
    gxi += w[c] * wave_sum(dot);
    sqs += w[c] * wave_sum(sq);
  }
  if (lane == 0) {
    acc_gxi[row] = gxi;
    acc_sq[row] = sqs;
  }
  if (acc_dx != nullptr) {
    float* o = acc_dx + row * D;
    for (int i = lane * 4; i < D; i += 256) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      if (!init) s = ldg_f32x4(o + i);
      for (int c = 0; c < C; ++c) s += w[c] * ldg_f32x4(dx + ((int64_t)c * M + row) * ldd + i);
      stg_f32x4(o + i, s);
    }
  }
}

__global__ void __launch_bounds__(ROW_WAVES * 64)
path_mask_points_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ base, const int* __restrict__ rank,
                        int64_t ldr, const int* __restrict__ thr, const int* __restrict__ insert, const int64_t* __restrict__ num_ims,
                        int rows_per_slide, int D, int B, int C, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t M = (int64_t)B * rows_per_slide;
  int64_t row, b, r;
  bool padded;
  if (!row_of_wave(num_ims, rows_per_slide, M, row, b, r, padded)) return;
  if (padded) {
    zero_row(out, C, M, row, D, lane);
    return;
  }
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int rk = rank[b * ldr + r];
  const float* v = x + row * ldx;
  for (int c = 0; c < C; ++c) {
    const int t = thr[(int64_t)c * B + b];
    const bool keep = rk < 0 || (insert[c] != 0 ? rk < t : rk >= t);        // (uniform over the wave)
    float* o = out + ((int64_t)c * M + row) * D;
    if (keep) {
      for (int i = lane * 4; i < D; i += 256) stg_f32x4(o + i, ldg_f32x4(v + i));
    } else if (base != nullptr) {
      for (int i = lane * 4; i < D; i += 256) stg_f32x4(o + i, ldg_f32x4(base + i));
    } else {
      for (int i = lane * 4; i < D; i += 256) stg_f32x4(o + i, zero);
    }
  }
}

extern "C" {

int paths_saliency_rows(const float* dx, int64_t ldd, const float* x, int64_t ldx, const int64_t* num_ims, int rows_per_slide, int D,
                        int B, float* gxi, float* gnorm, hipStream_t stream) {
  PATHS_REQUIRE(dx != nullptr && x != nullptr && num_ims != nullptr && gxi != nullptr && gnorm != nullptr,
                "saliency_rows: null pointer (dx, x, num_ims, gxi and gnorm are required)");
  if (const int rc = path_rows_check("saliency_rows", D, B, 1, rows_per_slide, {ldd, ldx}, {dx, x}, "dx and x"); rc != PATHS_OK) return rc;
  hipLaunchKernelGGL(saliency_rows_kernel, path_rows_grid(B, rows_per_slide), dim3(ROW_WAVES * 64), 0, stream, dx, ldd, x, ldx, num_ims,
                     rows_per_slide, D, (int64_t)B * rows_per_slide, gxi, gnorm);
  PATHS_LAUNCH_CHECK("saliency_rows");
  return PATHS_OK;
}

int paths_path_points(const float* x, int64_t ldx, const float* base, const float* alpha, const float* sigma, const uint64_t* keys,
                      const int64_t* num_ims, int rows_per_slide, int D, int B, int C, float* out, hipStream_t stream) {
  PATHS_REQUIRE(x != nullptr && alpha != nullptr && sigma != nullptr && num_ims != nullptr && out != nullptr,
                "path_points: null pointer (x, alpha, sigma, num_ims and out are required; keys wherever a sigma is not 0)");
  if (const int rc = path_rows_check("path_points", D, B, C, rows_per_slide, {ldx}, {x, base, out}, "x, base and out"); rc != PATHS_OK) return rc;
  hipLaunchKernelGGL(path_points_kernel, path_rows_grid(B, rows_per_slide), dim3(ROW_WAVES * 64), 0, stream, x, ldx, base, alpha, sigma,
                     keys, num_ims, rows_per_slide, D, B, C, out);
  PATHS_LAUNCH_CHECK("path_points");
  return PATHS_OK;
}

int paths_path_accumulate(const float* dx, int64_t ldd, const float* x, int64_t ldx, const float* base, const float* w,
                          const int64_t* num_ims, int rows_per_slide, int D, int B, int C, int init, float* acc_gxi, float* acc_sq,
                          float* acc_dx, hipStream_t stream) {
  PATHS_REQUIRE(dx != nullptr && x != nullptr && w != nullptr && num_ims != nullptr && acc_gxi != nullptr && acc_sq != nullptr,
                "path_accumulate: null pointer (dx, x, w, num_ims, acc_gxi and acc_sq are required)");
  if (const int rc = path_rows_check("path_accumulate", D, B, C, rows_per_slide, {ldd, ldx}, {dx, x, base, acc_dx}, "dx, x, base and acc_dx"); rc != PATHS_OK) return rc;
  hipLaunchKernelGGL(path_accumulate_kernel, path_rows_grid(B, rows_per_slide), dim3(ROW_WAVES * 64), 0, stream, dx, ldd, x, ldx, base, w,
                     num_ims, rows_per_slide, D, B, C, init, acc_gxi, acc_sq, acc_dx);
  PATHS_LAUNCH_CHECK("path_accumulate");
  return PATHS_OK;
}

int paths_path_mask_points(const float* x, int64_t ldx, const float* base, const int* rank, int64_t ldr, const int* thr, const int* insert,
                           const int64_t* num_ims, int rows_per_slide, int D, int B, int C, float* out, hipStream_t stream) {
  PATHS_REQUIRE(x != nullptr && rank != nullptr && thr != nullptr && insert != nullptr && num_ims != nullptr && out != nullptr,
                "path_mask_points: null pointer (x, rank, thr, insert, num_ims and out are required)");
  if (const int rc = path_rows_check("path_mask_points", D, B, C, rows_per_slide, {ldx}, {x, base, out}, "x, base and out"); rc != PATHS_OK) return rc;
  PATHS_REQUIRE(ldr >= rows_per_slide, "path_mask_points: rank stride (%lld) must be at least rows_per_slide (%d)", (long long)ldr,
                rows_per_slide);
  PATHS_REQUIRE((uintptr_t)rank % 4 == 0 && (uintptr_t)thr % 4 == 0 && (uintptr_t)insert % 4 == 0,
                "path_mask_points: rank, thr and insert must be 4-byte aligned");
  hipLaunchKernelGGL(path_mask_points_kernel, path_rows_grid(B, rows_per_slide), dim3(ROW_WAVES * 64), 0, stream, x, ldx, base, rank, ldr,
                     thr, insert, num_ims, rows_per_slide, D, B, C, out);
  PATHS_LAUNCH_CHECK("path_mask_points");
  return PATHS_OK;
}

}  // extern "C"
