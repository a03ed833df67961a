// Attention rollout of the special token (Abnar & Zuidema 2020; inference side path, not on the default launch sequence).
//
// Per slide, with T = num_ims + 1 valid tokens and A_l^h layer l's softmax attention of head h over the valid keys (valid query
// rows only, T x T, row-stochastic):
//   Â_l = 0.5 mean_h(A_l^h) + 0.5 I,      r = e_s^T Â_{L-1} ... Â_0.
// Evaluated from the last layer down: r = 0.5 e_s + 0.5 mean_h(a_{L-1}) from the last layer's token-0 attention (paths_token0_attention),
// then for l = L-2 .. 0:  r <- 0.5 r + 0.5 mean_h(r^T A_l^h).  The T x T matrices are never materialised:
//   prepare (layer l)   project   grid (T/64, H, B): Q_h (scaled by 1/sqrt(hd)) and K_h of the valid rows into the workspace (MFMA), rows in
//                                 CANONICAL order (row 0 = special token, row 1 + j = patch j: either token order maps onto it here);
//                                 the key bias is constant along a softmax row and cancels
//                       stats     grid (T/64, H, B): per query row i the softmax statistics (m_i, l_i) over the valid keys
//   seed                          grid (T/256, B): r from the last layer's token-0 attention
//   step (layer l)      columns   grid (T/64, B): r_out[j] = 0.5 r_in[j] + 0.5/H sum_h sum_i r_in[i] exp(s_ij - m_i) / l_i
//
// Scores run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: an exact fp32 k-ordered chain), S^T tiles of 16 keys x 16 queries
// (A = K rows, B = Q rows; lane (q = lane & 15, g = lane >> 4) holds keys 4g + r of query q, k = 16c + 4g + e in step (c, e)).  The
// stats and the column pass call the same tile routine on the same 16-aligned tiles, so s_ij is bit-identical in both and every row
// of P sums to 1 within rounding.  The column pass is key-block-major: a workgroup owns 64 keys and walks the heads and the query
// tiles in a fixed order with its column sums in registers, then one fixed butterfly over the 16 query lanes: no atomics, reruns
// are bit-identical.  Rows past num_ims[b] (clamped to [0, T-1] on the device) are never read: operand rows are clamped to the last
// valid row and their products discarded, so NaN in padding never reaches an exp.
#include "common.h"

#include <algorithm>
#include <math.h>

namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_BLOCK = 64;          // rows per workgroup: 4 waves x 16
constexpr int RO_D_MAX = 2048;

__host__ __device__ inline int ro_hdp(int hd) { return (hd + 15) / 16 * 16; }   // workspace row width: head_dim zero-padded to 16

__device__ __forceinline__ int ro_valid_last(const int64_t* num_ims, int b, int T) {
  const int64_t n = num_ims[b];
  return (int)(n < 0 ? 0 : (n > T - 1 ? T - 1 : n));
}

// four S^T tiles at once (independent accumulators): tile u = sum_k K[ka[u]][k] Q[qb[u]][k], each lane's rows given by the caller.
// SAME_K / SAME_Q: all four tiles share the K (step) or the Q (stats) operand, loaded once; the MFMA sequence is the same either way
template <bool SAME_K, bool SAME_Q>
__device__ __forceinline__ void ro_tiles4(const float* const ka[4], const float* const qb[4], int hdp, int g, f32x4 s[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < hdp; c += 16) {
    f32x4 a[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = (SAME_K && u > 0) ? a[0] : ldg_f32x4(ka[u] + c + 4 * g);
      q[u] = (SAME_Q && u > 0) ? q[0] : ldg_f32x4(qb[u] + c + 4 * g);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = mfma16(a[u][e], q[u][e], s[u]);
  }
}

// Q_h (scaled) | K_h of the valid rows on the f32-input MFMA: wave = 16 rows (A = x rows), 16-column tiles of the packed Q | K
// workspace row (B = in_proj rows, columns >= hd are zero), k = 16c + 4g + e as in ro_tiles4; lane (col, g) holds rows 4g + r
__global__ void __launch_bounds__(RO_THREADS)
rollout_project_kernel(const float* __restrict__ x, const int64_t* __restrict__ num_ims, const float* __restrict__ w_in,
                       const float* __restrict__ b_in, float* __restrict__ qk, int T, int d, int H, int special_last, float scale) {
  const int h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = ro_valid_last(num_ims, b, T);
  const int t0 = blockIdx.x * RO_BLOCK + wave * 16;
  if (t0 > n) return;                                             // padding rows: never read
  const int hd = d / H, hdp = ro_hdp(hd);
  const int ql = lane & 15, g = lane >> 4;
  const float* xr = x + ((int64_t)b * T + min(t0 + ql, n)) * d;   // (rows past n: clamped, products discarded)
  const int64_t kofs = (int64_t)gridDim.z * H * T * hdp;          // K follows Q
  float* base = qk + ((int64_t)b * H + h) * T * hdp;
  for (int ct = 0; ct < 2 * hdp; ct += 16) {
    const bool is_k = ct >= hdp;
    const int c = ct - (is_k ? hdp : 0) + ql;                     // this lane's output column
    const bool live = c < hd;
    const float* wr = w_in + (int64_t)((is_k ? d : 0) + h * hd + (live ? c : 0)) * d;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += 16) {
      const int kk = k0 + 4 * g;                                  // (d % 4 == 0: a 4-column group is wholly in or out)
      const f32x4 a = kk < d ? ldg_f32x4(xr + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
      const f32x4 w = kk < d ? ldg_f32x4(wr + kk) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = mfma16(a[e], w[e], acc);
    }
    const float bias = (live && !is_k) ? b_in[h * hd + c] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int t = t0 + 4 * g + r;
      if (t > n) continue;
      const int row = special_last ? (t == n ? 0 : t + 1) : t;    // canonical row
      base[(is_k ? kofs : 0) + (int64_t)row * hdp + c] = !live ? 0.f : (is_k ? acc[r] : (acc[r] + bias) * scale);
    }
  }
}

// (m, l) of every valid query row over the valid keys: wave = 16 queries, lane (q, g) runs an online (m, l) over keys 4g + r of
// each 64-key tile, then a fixed merge over the four lane groups
__device__ __forceinline__ void ro_merge(float& m, float& l, float m2, float l2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  l = (m == -INFINITY ? 0.f : l * expf(m - M)) + (m2 == -INFINITY ? 0.f : l2 * expf(m2 - M));
  m = M;
}

__global__ void __launch_bounds__(RO_THREADS)
rollout_stats_kernel(const int64_t* __restrict__ num_ims, float* __restrict__ ws, int T, int H, int hdp) {
  const int h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = ro_valid_last(num_ims, b, T);
  const int q0 = blockIdx.x * RO_BLOCK + wave * 16;
  if (q0 > n) return;
  const int ql = lane & 15, g = lane >> 4;
  const int64_t BHT = (int64_t)gridDim.z * H * T;
  const float* Q = ws + ((int64_t)b * H + h) * T * hdp;
  const float* K = Q + BHT * hdp;
  const float* qrow = Q + (int64_t)min(q0 + ql, n) * hdp;
  const float* qb[4] = {qrow, qrow, qrow, qrow};
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 <= n; k0 += RO_BLOCK) {
    const float* ka[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ka[u] = K + (int64_t)min(k0 + 16 * u + ql, n) * hdp;
    f32x4 s[4];
    ro_tiles4<false, true>(ka, qb, hdp, g, s);
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (k0 + 16 * u + 4 * g + r > n) s[u][r] = -INFINITY;
        mx = fmaxf(mx, s[u][r]);
      }
    if (mx == -INFINITY) continue;                                  // no valid key of this lane group in the tile
    const float m_new = fmaxf(m, mx);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum += s[u][r] == -INFINITY ? 0.f : expf(s[u][r] - m_new);
    l = (m == -INFINITY ? 0.f : l * expf(m - m_new)) + sum;
    m = m_new;
  }
  for (int o = 16; o < 64; o <<= 1) {
    const float m2 = __shfl_xor(m, o), l2 = __shfl_xor(l, o);
    ro_merge(m, l, m2, l2);
  }
  if (g == 0 && q0 + ql <= n) {
    float* st = ws + 2 * BHT * hdp;
    st[((int64_t)b * H + h) * T + q0 + ql] = m;
    st[BHT + ((int64_t)b * H + h) * T + q0 + ql] = l;
  }
}

// r (canonical rows) from the last layer's token-0 attention: r_0 = 0.5 + 0.5 mean_h(self), r_{1+j} = 0.5 mean_h(patch_j)
__global__ void __launch_bounds__(RO_THREADS)
rollout_seed_kernel(const float* __restrict__ attn_patch, int64_t patch_ld, const float* __restrict__ attn_self, int64_t self_ld,
                    const int64_t* __restrict__ num_ims, float* __restrict__ r, float* __restrict__ out, int64_t out_ld,
                    float* __restrict__ out_self, int T, int H) {
  const int b = blockIdx.y, c = blockIdx.x * RO_THREADS + threadIdx.x;
  if (c >= T) return;
  const int n = ro_valid_last(num_ims, b, T);
  float v = 0.f;
  if (c == 0) {
    float a = 0.f;
    for (int h = 0; h < H; ++h) a += attn_self[(int64_t)b * self_ld + h];
    v = 0.5f + 0.5f * (a / H);
  } else if (c <= n) {
    float a = 0.f;
    for (int h = 0; h < H; ++h) a += attn_patch[(int64_t)b * patch_ld + (int64_t)h * (T - 1) + c - 1];
    v = 0.5f * (a / H);
  }
  if (r != nullptr) r[(int64_t)b * T + c] = v;
  else if (c == 0) out_self[b] = v;
  else out[(int64_t)b * out_ld + c - 1] = v;
}

// one rollout step through a prepared layer: wave = 16 keys (A operand), lane (q, g) sums over the query rows q (mod 16) of
// every head, then a fixed butterfly over the 16 query lanes
__global__ void __launch_bounds__(RO_THREADS)
rollout_step_kernel(const float* __restrict__ ws, const int64_t* __restrict__ num_ims, const float* __restrict__ r_in,
                    float* __restrict__ r_out, float* __restrict__ out, int64_t out_ld, float* __restrict__ out_self, int T, int H, int hdp) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = ro_valid_last(num_ims, b, T);
  const int k0 = blockIdx.x * RO_BLOCK + wave * 16;
  const int ql = lane & 15, g = lane >> 4;
  const float* rin = r_in + (int64_t)b * T;
  float col[4] = {0.f, 0.f, 0.f, 0.f};
  if (k0 <= n) {
    const int64_t BHT = (int64_t)gridDim.y * H * T;
    for (int h = 0; h < H; ++h) {
      const float* Q = ws + ((int64_t)b * H + h) * T * hdp;
      const float* K = Q + BHT * hdp;
      const float* st_m = ws + 2 * BHT * hdp + ((int64_t)b * H + h) * T;
      const float* st_l = st_m + BHT;
      const float* krow = K + (int64_t)min(k0 + ql, n) * hdp;
      const float* ka[4] = {krow, krow, krow, krow};
      for (int q0 = 0; q0 <= n; q0 += RO_BLOCK) {
        const float* qb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) qb[u] = Q + (int64_t)min(q0 + 16 * u + ql, n) * hdp;
        f32x4 s[4];
        ro_tiles4<true, false>(ka, qb, hdp, g, s);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int q = q0 + 16 * u + ql;
          if (q <= n) {
            const float w = rin[q] / st_l[q], m = st_m[q];
#pragma unroll
            for (int r = 0; r < 4; ++r) col[r] = fmaf(w, expf(s[u][r] - m), col[r]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      for (int o = 1; o < 16; o <<= 1) col[r] += __shfl_xor(col[r], o);
  }
  if (ql != 0) return;
  const float half_h = 0.5f / H;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + 4 * g + r;
    if (k >= T) continue;
    const float v = k <= n ? fmaf(half_h, col[r], 0.5f * rin[k]) : 0.f;
    if (r_out != nullptr) r_out[(int64_t)b * T + k] = v;
    else if (k == 0) out_self[b] = v;
    else out[(int64_t)b * out_ld + k - 1] = v;
  }
}

}  // namespace

extern "C" {

// floats of one prepared layer: Q and K [B][H][T][hdp] (hdp = head_dim rounded up to 16) + softmax statistics m, l [B][H][T]
int64_t paths_attention_rollout_workspace(int B, int T, int d, int H) {
  if (B <= 0 || T <= 0 || d <= 0 || H <= 0 || d % H != 0) return 0;
  return (int64_t)B * H * T * (2 * ro_hdp(d / H) + 2);
}

// layer l's Q / K rows and softmax statistics from its input rows x [B, T, d] (token order special_last, as paths_token0_attention)
// and its true in_proj w_in [3d, d], b_in [3d]
int paths_attention_rollout_prepare(const float* x, const int64_t* num_ims, const float* w_in, const float* b_in, float* ws, int B, int T,
                                    int d, int H, int special_last, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && T > 0, "attention_rollout: B = %d and T = %d must be positive", B, T);
  PATHS_REQUIRE(H > 0 && d > 0 && d % H == 0, "attention_rollout: d %% H must be 0 (d = %d, H = %d)", d, H);
  PATHS_REQUIRE(d <= RO_D_MAX && d % 4 == 0, "attention_rollout: d = %d must be a multiple of 4 and d <= %d", d, RO_D_MAX);
  PATHS_REQUIRE(special_last == 0 || special_last == 1, "attention_rollout: special_last must be 0 or 1 (got %d)", special_last);
  PATHS_REQUIRE(x && num_ims && w_in && b_in && ws, "attention_rollout: null pointer");
  PATHS_REQUIRE(((uintptr_t)x | (uintptr_t)w_in | (uintptr_t)ws) % 16 == 0, "attention_rollout: x, w_in and ws must be 16-byte aligned");
  const int hd = d / H, hdp = ro_hdp(hd);
  const dim3 grid((T + RO_BLOCK - 1) / RO_BLOCK, H, B);
  const float scale = (float)(1.0 / sqrt((double)hd));
  hipLaunchKernelGGL(rollout_project_kernel, grid, dim3(RO_THREADS), 0, stream, x, num_ims, w_in, b_in, ws, T, d, H, special_last, scale);
  PATHS_LAUNCH_CHECK("attention_rollout(project)");
  hipLaunchKernelGGL(rollout_stats_kernel, grid, dim3(RO_THREADS), 0, stream, num_ims, ws, T, H, hdp);
  PATHS_LAUNCH_CHECK("attention_rollout(stats)");
  return PATHS_OK;
}

// r [B][T] (canonical rows: 0 = special token, 1 + j = patch j; 0 past num_ims) from the last layer's token-0 attention
// (attn_patch[b * patch_ld + h * (T-1) + j], attn_self[b * self_ld + h]: paths_token0_attention's layout).  r == nullptr: write the
// rollout itself instead (L = 1): rollout[b * rollout_ld + j], rollout_self[b]
int paths_attention_rollout_seed(const float* attn_patch, int64_t patch_ld, const float* attn_self, int64_t self_ld, const int64_t* num_ims,
                                 float* r, float* rollout, int64_t rollout_ld, float* rollout_self, int B, int T, int H, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && T > 0 && H > 0, "attention_rollout_seed: bad shape B = %d T = %d H = %d", B, T, H);
  PATHS_REQUIRE(attn_self && num_ims && (attn_patch || T == 1), "attention_rollout_seed: null pointer");
  PATHS_REQUIRE(r || (rollout_self && (rollout || T == 1)), "attention_rollout_seed: null pointer");
  PATHS_REQUIRE(patch_ld >= (int64_t)H * (T - 1) && self_ld >= H && (r || rollout_ld >= T - 1), "attention_rollout_seed: strides too small");
  hipLaunchKernelGGL(rollout_seed_kernel, dim3((T + RO_THREADS - 1) / RO_THREADS, B), dim3(RO_THREADS), 0, stream, attn_patch, patch_ld,
                     attn_self, self_ld, num_ims, r, rollout, rollout_ld, rollout_self, T, H);
  PATHS_LAUNCH_CHECK("attention_rollout(seed)");
  return PATHS_OK;
}

// r_out = 0.5 r_in + 0.5 mean_h(r_in^T A^h) through a layer prepared in ws (canonical rows, r_in 0 past num_ims is not required: rows
// past num_ims are never read).  r_out == nullptr: write the rollout itself (the last step): rollout[b * rollout_ld + j], rollout_self[b]
int paths_attention_rollout_step(const float* ws, const int64_t* num_ims, const float* r_in, float* r_out, float* rollout, int64_t rollout_ld,
                                 float* rollout_self, int B, int T, int d, int H, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && T > 0, "attention_rollout_step: B = %d and T = %d must be positive", B, T);
  PATHS_REQUIRE(H > 0 && d > 0 && d % H == 0, "attention_rollout_step: d %% H must be 0 (d = %d, H = %d)", d, H);
  PATHS_REQUIRE(d <= RO_D_MAX && d % 4 == 0, "attention_rollout_step: d = %d must be a multiple of 4 and d <= %d", d, RO_D_MAX);
  PATHS_REQUIRE(ws && num_ims && r_in && (r_out || (rollout_self && (rollout || T == 1))), "attention_rollout_step: null pointer");
  PATHS_REQUIRE((uintptr_t)ws % 16 == 0, "attention_rollout_step: ws must be 16-byte aligned");
  PATHS_REQUIRE(r_out || rollout_ld >= T - 1, "attention_rollout_step: rollout stride too small");
  hipLaunchKernelGGL(rollout_step_kernel, dim3((T + RO_BLOCK - 1) / RO_BLOCK, B), dim3(RO_THREADS), 0, stream, ws, num_ims, r_in, r_out,
                     rollout, rollout_ld, rollout_self, T, H, ro_hdp(d / H));
  PATHS_LAUNCH_CHECK("attention_rollout(step)");
  return PATHS_OK;
}

}  // extern "C"
