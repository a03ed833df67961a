// Gradient-weighted attention relevance of the special token (Chefer, Gur & Wolf, ICCV 2021, "Generic Attention-model
// Explainability"; attribution side path of the backward pass, not on the training launch sequence).
//
// Per slide, with T = num_ims + 1 valid tokens (row 0 = special token s, the training forward's order), A_l^h layer l's softmax
// attention of head h over the valid keys (valid query rows only) and gradA_l^h = d target / d A_l^h, entry (i, j) = dO_i^h . V_j^h
// (dO: gradient of the attention output in front of out_proj, V: value rows with bias):
//   Abar_l = mean_h (A_l^h * gradA_l^h)^+,      r = e_s^T (I + Abar_{L-1}) ... (I + Abar_0)
// (Chefer's rule R <- R + Abar R from R = I, read at the special token's row).  Evaluated from the last layer down, at the points
// of the hand-written backward where the operands are alive (paths_amd/backward.py:attention_relevance):
//   seed (last layer, read at token 0 only)   grid (T/256, B): r = e_s + mean_h (a0^h * (da0^h . V_j^h))^+, each key's probability
//                                             a0^h[j] = exp2(qscale q_0 . k_j - lse0) from the SAVED statistic (log2 domain): O(T d)
//   step (full layer l = L-2 .. 0)            grid (T/64, B): r_out[j] = r_in[j] + 1/H sum_h sum_i r_in[i] (A^h[i,j] gradA^h[i,j])^+
// A slide without patches (num_ims = 0) has nothing to attribute to: its r stays e_s through both (relevance_self exactly 1).
//
// The step is the T x T pass; no T x T matrix is stored.  Both score products run on the f32-input MFMA (v_mfma_f32_16x16x4_f32: an
// exact fp32 k-ordered chain), as transposed tiles of 16 keys x 16 queries: S^T = K Q^T and G^T = V dO^T (A = K / V rows, B = Q / dO
// rows; lane (q = lane & 15, g = lane >> 4) holds keys 4g + r of query q).  Key-block-major as csrc/attn_rollout.hip: a wave owns 16
// keys, its K and V fragments of the current head stay in registers, heads and query blocks are walked in a fixed order with the
// column sums in registers, then one fixed butterfly over the 16 query lanes: no atomics, no cross-workgroup waiting, reruns are
// bit-identical.  The query side (64 rows of Q and dO, r and lse) is staged in LDS once per (head, query block) and shared by the
// workgroup's four waves - the rollout step re-reads it from L2 for every 16 x 16 tile.
//
// Operands are addressed as base + b * sb + h * sh + t * st + e, so one kernel serves the shipped geometry's head-major [B, H, T, hd]
// (q pre-scaled, qscale = 1) and the shape-generic path's token-major qkv [B, T, 3 di] (bases at 0 / di / 2 di, qscale as its
// attention backward takes it).  Rows past num_ims[b] (clamped to [0, T-1] on the device) are never read: operand rows are clamped
// to the last valid row and their products discarded, so NaN in padding never reaches an exp2 or an output.
#include "common.h"

#include <math.h>

namespace {

constexpr int RV_THREADS = 256;
constexpr int RV_BLOCK = 64;          // keys per workgroup (4 waves x 16) = query rows per LDS stage

__device__ __forceinline__ int rv_valid_last(const int64_t* num_ims, int b, int T) {
  const int64_t n = num_ims[b];
  return (int)(n < 0 ? 0 : (n > T - 1 ? T - 1 : n));
}

// canonical row c of slide b: r [B][T], or the outputs (patch j = row 1 + j)
__device__ __forceinline__ void rv_store(float* r, float* out, int64_t out_ld, float* out_self, int b, int T, int c, float v) {
  if (r != nullptr) r[(int64_t)b * T + c] = v;
  else if (c == 0) out_self[b] = v;
  else out[(int64_t)b * out_ld + c - 1] = v;
}

__global__ void __launch_bounds__(RV_THREADS)
relevance_seed_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t sb, int64_t sh, int64_t st,
                      float qscale, const float* __restrict__ da0, int64_t da0_ld, const float* __restrict__ lse0, int64_t lse0_sb,
                      int64_t lse0_sh, const int64_t* __restrict__ num_ims, float* __restrict__ r, float* __restrict__ out, int64_t out_ld,
                      float* __restrict__ out_self, int T, int H, int hd) {
  const int b = blockIdx.y, j = blockIdx.x * RV_THREADS + threadIdx.x;
  if (j >= T) return;
  const int n = rv_valid_last(num_ims, b, T);
  float val = j == 0 ? 1.f : 0.f;
  if (j <= n && n > 0) {
    float acc = 0.f;
    for (int h = 0; h < H; ++h) {
      const float* q0 = q + b * sb + h * sh;                      // query row 0 = the special token
      const float* kr = k + b * sb + h * sh + j * st;
      const float* vr = v + b * sb + h * sh + j * st;
      const float* dr = da0 + b * da0_ld + (int64_t)h * hd;
      float s = 0.f, g = 0.f;
      for (int e = 0; e < hd; e += 4) {
        const f32x4 qq = ldg_f32x4(q0 + e), kk = ldg_f32x4(kr + e), vv = ldg_f32x4(vr + e), dd = ldg_f32x4(dr + e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s = fmaf(qq[i], kk[i], s);
          g = fmaf(dd[i], vv[i], g);
        }
      }
      const float p = __builtin_amdgcn_exp2f(fmaf(qscale, s, -lse0[b * lse0_sb + h * lse0_sh]));
      acc += fmaxf(0.f, p * g);
    }
    val += acc / H;
  }
  rv_store(r, out, out_ld, out_self, b, T, j, val);
}

template <int HD>
__global__ void __launch_bounds__(RV_THREADS)
relevance_step_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t sb, int64_t sh, int64_t st,
                      float qscale, const float* __restrict__ d_o, int64_t ld_o, const float* __restrict__ lse,
                      const int64_t* __restrict__ num_ims, const float* __restrict__ r_in, float* __restrict__ r_out, float* __restrict__ out,
                      int64_t out_ld, float* __restrict__ out_self, int T, int H) {
  constexpr int LDR = HD + 4;          // LDS row stride in floats (16-byte aligned rows, 128-byte-stride bank pattern broken)
  constexpr int NC = HD / 16;          // 16-wide k chunks of a row
  constexpr int V4 = HD / 4;           // float4s of a row
  __shared__ __attribute__((aligned(16))) float sQ[RV_BLOCK * LDR];
  __shared__ __attribute__((aligned(16))) float sG[RV_BLOCK * LDR];
  __shared__ float sW[RV_BLOCK], sL[RV_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = rv_valid_last(num_ims, b, T);
  const int kb0 = blockIdx.x * RV_BLOCK;
  const float* rin = r_in + (int64_t)b * T;
  if (kb0 > n || n == 0) {             // a block of padding keys, or a slide without patches (r stays as it is): no product
    if (tid < RV_BLOCK && kb0 + tid < T) rv_store(r_out, out, out_ld, out_self, b, T, kb0 + tid, kb0 + tid <= n ? rin[kb0 + tid] : 0.f);
    return;
  }
  const int k0 = kb0 + wave * 16;
  const bool live = k0 <= n;           // (a wave of padding keys still stages and meets the barriers)
  const int ql = lane & 15, g = lane >> 4;
  float col[4] = {0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < H; ++h) {
    const float* qh = q + b * sb + h * sh;
    const float* dh = d_o + (int64_t)b * T * ld_o + (int64_t)h * HD;
    const float* lh = lse + ((int64_t)b * H + h) * T;
    f32x4 kf[NC], vf[NC];
    if (live) {
      const int64_t ro = b * sb + h * sh + (int64_t)min(k0 + ql, n) * st;       // (keys past n: clamped, products discarded)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        kf[c] = ldg_f32x4(k + ro + 16 * c + 4 * g);
        vf[c] = ldg_f32x4(v + ro + 16 * c + 4 * g);
      }
    }
    for (int q0 = 0; q0 <= n; q0 += RV_BLOCK) {
      __syncthreads();                 // the previous stage has been read
      for (int idx = tid; idx < RV_BLOCK * V4; idx += RV_THREADS) {
        const int row = idx / V4, c4 = idx - row * V4;
        const int t = min(q0 + row, n);                                          // (rows past n: clamped, products discarded)
        *reinterpret_cast<f32x4*>(&sQ[row * LDR + 4 * c4]) = ldg_f32x4(qh + (int64_t)t * st + 4 * c4);
        *reinterpret_cast<f32x4*>(&sG[row * LDR + 4 * c4]) = ldg_f32x4(dh + (int64_t)t * ld_o + 4 * c4);
      }
      if (tid < RV_BLOCK) {
        const int t = q0 + tid;
        sW[tid] = t <= n ? rin[t] : 0.f;
        sL[tid] = lh[min(t, n)];
      }
      __syncthreads();
      if (!live) continue;
      f32x4 s[4], gr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] = gr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        f32x4 qf[4], df[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          qf[u] = *reinterpret_cast<const f32x4*>(&sQ[(16 * u + ql) * LDR + 16 * c + 4 * g]);
          df[u] = *reinterpret_cast<const f32x4*>(&sG[(16 * u + ql) * LDR + 16 * c + 4 * g]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            s[u] = mfma16(kf[c][e], qf[u][e], s[u]);
            gr[u] = mfma16(vf[c][e], df[u][e], gr[u]);
          }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (q0 + 16 * u + ql <= n) {
          const float w = sW[16 * u + ql], L = sL[16 * u + ql];
#pragma unroll
          for (int r = 0; r < 4; ++r)
            col[r] = fmaf(w, fmaxf(0.f, __builtin_amdgcn_exp2f(fmaf(qscale, s[u][r], -L)) * gr[u][r]), col[r]);
        }
      }
    }
  }
  if (!live) {                         // padding keys of a live block
    if (lane < 16 && k0 + lane < T) rv_store(r_out, out, out_ld, out_self, b, T, k0 + lane, 0.f);
    return;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    for (int o = 1; o < 16; o <<= 1) col[r] += __shfl_xor(col[r], o);
  if (ql != 0) return;
  const float inv_h = 1.0f / H;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kk = k0 + 4 * g + r;
    if (kk >= T) continue;
    rv_store(r_out, out, out_ld, out_self, b, T, kk, kk <= n ? fmaf(inv_h, col[r], rin[kk]) : 0.f);
  }
}

template <int HD>
void launch_step(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, float qscale, const float* d_o,
                 int64_t ld_o, const float* lse, const int64_t* num_ims, const float* r_in, float* r_out, float* out, int64_t out_ld,
                 float* out_self, int B, int T, int H, hipStream_t stream) {
  hipLaunchKernelGGL(relevance_step_kernel<HD>, dim3((T + RV_BLOCK - 1) / RV_BLOCK, B), dim3(RV_THREADS), 0, stream, q, k, v, sb, sh, st, qscale,
                     d_o, ld_o, lse, num_ims, r_in, r_out, out, out_ld, out_self, T, H);
}

bool rv_head_dim_ok(int hd) { return hd == 16 || hd == 32 || hd == 48 || hd == 64; }

}  // namespace

extern "C" {

int paths_attention_relevance_seed(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, float qscale,
                                   const float* da0, int64_t da0_ld, const float* lse0, int64_t lse0_sb, int64_t lse0_sh,
                                   const int64_t* num_ims, float* r, float* relevance, int64_t relevance_ld, float* relevance_self, int B,
                                   int T, int H, int head_dim, hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && T > 0 && H > 0, "attention_relevance_seed: bad shape B = %d T = %d H = %d", B, T, H);
  PATHS_REQUIRE(rv_head_dim_ok(head_dim), "attention_relevance_seed: head_dim must be 16, 32, 48 or 64 (got %d)", head_dim);
  PATHS_REQUIRE(q && k && v && da0 && lse0 && num_ims, "attention_relevance_seed: null pointer");
  PATHS_REQUIRE(r || (relevance_self && (relevance || T == 1)), "attention_relevance_seed: null pointer");
  PATHS_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)da0) % 16 == 0,
                "attention_relevance_seed: q, k, v and da0 must be 16-byte aligned");
  PATHS_REQUIRE(sb >= 0 && sh >= 0 && st >= head_dim && (sb | sh | st | da0_ld) % 4 == 0 && da0_ld >= (int64_t)H * head_dim,
                "attention_relevance_seed: operand strides must be multiples of 4 floats, the token stride and da0's row must hold a head");
  PATHS_REQUIRE(lse0_sb >= 0 && lse0_sh >= 0 && (r || relevance_ld >= T - 1), "attention_relevance_seed: strides too small");
  hipLaunchKernelGGL(relevance_seed_kernel, dim3((T + RV_THREADS - 1) / RV_THREADS, B), dim3(RV_THREADS), 0, stream, q, k, v, sb, sh, st, qscale,
                     da0, da0_ld, lse0, lse0_sb, lse0_sh, num_ims, r, relevance, relevance_ld, relevance_self, T, H, head_dim);
  PATHS_LAUNCH_CHECK("attention_relevance(seed)");
  return PATHS_OK;
}

int paths_attention_relevance_step(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, float qscale,
                                   const float* d_o, int64_t ld_o, const float* lse, const int64_t* num_ims, const float* r_in, float* r_out,
                                   float* relevance, int64_t relevance_ld, float* relevance_self, int B, int T, int H, int head_dim,
                                   hipStream_t stream) {
  PATHS_REQUIRE(B > 0 && T > 0 && H > 0, "attention_relevance_step: bad shape B = %d T = %d H = %d", B, T, H);
  PATHS_REQUIRE(rv_head_dim_ok(head_dim), "attention_relevance_step: head_dim must be 16, 32, 48 or 64 (got %d)", head_dim);
  PATHS_REQUIRE(q && k && v && d_o && lse && num_ims && r_in, "attention_relevance_step: null pointer");
  PATHS_REQUIRE(r_out || (relevance_self && (relevance || T == 1)), "attention_relevance_step: null pointer");
  PATHS_REQUIRE(r_out != r_in, "attention_relevance_step: r_out must not be r_in (every workgroup reads all of r_in)");
  PATHS_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)d_o) % 16 == 0,
                "attention_relevance_step: q, k, v and d_o must be 16-byte aligned");
  PATHS_REQUIRE(sb >= 0 && sh >= 0 && st >= head_dim && (sb | sh | st | ld_o) % 4 == 0 && ld_o >= (int64_t)H * head_dim,
                "attention_relevance_step: operand strides must be multiples of 4 floats, the token stride and d_o's row must hold a head");
  PATHS_REQUIRE(r_out || relevance_ld >= T - 1, "attention_relevance_step: relevance stride too small");
  switch (head_dim) {
    case 16: launch_step<16>(q, k, v, sb, sh, st, qscale, d_o, ld_o, lse, num_ims, r_in, r_out, relevance, relevance_ld, relevance_self, B, T, H, stream); break;
    case 32: launch_step<32>(q, k, v, sb, sh, st, qscale, d_o, ld_o, lse, num_ims, r_in, r_out, relevance, relevance_ld, relevance_self, B, T, H, stream); break;
    case 48: launch_step<48>(q, k, v, sb, sh, st, qscale, d_o, ld_o, lse, num_ims, r_in, r_out, relevance, relevance_ld, relevance_self, B, T, H, stream); break;
    default: launch_step<64>(q, k, v, sb, sh, st, qscale, d_o, ld_o, lse, num_ims, r_in, r_out, relevance, relevance_ld, relevance_self, B, T, H, stream); break;
  }
  PATHS_LAUNCH_CHECK("attention_relevance(step)");
  return PATHS_OK;
}

}  // extern "C"
