// Masked self-attention with fp8 (OCP e4m3) operands on the CDNA4 matrix cores: the low-precision variant BASELINE.json configs[4]
// names for the stress geometry (one level, 8192 patches -> 8193 tokens of full quadratic attention).  NOT the product path: an
// e4m3 operand has 4 significant bits, the result misses the 1e-4 logit bar of the north star by two orders of magnitude (the
// measured error is printed by `bench.py --mode stress --fp8` and asserted loosely in tests/test_gpu_parity.py); it exists so that
// the cost / accuracy trade of that config is measured rather than guessed.  Opt-in: PATHS_ATTN_FP8=1 or ops.ATTN_FP8 = True.
//
// Same contract and the same structure as attn_x6.hip (reference model/aggregator.py:70-72 + utils.py:97-103; q pre-scaled by
// log2(e)/sqrt(hd); keys >= num_ims[b]+1 masked; one wave = 32 queries, a 4-wave workgroup shares 64-key K / V^T fragment sets
// through LDS, S(k+1) issued before the softmax of S(k), P never leaves the registers), with ONE v_mfma_f32_16x16x32_fp8_fp8 where
// the split kernels issue 3 (fp16 hi|lo) or 6 (bf16 hi|mid|lo), 8-byte fragments per lane instead of 16 x planes, and no operand
// split of P in the loop.  Scaling: q_s, k, v are O(1) and go to e4m3 as they are (saturated at +-448); P in [0, 1] is multiplied
// by 256 before the conversion (e4m3's normal range starts at 2^-6) and the 1/256 is folded into the final normalisation; the row
// sum l is accumulated in fp32 from the unquantised probabilities.
#include "common.h"
#include "lanes.h"

namespace {

constexpr int F8 = 512;                    // bytes of one 16-row x 32-k fp8 fragment (64 lanes x 8 bytes)
constexpr int KSTEP = 64;                  // keys per LDS buffer
// QT = 16-query tiles per wave: 2 up to head_dim 64; 1 for wide heads (head_dim 128 .. 384: the output accumulators alone are
// HD / 4 registers per query tile, and the K / V^T fragment sets of a 64-key step grow to 24 KB each at 384)
constexpr float P_SCALE = 256.0f;

__device__ __forceinline__ u32x2 fp8x8(const float (&x)[8], float scale) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] * scale, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}
__device__ __forceinline__ long as_long(u32x2 v) { return __builtin_bit_cast(long, v); }
__device__ __forceinline__ f32x4 mfma8(long a, long b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }

// Fragment images per (slide, head), Tp = T rounded up to 64 (the lane maps of attn_x6.hip, 8 bytes per lane), NK = HD / 32 k-steps,
// NDV = HD / 16 output-dim tiles:
//   Q8 / K8 : [Tp/16 tiles][NK][64 lanes][8 fp8]      lane (r = l&15, g = l>>4): token 16 tile + r, dims 32 kk + 8g .. + 7
//   V8      : [Tp/32 groups][NDV][64 lanes][8]         lane (dv = l&15, g): dim 16 dvt + dv, keys 32 grp + 4g + (j&3) + 16 (j>>2)
// Element (b, head, token, c) of q / k / v sits at base + b * bstride + head * hstride + token * ld + c: head-major [B][H][T][HD]
// (ld = HD, the layout paths_token_layer_f32 writes, q pre-scaled: qmul = 1) or token-major in_proj output [B*T, 3d] (ld = 3d, hstride = HD,
// q unscaled: qmul = log2(e) / sqrt(HD)).
template <int HD>
__global__ void __launch_bounds__(256)
attn_fp8_prep_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, int64_t ld, int64_t hstride,
                     int64_t bstride, float qmul, char* __restrict__ q8, char* __restrict__ k8, char* __restrict__ v8,
                     const int64_t* __restrict__ num_ims, int T, int Tp, int H) {
  constexpr int NK = HD / 32, NDV = HD / 16;
  extern __shared__ __attribute__((aligned(16))) char smem_prep[];
  float (*sv)[HD + 1] = reinterpret_cast<float (*)[HD + 1]>(smem_prep);          // [KSTEP][HD + 1]
  const int b = blockIdx.z, head = blockIdx.y, t0 = blockIdx.x * KSTEP;
  const int len = min((int)num_ims[b] + 1, T);
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)b * bstride + (int64_t)head * hstride;
  const int64_t ibase = ((int64_t)b * H + head) * (int64_t)Tp * HD;
  {
    const int tl = tid >> 2, g = tid & 3, tok = t0 + tl;
    const bool kvalid = tok < len, qvalid = tok < T;
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
      float xq[8], xk[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xk[i] = kvalid ? k[base + (int64_t)tok * ld + 32 * kk + 8 * g + i] : 0.f;
        xq[i] = qvalid ? q[base + (int64_t)tok * ld + 32 * kk + 8 * g + i] : 0.f;
      }
      const int64_t off = ibase + ((int64_t)(tok >> 4) * NK + kk) * F8 + ((tok & 15) + 16 * g) * 8;
      *reinterpret_cast<u32x2*>(k8 + off) = fp8x8(xk, 1.0f);
      *reinterpret_cast<u32x2*>(q8 + off) = fp8x8(xq, qmul);
    }
  }
#pragma unroll
  for (int p = 0; p < KSTEP * HD / 256; ++p) {
    const int idx = tid + 256 * p, tl = idx / HD, dcol = idx % HD, tok = t0 + tl;
    sv[tl][dcol] = tok < len ? v[base + (int64_t)tok * ld + dcol] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int job = tid; job < 2 * NDV * 64; job += 256) {
    const int kg = job / (NDV * 64), dvt = (job / 64) % NDV, l = job & 63, dv = l & 15, g = l >> 4;
    float xv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) xv[j] = sv[32 * kg + 4 * g + (j & 3) + 16 * (j >> 2)][16 * dvt + dv];
    const int64_t off = ibase + (int64_t)(((t0 >> 5) + kg) * NDV + dvt) * F8 + l * 8;
    *reinterpret_cast<u32x2*>(v8 + off) = fp8x8(xv, 1.0f);
  }
}

template <int HD, int QT>
__global__ void __launch_bounds__(256, HD <= 64 ? 2 : 1)
attn_fp8_kernel(const char* __restrict__ q8, const char* __restrict__ k8, const char* __restrict__ v8,
                float* __restrict__ o, const int64_t* __restrict__ num_ims, int T, int Tp, int H, int npairs, int nqb) {
  constexpr int NK = HD / 32, NDV = HD / 16;
  constexpr int KB = 4 * NK * F8, VB = 2 * NDV * F8;      // bytes of K / V^T fragments per 64-key step
  extern __shared__ __attribute__((aligned(16))) char smem_attn[];              // sKb [2][KB] | sVb [2][VB]
  char (*sKb)[KB] = reinterpret_cast<char (*)[KB]>(smem_attn);
  char (*sVb)[VB] = reinterpret_cast<char (*)[VB]>(smem_attn + 2 * KB);
  // XCD-aware placement as in attn_x6.hip: pair p only ever runs on the XCD group p % 8
  const int lin = blockIdx.x, xg = lin & 7, jx = lin >> 3;
  const int cnt = (npairs - xg + 7) >> 3;
  if (cnt <= 0) return;
  const int pair = xg + 8 * (jx % cnt), qb = jx / cnt;
  if (qb >= nqb) return;
  const int b = pair / H, head = pair - b * H, q0 = qb * 64 * QT;
  const int len = min((int)num_ims[b] + 1, T);
  if (q0 >= len) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ql = lane & 15, g4 = lane >> 4;
  const int64_t ibase = ((int64_t)b * H + head) * (int64_t)Tp * HD;
  const int qw = q0 + wave * 16 * QT;

  long qf[QT][NK];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int kk = 0; kk < NK; ++kk)
      qf[qt][kk] = *reinterpret_cast<const long*>(q8 + ibase + ((int64_t)(min(qw + 16 * qt, Tp - 16) >> 4) * NK + kk) * F8 + lane * 8);
  f32x4 oacc[NDV][QT];
#pragma unroll
  for (int i = 0; i < NDV; ++i)
#pragma unroll
    for (int j = 0; j < QT; ++j) oacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int j = 0; j < QT; ++j) { m_run[j] = -INFINITY; l_run[j] = 0.f; }

  // staging: threads 0-127 carry the K fragments of a 64-key step (one step ahead), 128-255 its V^T fragments: NK 16-byte pieces each
  const int nkt = (len + KSTEP - 1) / KSTEP;
  const bool carriesK = tid < 128;
  const int chunk = (tid & 127) * 16;
  u32x4 st[NK];
  auto gload = [&](int ktk, int ktv) {        // K of step ktk / V of step ktv (the caller checks the ranges)
    const char* src = carriesK ? k8 + ibase + (int64_t)ktk * KB : v8 + ibase + (int64_t)ktv * VB;
#pragma unroll
    for (int c = 0; c < NK; ++c) st[c] = *reinterpret_cast<const u32x4*>(src + chunk + 2048 * c);
  };
  auto swrite = [&](int ktk, int ktv, bool dok, bool dov) {
#pragma unroll
    for (int c = 0; c < NK; ++c) {
      if (carriesK) { if (dok) *reinterpret_cast<u32x4*>(&sKb[ktk & 1][chunk + 2048 * c]) = st[c]; }
      else if (dov) *reinterpret_cast<u32x4*>(&sVb[ktv & 1][chunk + 2048 * c]) = st[c];
    }
  };
  auto qk = [&](int kt, f32x4 (&s)[QT][4]) __attribute__((always_inline)) {
    const char* sK = &sKb[kt & 1][lane * 8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int kk = 0; kk < NK; ++kk) {
        const long kf = *reinterpret_cast<const long*>(sK + (t * NK + kk) * F8);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) s[qt][t] = mfma8(kf, qf[qt][kk], kk == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : s[qt][t]);
      }
    }
  };
  gload(0, 0);
  swrite(0, 0, true, true);
  if (nkt > 1) { if (carriesK) gload(1, 0); swrite(1, 0, true, false); }
  __syncthreads();
  f32x4 sA[QT][4], sB[QT][4];
  qk(0, sA);
  auto step = [&](int kt, f32x4 (&s)[QT][4], f32x4 (&sn)[QT][4], bool last) __attribute__((always_inline)) {
    const bool morek = kt + 2 < nkt, morev = kt + 1 < nkt;
    if (carriesK ? morek : morev) gload(kt + 2, kt + 1);
    const char* sV = &sVb[kt & 1][lane * 8];
    if (last) {
      const int kbase = kt * KSTEP + 4 * g4;
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kbase + 16 * t + r >= len) s[qt][t][r] = -INFINITY;
    }
    qk(kt + 1, sn);                                     // (past the end: stale K fragments, finite garbage nobody reads)
    long pf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mx = fmaxf(fmaxf(mx, s[qt][t][0]), s[qt][t][1]);
        mx = fmaxf(fmaxf(mx, s[qt][t][2]), s[qt][t][3]);
      }
      mx = rows_max(mx);
      const float m_new = fmaxf(m_run[qt], mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);
      float psum = 0.f;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        float pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                   // k-slot (g4, j) of the PV product = key 4 g4 + (j&3) + 16 (j>>2) of the group
          pv[j] = __builtin_amdgcn_exp2f(s[qt][2 * kg + (j >> 2)][j & 3] - m_new);
          psum += pv[j];
        }
        pf[qt][kg] = as_long(fp8x8(pv, P_SCALE));
      }
      l_run[qt] = l_run[qt] * alpha + psum;
      m_run[qt] = m_new;
#pragma unroll
      for (int dvt = 0; dvt < NDV; ++dvt) oacc[dvt][qt] *= alpha;
    }
#pragma unroll
    for (int kg = 0; kg < 2; ++kg)
#pragma unroll
      for (int dvt = 0; dvt < NDV; ++dvt) {
        const long vf = *reinterpret_cast<const long*>(sV + (kg * NDV + dvt) * F8);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) oacc[dvt][qt] = mfma8(vf, pf[qt][kg], oacc[dvt][qt]);
      }
    swrite(kt + 2, kt + 1, morek, morev);               // K over K(kt) (read one step ago), V over V(kt-1)
    __syncthreads();
  };
  {
    int kt = 0;
    for (; kt + 2 < nkt; kt += 2) {
      step(kt, sA, sB, false);
      step(kt + 1, sB, sA, false);
    }
    if (kt + 1 < nkt) { step(kt, sA, sB, false); step(kt + 1, sB, sA, true); }
    else step(kt, sA, sB, true);
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float l = rows_sum(l_run[qt]);
    const float inv = 1.0f / (l * P_SCALE);
    const int qi = qw + 16 * qt + ql;
    if (qi < T) {
      float* op = o + ((int64_t)b * T + qi) * (H * HD) + head * HD + 4 * g4;
#pragma unroll
      for (int dvt = 0; dvt < NDV; ++dvt) *reinterpret_cast<f32x4*>(op + 16 * dvt) = oacc[dvt][qt] * inv;
    }
  }
}

template <int HD>
int launch_fp8(const float* q, const float* k, const float* v, int64_t ld, int64_t hstride, int64_t bstride, float qmul, float* o,
               const int64_t* num_ims, int B, int T, int H, void* workspace, hipStream_t stream) {
  constexpr int QT = HD <= 64 ? 2 : 1;
  constexpr size_t lds_prep = (size_t)KSTEP * (HD + 1) * sizeof(float), lds_attn = 2ull * (4 * (HD / 32) * F8 + 2 * (HD / 16) * F8);
  PATHS_LDS_OPT_IN((attn_fp8_prep_kernel<HD>), lds_prep, "attention_fp8(prep)");
  PATHS_LDS_OPT_IN((attn_fp8_kernel<HD, QT>), lds_attn, "attention_fp8");
  const int Tp = (T + KSTEP - 1) / KSTEP * KSTEP;
  const int64_t img = (int64_t)B * H * Tp * HD;
  char* q8 = reinterpret_cast<char*>(workspace);
  char* k8 = q8 + img;
  char* v8 = k8 + img;
  hipLaunchKernelGGL(attn_fp8_prep_kernel<HD>, dim3(Tp / KSTEP, H, B), dim3(256), lds_prep, stream, q, k, v, ld, hstride, bstride, qmul, q8, k8, v8,
                     num_ims, T, Tp, H);
  PATHS_LAUNCH_CHECK("attention_fp8(prep)");
  const int nqb = (T + 64 * QT - 1) / (64 * QT), npairs = H * B;
  hipLaunchKernelGGL((attn_fp8_kernel<HD, QT>), dim3(8 * ((npairs + 7) / 8) * nqb), dim3(256), lds_attn, stream, q8, k8, v8, o, num_ims, T, Tp, H, npairs, nqb);
  PATHS_LAUNCH_CHECK("attention_fp8");
  return PATHS_OK;
}

inline bool fp8_head_dim_ok(int hd) { return hd == 32 || hd == 64 || hd == 128 || hd == 256 || hd == 384; }
// head_dim 128 / 256 / 384 (round 5: the stress row's own 1536 / 4 heads form): the same kernel with 4 / 8 / 12 k-steps per
// score tile and 8 / 16 / 24 output-dim tiles, one 16-query tile per wave
int dispatch_fp8(int hd, const float* q, const float* k, const float* v, int64_t ld, int64_t hstride, int64_t bstride, float qmul, float* o,
                 const int64_t* num_ims, int B, int T, int H, void* workspace, hipStream_t stream) {
  switch (hd) {
    case 32: return launch_fp8<32>(q, k, v, ld, hstride, bstride, qmul, o, num_ims, B, T, H, workspace, stream);
    case 64: return launch_fp8<64>(q, k, v, ld, hstride, bstride, qmul, o, num_ims, B, T, H, workspace, stream);
    case 128: return launch_fp8<128>(q, k, v, ld, hstride, bstride, qmul, o, num_ims, B, T, H, workspace, stream);
    case 256: return launch_fp8<256>(q, k, v, ld, hstride, bstride, qmul, o, num_ims, B, T, H, workspace, stream);
    default: return launch_fp8<384>(q, k, v, ld, hstride, bstride, qmul, o, num_ims, B, T, H, workspace, stream);
  }
}

}  // namespace

extern "C" {

// bytes of the workspace paths_attention_fp8 needs (three e4m3 fragment images)
int64_t paths_attention_fp8_workspace(int B, int T, int H, int head_dim) {
  const int64_t Tp = ((int64_t)T + KSTEP - 1) / KSTEP * KSTEP;
  return 3 * (int64_t)B * H * Tp * head_dim;
}

// o[B, T, H*hd] = softmax(q_s k^T) v with e4m3 operands (see the file header: opt-in, outside the 1e-4 logit bar), head_dim 32 or 64.
// q, k, v head-major [B][H][T][hd] fp32, q pre-scaled by log2(e)/sqrt(head_dim); keys >= num_ims[b] + 1 are masked.
int paths_attention_fp8(const float* q, const float* k, const float* v, float* o, const int64_t* num_ims, int B, int T, int H,
                        int head_dim, void* workspace, hipStream_t stream) {
  PATHS_REQUIRE(fp8_head_dim_ok(head_dim), "attention_fp8: head_dim must be 32, 64, 128, 256 or 384 (got %d)", head_dim);
  PATHS_REQUIRE(B > 0 && T > 0 && H > 0 && q && k && v && o && num_ims && workspace, "attention_fp8: bad arguments B=%d T=%d H=%d", B, T, H);
  PATHS_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)workspace) % 16 == 0, "attention_fp8: buffers must be 16-byte aligned");
  const int64_t hs = (int64_t)T * head_dim, bs = (int64_t)H * T * head_dim;
  return dispatch_fp8(head_dim, q, k, v, head_dim, hs, bs, 1.0f, o, num_ims, B, T, H, workspace, stream);
}

// The same on the token-major in_proj output qkv [B*T, 3d] (row stride ld; q | k | v blocks of d = H * head_dim columns, q UNscaled:
// qscale = log2(e) / sqrt(head_dim) is applied while the operand images are written).
int paths_attention_fp8_qkv(const float* qkv, int64_t ld, float* o, const int64_t* num_ims, int B, int T, int H, int head_dim, float qscale,
                            void* workspace, hipStream_t stream) {
  PATHS_REQUIRE(fp8_head_dim_ok(head_dim), "attention_fp8_qkv: head_dim must be 32, 64, 128, 256 or 384 (got %d)", head_dim);
  PATHS_REQUIRE(B > 0 && T > 0 && H > 0 && qkv && o && num_ims && workspace && ld >= 3 * H * head_dim, "attention_fp8_qkv: bad arguments B=%d T=%d H=%d", B, T, H);
  PATHS_REQUIRE(((uintptr_t)qkv | (uintptr_t)o | (uintptr_t)workspace) % 16 == 0, "attention_fp8_qkv: buffers must be 16-byte aligned");
  const int d = H * head_dim;
  const int64_t bs = (int64_t)T * ld;
  return dispatch_fp8(head_dim, qkv, qkv + d, qkv + 2 * d, ld, head_dim, bs, qscale, o, num_ims, B, T, H, workspace, stream);
}

}  // extern "C"
