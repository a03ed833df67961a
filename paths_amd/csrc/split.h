// Split operands for the 16-bit matrix cores: an fp32 value becomes two or three 16-bit PLANES whose sum is the value (to 16, 22 or
// 24 significant bits), a product of two split operands is the sum of the largest partial products of their planes, accumulated
// in fp32 by v_mfma_f32_16x16x32_{f16,bf16}.  Two 16-bit values travel packed in one uint32_t, 8 (one lane's share of a 16 x 32
// fragment) in a u32x4.
//   fp16 hi | lo         22 bits; operands must sit in fp16's range (O(1) activations, pre-scaled weights)
//   bf16 hi | mid | lo   exact: 3 x 8 = the 24 bits of fp32, at fp32's exponent range
//   bf16 hi | mid        16 bits at fp32's exponent range (gradient operands: no scales, nothing overflows)
#pragma once
#include "common.h"

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- pack two fp32 into one register (round to nearest even: v_cvt_pk_bf16_f32, v_cvt_pk_f16_f32) and widen either half again
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ float bf_lo(uint32_t p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf_hi(uint32_t p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

__device__ __forceinline__ uint32_t pk_f16(float a, float b) {
  f32x2 v = {a, b};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ float h_lo(uint32_t p) { return (float)__builtin_bit_cast(f16x2, p)[0]; }
__device__ __forceinline__ float h_hi(uint32_t p) { return (float)__builtin_bit_cast(f16x2, p)[1]; }

// ---- fp32 -> fp16 hi | lo planes
// Residuals of a packed fp16 pair: ra = a - (float)h.lo, rb = b - (float)h.hi, one v_fma_mix_f32 each (the mixed-precision FMA reads
// the half straight out of the packed register; written as a - (float)h hipcc emits v_cvt_f32_f16 + v_sub_f32, and turns an
// fmaf(h, -1, a) back into that).  Exact either way: the same fp32 subtraction.
__device__ __forceinline__ void f16_pair_residuals(uint32_t h, float a, float b, float& ra, float& rb) {
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(ra) : "v"(h), "v"(a));
  asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(rb) : "v"(h), "v"(b));
}
// 8 (4) fp32 -> hi | lo planes of 8 (4) fp16: 22 significant bits
__device__ __forceinline__ void split8h(const float (&x)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = x[2 * i], b = x[2 * i + 1];
    const uint32_t h = pk_f16(a, b);
    float ra, rb;
    f16_pair_residuals(h, a, b, ra, rb);
    hi[i] = h; lo[i] = pk_f16(ra, rb);
  }
}
__device__ __forceinline__ void split4h(const float (&x)[4], u32x2& hi, u32x2& lo) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float a = x[2 * i], b = x[2 * i + 1];
    const uint32_t h = pk_f16(a, b);
    float ra, rb;
    f16_pair_residuals(h, a, b, ra, rb);
    hi[i] = h; lo[i] = pk_f16(ra, rb);
  }
}
// The same planes as split8h (bit for bit), by another instruction stream - attn_x6.hip's, whose key step is VALU-issue bound.
// Residual + rounding of the lo plane: one v_fma_mixlo_f16 / v_fma_mixhi_f16 per value (they compute the fp32 FMA and write its
// fp16 rounding, nearest even as v_cvt_pk_f16_f32, into one half of the destination: two instructions where residuals + pack take
// three), the four low halves first: a half-register write directly in front of the other half's costs a wait state each (16 s_nop
// per key step).
__device__ __forceinline__ void split8h_lows_first(const float (&x)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) hi[i] = pk_f16(x[2 * i], x[2 * i + 1]);
  uint32_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r[i]) : "v"(hi[i]), "v"(x[2 * i]));
#pragma unroll
  for (int i = 0; i < 4; ++i) asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(r[i]) : "v"(hi[i]), "v"(x[2 * i + 1]));
#pragma unroll
  for (int i = 0; i < 4; ++i) lo[i] = r[i];
}

// ---- fp32 -> bf16 planes
// 8 fp32 -> PL planes of 8 bf16: PL = 3 hi, mid, lo (exact); PL = 2 hi, mid only (lo is not touched)
template <int PL>
__device__ __forceinline__ void split8(const float (&x)[8], u32x4& hi, u32x4& mid, u32x4& lo) {
  static_assert(PL == 2 || PL == 3, "two or three bf16 planes");
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = x[2 * i], b = x[2 * i + 1];
    const uint32_t h = pk_bf16(a, b);
    const float ra = a - bf_lo(h), rb = b - bf_hi(h);
    const uint32_t m = pk_bf16(ra, rb);
    hi[i] = h; mid[i] = m;
    if constexpr (PL == 3) {
      const float sa = ra - bf_lo(m), sb = rb - bf_hi(m);
      lo[i] = pk_bf16(sa, sb);
    }
  }
}
// the same into planes[0..PL).  (The loop lives in the reference form: written over the array, attn_x6.hip's assembly keeps its
// instructions but not the order of its register-kill annotations, and a plain compare against the previous build no longer holds.)
template <int PL>
__device__ __forceinline__ void split8(const float (&x)[8], u32x4 (&pl)[PL]) { split8<PL>(x, pl[0], pl[1], pl[PL - 1]); }

// ---- products: acc += A * B, one 16 x 16 x 32 block, the kept partial products smallest first
__device__ __forceinline__ f32x4 mfma_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// fp16 hi, lo: all but lo*lo
__device__ __forceinline__ f32x4 mfma_split_f16(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x4 c) {
  c = mfma_f16(a[1], b[0], c);
  c = mfma_f16(a[0], b[1], c);
  c = mfma_f16(a[0], b[0], c);
  return c;
}
// bf16, PL = 3 hi, mid, lo: the six largest of nine; PL = 2 hi, mid: all but mid*mid
template <int PL>
__device__ __forceinline__ f32x4 mfma_split_bf16(const u32x4 (&a)[PL], const u32x4 (&b)[PL], f32x4 c) {
  static_assert(PL == 2 || PL == 3, "two or three bf16 planes");
  if constexpr (PL == 3) {
    c = mfma_bf16(a[2], b[0], c);
    c = mfma_bf16(a[0], b[2], c);
    c = mfma_bf16(a[1], b[1], c);
  }
  c = mfma_bf16(a[1], b[0], c);
  c = mfma_bf16(a[0], b[1], c);
  c = mfma_bf16(a[0], b[0], c);
  return c;
}
