// Cross-lane reductions of a 64-lane wave; every lane ends up with the result.
#pragma once
#include "common.h"

// ---- all 64 lanes, xor butterfly, offsets 1, 2, .. 32 (the summation order is part of the result: keep it)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {            // integer counts: exact in any order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- the 4 lanes l, l ^ 16, l ^ 32, l ^ 48: the lanes that hold one column of a 16 x 16 MFMA accumulator tile
__device__ __forceinline__ float rows_max(float x) { x = fmaxf(x, __shfl_xor(x, 16)); return fmaxf(x, __shfl_xor(x, 32)); }
__device__ __forceinline__ float rows_sum(float x) { x += __shfl_xor(x, 16); return x + __shfl_xor(x, 32); }

// ---- without LDS round trips (ds_bpermute), for dependent chains
// x + (x of lane ^ 16) and x + (x of lane ^ 32) by v_permlane16/32_swap (VALU latency instead of the LDS round trip of
// ds_bpermute).  v_permlane16_swap exchanges the odd 16-lane rows of its first operand with the even rows of the second,
// v_permlane32_swap the upper half of the first with the lower half of the second: given the same value in both, the two results
// add up to the pair sum in every lane.  Inline asm: through __builtin_amdgcn_permlane16_swap hipcc (ROCm 7.2) added result 0 to
// itself here (v_add v, r0, r0: wrong sums).  s_nop 1 = the two wait states between a VALU write of an operand and the swap.
__device__ __forceinline__ float sum_xor16(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
__device__ __forceinline__ float sum_xor32(float x) {
  float a = x, b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
// sum over the 16 lanes of a row (DPP: two quad permutes, two mirrors), over the 32 of a half (+ v_permlane16_swap) and over all 64
// (+ v_permlane32_swap).  Not wave_sum's order: other bits.
__device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));  // row_half_mirror
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true));  // row_mirror
  return v;
}
__device__ __forceinline__ float half_sum32(float v) { return sum_xor16(row_sum16(v)); }
__device__ __forceinline__ float wave_sum64(float v) { return sum_xor32(half_sum32(v)); }
