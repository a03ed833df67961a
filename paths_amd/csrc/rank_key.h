// The 64-bit key of the rank-counting kernels (select.hip: paths_topk / paths_topk_rows; topk_tiled.hip: their _tiled forms;
// perturb_rows.hip: paths_rank_joint).
#pragma once
#include <stdint.h>

// (~monotone(score) << 32) | index: keys are unique, and ascending keys are descending scores with ties in ascending index.
__device__ __forceinline__ unsigned long long topk_key(float score, int idx) {
  uint32_t u = __float_as_uint(score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // monotone float -> uint
  return ((unsigned long long)(~u) << 32) | (uint32_t)idx;
}
