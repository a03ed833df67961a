// Launchers of the packed forms of select.hip's two address-forming kernels (gather_kernel<T, true>, level0_kernel<T, true>), defined
// in select.hip beside the kernels; pack_rows.hip holds their C entry points with the rest of the packed-slide surface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

int paths_select_gather_rows_packed(bool h16, const int64_t* grid_ptrs, const int64_t* index_ptrs, const int* src_cell, int D, const float* state_cur,
                                    int64_t n_cur, int64_t ld_state_cur, const int* src_row, int Dp, const int64_t* num_out, int B, int64_t n_next,
                                    float* fts_out, float* state_out, int zero_pad, int64_t* row_ptrs, const float* zero_row, hipStream_t stream);
int paths_select_level0_packed(bool h16, const int64_t* grid_ptrs, const int64_t* index_ptrs, const int* gx, const int* gy, int B, int D,
                               int patch_size, int64_t n0, float* fts, int64_t* locs, int64_t* parent, int64_t* num_ims, int zero_pad,
                               int64_t* row_ptrs, const float* zero_row, hipStream_t stream);
