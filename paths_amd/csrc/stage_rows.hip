// paths_stage_rows: the host-link hot path of host-resident slides (paths_amd/data_utils/slide.py:HostSlide).  Kernel: stage_rows.h.
#include "common.h"
#include "stage_rows.h"

constexpr int STAGE_WAVES = 4;      // rows per workgroup (1, 4 and 8 measured)

extern "C" {

int paths_stage_rows(int64_t* row_ptrs, int64_t rows, int row_bytes, void* stage, const void* zero_row, hipStream_t stream) {
  PATHS_REQUIRE(row_ptrs != nullptr && stage != nullptr && zero_row != nullptr, "stage_rows: null pointer (row_ptrs, stage and zero_row are required)");
  PATHS_REQUIRE(rows > 0 && rows <= ((int64_t)1 << 31), "stage_rows: rows (%lld) must be in [1, 2^31]", (long long)rows);
  PATHS_REQUIRE(row_bytes > 0 && row_bytes % 16 == 0, "stage_rows: row_bytes (%d) must be a positive multiple of 16", row_bytes);
  PATHS_REQUIRE((uintptr_t)stage % 16 == 0, "stage_rows: stage must be 16-byte aligned");
  hipLaunchKernelGGL((stage_rows_kernel<STAGE_WAVES, false>), dim3((unsigned)((rows + STAGE_WAVES - 1) / STAGE_WAVES)), dim3(STAGE_WAVES * 64), 0,
                     stream, row_ptrs, rows, row_bytes, reinterpret_cast<unsigned char*>(stage),
                     (int64_t)reinterpret_cast<uintptr_t>(zero_row));
  PATHS_LAUNCH_CHECK("stage_rows");
  return PATHS_OK;
}

}  // extern "C"
