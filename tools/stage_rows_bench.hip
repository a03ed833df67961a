// Shapes of the row-staging kernel (paths_amd/csrc/stage_rows.h) over the host link: rows per workgroup 1 / 4 / 8, plain against
// non-temporal loads, 4-KiB (fp32) and 2-KiB (fp16) rows.  The source is a pinned host table far larger than any cache, the rows are
// distinct and in random order (what a level's top-K selects); the address table is restored before every launch because the kernel
// rewrites it.  Prints ONE JSON object: median / min microseconds per launch and the host-link rate (bytes staged / time).
// build: hipcc -O3 --offload-arch=gfx950 -I paths_amd/csrc tools/stage_rows_bench.hip -o tools/_bin/stage_rows_bench
// run:   tools/_bin/stage_rows_bench [rows = 65536] [reps = 7]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "stage_rows.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

static uint32_t fmix32(uint32_t h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16; return h; }

template <int WAVES, bool NT>
static void run(const char* name, int64_t* d_ptrs, const int64_t* d_ptrs0, int64_t rows, int row_bytes, unsigned char* stage,
                int64_t zero_row, int reps) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  std::vector<float> us;
  for (int r = 0; r < reps + 2; ++r) {
    CK(hipMemcpyAsync(d_ptrs, d_ptrs0, rows * sizeof(int64_t), hipMemcpyDeviceToDevice, 0));
    CK(hipEventRecord(a, 0));
    hipLaunchKernelGGL((stage_rows_kernel<WAVES, NT>), dim3((unsigned)((rows + WAVES - 1) / WAVES)), dim3(WAVES * 64), 0, 0, d_ptrs, rows,
                       row_bytes, stage, zero_row);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    CK(hipGetLastError());
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    if (r >= 2) us.push_back(ms * 1e3f);
  }
  std::sort(us.begin(), us.end());
  const double med = us[us.size() / 2], bytes = (double)(rows - (rows + 96) / 97) * row_bytes;      // (padding entries move no bytes)
  printf(",\n  \"%s_%dB\": {\"median_us\": %.1f, \"min_us\": %.1f, \"GB_per_s\": %.2f}", name, row_bytes, med, us[0], bytes / (med * 1e-6) / 1e9);
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
}

int main(int argc, char** argv) {
  const int64_t rows = argc > 1 ? atoll(argv[1]) : 65536;
  const int reps = argc > 2 ? atoi(argv[2]) : 7;
  const int64_t src_rows = 4 * rows;                       // a quarter of the table's rows is fetched, in random order
  const int max_row = 4096;
  unsigned char* src = nullptr;
  CK(hipHostMalloc((void**)&src, (size_t)src_rows * max_row, hipHostMallocDefault));
  for (size_t i = 0; i < (size_t)src_rows * max_row; i += 64) src[i] = (unsigned char)(i >> 6);     // (touch every cache line)
  unsigned char *stage = nullptr, *zero = nullptr;
  int64_t *d_ptrs = nullptr, *d_ptrs0 = nullptr;
  CK(hipMalloc((void**)&stage, (size_t)rows * max_row));
  CK(hipMalloc((void**)&zero, max_row));
  CK(hipMemset(zero, 0, max_row));
  CK(hipMalloc((void**)&d_ptrs, rows * sizeof(int64_t)));
  CK(hipMalloc((void**)&d_ptrs0, rows * sizeof(int64_t)));
  printf("{\"rows\": %lld, \"reps\": %d, \"pinned_source_MiB\": %lld", (long long)rows, reps, (long long)(src_rows * max_row >> 20));
  for (int row_bytes : {4096, 2048}) {
    std::vector<int64_t> h(rows);
    for (int64_t m = 0; m < rows; ++m) {
      // a distinct source row per entry: slot m of 4 consecutive rows chosen by a hash, then the slots visited in a shuffled order
      const int64_t slot = (int64_t)(((uint64_t)m * 2654435761ull) % (uint64_t)rows);
      h[m] = (int64_t)(uintptr_t)(src + ((size_t)(4 * slot + (fmix32((uint32_t)m) & 3)) * row_bytes));
    }
    for (int64_t m = 0; m < rows; m += 97) h[m] = (int64_t)(uintptr_t)zero;                       // ~1 % padding entries
    CK(hipMemcpy(d_ptrs0, h.data(), rows * sizeof(int64_t), hipMemcpyHostToDevice));
    const int64_t zr = (int64_t)(uintptr_t)zero;
    run<1, false>("waves1", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
    run<4, false>("waves4", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
    run<8, false>("waves8", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
    run<1, true>("waves1_nt", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
    run<4, true>("waves4_nt", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
    run<8, true>("waves8_nt", d_ptrs, d_ptrs0, rows, row_bytes, stage, zr, reps);
  }
  printf("\n}\n");
  CK(hipFree(stage));
  CK(hipFree(zero));
  CK(hipFree(d_ptrs));
  CK(hipFree(d_ptrs0));
  CK(hipHostFree(src));
  return 0;
}
