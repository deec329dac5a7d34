// The alternative to cordahip_commit_log_revoke's mark + per-cluster repair: ONE lane
// applying commit_core.hpp's erase_row to the rows in order (the in-order statement of
// revoke, with no marks, no claim table and no second launch). Times that kernel with
// HIP events on a table of 2^log2 slots filled to `fill` of its capacity, the rows to
// remove being the last `n` inserted, and checks that it removed them all. The table
// is built on the host with load_row and copied over. One JSON line.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -o commit_erase_serial commit_erase_serial.hip
//   commit_erase_serial [log2=24] [n=131072] [fill_percent=50]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../corda_amd/csrc/commit_core.hpp"

using namespace cordahip::commit;

#define CK(x)                                                      \
  do {                                                             \
    hipError_t e_ = (x);                                           \
    if (e_ != hipSuccess) {                                        \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));      \
      return 1;                                                    \
    }                                                              \
  } while (0)

constexpr uint32_t kRowWords = kRefWords + kByWords;

__global__ void __launch_bounds__(64) erase_serial_kernel(Table T, const uint32_t* __restrict__ rows, uint64_t n,
                                                          unsigned long long* __restrict__ removed) {
  if (blockIdx.x || threadIdx.x) return;
  unsigned long long r = 0;
  for (uint64_t i = 0; i < n; i++) r += erase_row(T, rows + i * kRowWords);
  *removed = r;
}

int main(int argc, char** argv) {
  const uint32_t log2 = argc > 1 ? (uint32_t)atoi(argv[1]) : 24;
  const uint64_t n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 131072;
  const uint64_t pct = argc > 3 ? strtoull(argv[3], nullptr, 10) : 50;
  if (log2 < 6 || log2 > 26 || pct > 80) return 2;
  const uint64_t cap = 1ull << log2, entries = cap / 100 * pct;
  if (n == 0 || n > entries) return 2;
  std::vector<uint32_t> slots(cap * kSlotWords, 0), rows(n * kRowWords);
  const Table H{slots.data(), cap - 1, 0x0123456789abcdefull, 0xfedcba9876543210ull};
  uint64_t s = 20261020;
  for (uint64_t e = 0; e < entries; e++) {
    uint32_t row[kRowWords];
    for (uint32_t q = 0; q < kRowWords; q += 2) {  // splitmix64, two words a draw
      uint64_t z = (s += 0x9e3779b97f4a7c15ull);
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      row[q] = (uint32_t)z;
      if (q + 1 < kRowWords) row[q + 1] = (uint32_t)(z >> 32);
    }
    if (load_row(H, row) != 1) return 3;
    if (e >= entries - n) std::memcpy(rows.data() + (e - (entries - n)) * kRowWords, row, sizeof(row));
  }
  uint32_t *d_slots = nullptr, *d_rows = nullptr;
  unsigned long long* d_removed = nullptr;
  CK(hipMalloc(&d_slots, slots.size() * 4));
  CK(hipMalloc(&d_rows, rows.size() * 4));
  CK(hipMalloc(&d_removed, 8));
  CK(hipMemcpy(d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(d_removed, 0, 8));
  const Table D{d_slots, cap - 1, H.k0, H.k1};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, nullptr));
  hipLaunchKernelGGL(erase_serial_kernel, dim3(1), dim3(64), 0, nullptr, D, d_rows, n, d_removed);
  CK(hipGetLastError());
  CK(hipEventRecord(e1, nullptr));
  CK(hipEventSynchronize(e1));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  unsigned long long removed = 0;
  CK(hipMemcpy(&removed, d_removed, 8, hipMemcpyDeviceToHost));
  printf("{\"kernel\": \"single-lane erase_row\", \"log2\": %u, \"entries\": %llu, \"rows\": %llu, \"removed\": %llu, "
         "\"device_ms\": %.3f}\n", log2, (unsigned long long)entries, (unsigned long long)n, removed, ms);
  CK(hipFree(d_slots));
  CK(hipFree(d_rows));
  CK(hipFree(d_removed));
  return removed == n ? 0 : 1;
}
