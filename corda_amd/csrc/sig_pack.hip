// K23: mixed-scheme signature batches classified and packed on the GPU (sig_pack.hpp has
// the rule, the geometry and the layouts). Three passes on one stream -- count, scan,
// pack -- then per class a gather of the message rows and, after the verifiers, a
// scatter of the rows' statuses back to lane order. No kernel waits for another
// workgroup; every grid is sized for the host's upper bound and reads its class's count
// from the counter block.
#include <hip/hip_runtime.h>

#include "runtime.hpp"
#include "sig_pack.hpp"

namespace cordahip {
namespace {
using namespace sigpack;

// Count: a thread classifies the kIter lanes of its tile it visits and keeps their code
// bytes; the block's totals go out count-major (btot[k * tiles + tile]).
__global__ void __launch_bounds__(256) sig_count_kernel(In in, uint8_t* __restrict__ code,
                                                       uint32_t* __restrict__ btot, uint64_t ntiles) {
  __shared__ uint32_t part[kCounts][4];
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  uint32_t tot[kCounts];
#pragma unroll
  for (int k = 0; k < (int)kCounts; k++) tot[k] = 0;
  for (int it = 0; it < kIter; it++) {
    const uint64_t i = tile_lane(blockIdx.x, it, t);
    int ci = -1;
    if (i < in.n) {
      const uint8_t c = count_lane(in, i);
      code[i] = c;
      ci = (int)code_count(c);
    }
#pragma unroll
    for (int k = 0; k < (int)kCounts; k++) tot[k] += (uint32_t)__popcll(__ballot(ci == k));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < (int)kCounts; k++) part[k][wave] = tot[k];
  }
  __syncthreads();
  if (t < kCounts) btot[t * ntiles + blockIdx.x] = part[t][0] + part[t][1] + part[t][2] + part[t][3];
}

// Scan: block k walks count k's block totals in strides of 256 with a running carry;
// boff gets the exclusive prefix, the counter block the total.
__global__ void __launch_bounds__(256) sig_scan_kernel(const uint32_t* __restrict__ btot, uint32_t* __restrict__ boff,
                                                      uint64_t ntiles, uint32_t* __restrict__ hdr) {
  __shared__ uint32_t wsum[4];
  const uint32_t k = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t* src = btot + k * ntiles;
  uint32_t* dst = boff + k * ntiles;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < ntiles; base += 256) {
    const uint64_t j = base + t;
    const uint32_t v = j < ntiles ? src[j] : 0u;
    uint32_t x = v;  // inclusive prefix within the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if ((int)lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; w++) before += wsum[w];
    const uint32_t all = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (j < ntiles) dst[j] = carry + before + x - v;
    carry += all;
    __syncthreads();
  }
  if (t == 0) hdr[kHdrRaw + k] = carry;
}

// Pack: the lane's rank among its tile's lanes of the same count = the totals of the
// segments before its own (LDS) + its rank in its wave's ballot; the tile's first row
// of each count comes from the scan. ECDSA rows are one run: a lane's row adds up its
// ranks in the four sub-counts, perm[] keeps the sub-counts apart.
__global__ void __launch_bounds__(256) sig_pack_kernel(In in, Out out, uint64_t ntiles) {
  __shared__ uint32_t seg[kCounts][kSegs + 1];
  const uint32_t t = threadIdx.x, lane = t & 63;
  const unsigned long long below = (1ull << lane) - 1;
  if (blockIdx.x == 0 && t == 0) derive_header(out.hdr, out.rsa_cap);
  uint8_t code[kIter];
  uint32_t rank[kIter], ecrank[kIter];
  for (int it = 0; it < kIter; it++) {
    const uint64_t i = tile_lane(blockIdx.x, it, t);
    code[it] = i < in.n ? out.code[i] : (uint8_t)0xff;
    const int ci = i < in.n ? (int)code_count(code[it]) : -1;
    rank[it] = ecrank[it] = 0;
#pragma unroll
    for (int k = 0; k < (int)kCounts; k++) {
      const unsigned long long m = __ballot(ci == k);
      const uint32_t r = (uint32_t)__popcll(m & below);
      if (ci == k) rank[it] = r;
      if (k >= (int)kCntEc0 && k < (int)kCntRsa0) ecrank[it] += r;
      if (lane == 0) seg[k][seg_of(it, t)] = (uint32_t)__popcll(m);
    }
  }
  __syncthreads();
  if (t < kCounts) {  // exclusive prefix over the tile's segments
    uint32_t acc = 0;
    for (int s = 0; s <= kSegs; s++) {
      const uint32_t v = s < kSegs ? seg[t][s] : 0u;
      seg[t][s] = acc;
      acc += v;
    }
  }
  __syncthreads();
  const uint32_t* raw = out.hdr + kHdrRaw;
  for (int it = 0; it < kIter; it++) {
    const uint64_t i = tile_lane(blockIdx.x, it, t);
    if (i >= in.n) continue;
    const uint32_t ci = code_count(code[it]);
    const int s = seg_of(it, t);
    uint64_t row = (uint64_t)out.boff[ci * ntiles + blockIdx.x] + seg[ci][s] + rank[it], perm_pos = 0;
    if (class_of_count(ci) == kEc) {
      perm_pos = row;
      for (uint32_t k = kCntEc0; k < ci; k++) perm_pos += raw[k];
      row = ecrank[it];
      for (uint32_t k = kCntEc0; k < kCntRsa0; k++) row += (uint64_t)out.boff[k * ntiles + blockIdx.x] + seg[k][s];
    }
    (void)pack_lane(in, out, i, code[it], row, perm_pos);
  }
}

// rows[r] = msgs[idx[r]], r below the class's count: 16 bytes a thread for aligned
// 32-byte rows (transaction ids), else a byte a thread
__global__ void __launch_bounds__(256) sig_gather32_kernel(const uint8_t* __restrict__ msgs,
                                                          const uint32_t* __restrict__ idx,
                                                          const uint32_t* __restrict__ count,
                                                          uint8_t* __restrict__ rows) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = t >> 1, h = t & 1;
  if (r >= *count) return;
  reinterpret_cast<uint4*>(rows + r * 32)[h] = reinterpret_cast<const uint4*>(msgs + (uint64_t)idx[r] * 32)[h];
}
__global__ void __launch_bounds__(256) sig_gather_kernel(const uint8_t* __restrict__ msgs, uint32_t msg_len,
                                                        const uint32_t* __restrict__ idx,
                                                        const uint32_t* __restrict__ count,
                                                        uint8_t* __restrict__ rows) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t r = t / msg_len, q = t % msg_len;
  if (r >= *count) return;
  rows[t] = msgs[(uint64_t)idx[r] * msg_len + q];
}

__global__ void __launch_bounds__(256) sig_scatter_kernel(const uint8_t* __restrict__ row_status,
                                                         const uint32_t* __restrict__ lane_of_row,
                                                         const uint32_t* __restrict__ count,
                                                         uint8_t* __restrict__ status) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= *count) return;
  status[lane_of_row[r]] = row_status[r];
}

// A signed-tx batch: signature s signs the id of its transaction; one thread per
// transaction writes its index over its signatures' range (as gather_txid_kernel walks
// it), so the ids are never copied per signature. A range reaching past nsig is clipped;
// a signature no transaction owns keeps what the buffer held and is a bad-range lane at
// worst (the packer checks every row index against ntx).
__global__ void __launch_bounds__(256) sig_tx_rows_kernel(const uint64_t* __restrict__ tx_sig_off, uint64_t ntx,
                                                         uint64_t nsig, uint32_t* __restrict__ rows) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntx) return;
  const uint64_t hi = tx_sig_off[t + 1] < nsig ? tx_sig_off[t + 1] : nsig;
  for (uint64_t s = tx_sig_off[t]; s < hi; s++) rows[s] = (uint32_t)t;
}

}  // namespace

hipError_t launch_sig_tx_rows(const uint64_t* tx_sig_off, uint64_t ntx, uint64_t nsig, uint32_t* rows,
                              hipStream_t s) {
  if (!ntx || !nsig) return hipSuccess;
  if (ntx > 0xffffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sig_tx_rows_kernel, dim3((uint32_t)((ntx + 255) / 256)), dim3(256), 0, s, tx_sig_off, ntx, nsig,
                     rows);
  return hipGetLastError();
}

hipError_t launch_sig_pack(const sigpack::In& in, const sigpack::Out& out, hipStream_t s) {
  if (in.n == 0) return hipSuccess;
  if (in.n >= kMaxLanes) return hipErrorInvalidValue;
  const uint64_t nt = tiles(in.n);
  hipLaunchKernelGGL(sig_count_kernel, dim3((uint32_t)nt), dim3(256), 0, s, in, out.code, out.btot, nt);
  hipLaunchKernelGGL(sig_scan_kernel, dim3(kCounts), dim3(256), 0, s, out.btot, out.boff, nt, out.hdr);
  hipLaunchKernelGGL(sig_pack_kernel, dim3((uint32_t)nt), dim3(256), 0, s, in, out, nt);
  return hipGetLastError();
}

hipError_t launch_sig_gather(const uint8_t* msgs, uint32_t msg_len, const uint32_t* idx, const uint32_t* count,
                             uint64_t cap, uint8_t* rows, hipStream_t s) {
  if (!cap || !msg_len) return hipSuccess;
  if (msg_len == 32 && !(reinterpret_cast<uintptr_t>(msgs) & 15)) {
    hipLaunchKernelGGL(sig_gather32_kernel, dim3((uint32_t)((2 * cap + 255) / 256)), dim3(256), 0, s, msgs, idx, count,
                       rows);
    return hipGetLastError();
  }
  const uint64_t blocks = (cap * msg_len + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sig_gather_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, msgs, msg_len, idx, count, rows);
  return hipGetLastError();
}

hipError_t launch_sig_scatter(const uint8_t* row_status, const uint32_t* lane_of_row, const uint32_t* count,
                              uint64_t cap, uint8_t* status, hipStream_t s) {
  if (!cap) return hipSuccess;
  hipLaunchKernelGGL(sig_scatter_kernel, dim3((uint32_t)((cap + 255) / 256)), dim3(256), 0, s, row_status,
                     lane_of_row, count, status);
  return hipGetLastError();
}

}  // namespace cordahip
