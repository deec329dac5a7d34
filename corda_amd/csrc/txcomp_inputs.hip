// K22: a component batch's inputs and time windows as commit rows
// (cordahip_txcomp_inputs_device; the rule is txcomp_inputs_core.hpp). Three launches on
// the caller's stream, no scratch and no atomics: the count pass leaves each
// transaction's ref count in tx_ref_off[t] and its flag in gate[t], the one-block scan
// turns them in place into the clamped offsets and the gate, and the copy pass writes
// the rows. One lane per transaction in the count and copy passes: a payment has a
// handful of items, and its refs lie next to each other in the payload.
#include <hip/hip_runtime.h>

#include "txcomp_inputs_core.hpp"

namespace cordahip {

namespace {

__global__ void __launch_bounds__(256) txin_count_kernel(txin::Batch B, uint64_t* __restrict__ tx_ref_off,
                                                         int64_t* __restrict__ tw_from, int64_t* __restrict__ tw_until,
                                                         uint8_t* __restrict__ gate) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B.ntx) return;
  const txin::TxScan x = txin::scan_tx(B, t);
  tx_ref_off[t] = x.nref;
  tw_from[t] = x.tw_from;
  tw_until[t] = x.tw_until;
  gate[t] = x.flagged;
}

// tx_ref_off[t]: count -> min(refs before t, ref_cap); gate[t]: flag -> the gate byte. One
// block, each thread a run of consecutive transactions, the 1024 run totals scanned by
// one thread (notary_prep_kernel's scheme).
__global__ void __launch_bounds__(1024) txin_scan_kernel(uint64_t ntx, uint64_t ref_cap,
                                                         const uint8_t* __restrict__ tx_status,
                                                         uint64_t* __restrict__ tx_ref_off, uint8_t* __restrict__ gate) {
  __shared__ uint64_t s_r[1024];
  const uint64_t per = (ntx + 1023) / 1024;
  const uint64_t t0 = threadIdx.x * per < ntx ? threadIdx.x * per : ntx, t1 = t0 + per < ntx ? t0 + per : ntx;
  uint64_t r = 0;
  for (uint64_t t = t0; t < t1; t++) r = txin::add_sat(r, tx_ref_off[t]);
  s_r[threadIdx.x] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0;
    for (uint32_t i = 0; i < 1024; i++) {
      const uint64_t c = s_r[i];
      s_r[i] = a;
      a = txin::add_sat(a, c);
    }
    tx_ref_off[ntx] = a < ref_cap ? a : ref_cap;
  }
  __syncthreads();
  r = s_r[threadIdx.x];
  for (uint64_t t = t0; t < t1; t++) {
    const uint64_t c = tx_ref_off[t];
    uint8_t g;
    tx_ref_off[t] = txin::place(r, c, gate[t] != 0, ref_cap, tx_status ? tx_status[t] : 0, g);
    gate[t] = g;
    r = txin::add_sat(r, c);
  }
}

__global__ void __launch_bounds__(256) txin_copy_kernel(txin::Batch B, const uint64_t* __restrict__ tx_ref_off,
                                                        uint32_t* __restrict__ refs) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B.ntx) return;
  const uint64_t a = tx_ref_off[t], e = tx_ref_off[t + 1];  // both at most ref_cap
  if (e > a) txin::copy_tx(B, t, refs + a * txin::kRefWords, e - a);
}

}  // namespace

hipError_t launch_txcomp_inputs(const cordahip_kryo_item* d_items, uint64_t n_items, const uint8_t* d_payload,
                                uint64_t payload_len, const uint64_t* d_tx_item_off, uint64_t ntx,
                                const uint8_t* d_tx_status, uint32_t* d_refs, uint64_t ref_cap, uint64_t* d_tx_ref_off,
                                int64_t* d_tw_from, int64_t* d_tw_until, uint8_t* d_gate, hipStream_t s) {
  if (!ntx) return hipSuccess;
  const txin::Batch B{d_items, n_items, d_payload, payload_len, d_tx_item_off, ntx};
  const dim3 grid((uint32_t)((ntx + 255) / 256)), blk(256);
  hipLaunchKernelGGL(txin_count_kernel, grid, blk, 0, s, B, d_tx_ref_off, d_tw_from, d_tw_until, d_gate);
  hipLaunchKernelGGL(txin_scan_kernel, dim3(1), dim3(1024), 0, s, ntx, ref_cap, d_tx_status, d_tx_ref_off, d_gate);
  hipLaunchKernelGGL(txin_copy_kernel, grid, blk, 0, s, B, d_tx_ref_off, d_refs);
  return hipGetLastError();
}

}  // namespace cordahip
