// libcordahip.so's notary commit log (K16, commit_log.hip): the host side of
// cordahip_commit_log_* and cordahip_commit_inputs*. The log itself (CommitLog) is in
// runtime.hpp, its rows and hash table in commit_core.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

#include "api_support.hpp"
#include "csr_check.hpp"
#include "notary_stage.hpp"

using namespace cordahip;
using namespace cordahip::rt;

namespace {

// ---- notary commit log (K16, commit_log.hip) -------------------------------------
std::shared_ptr<CommitLog> log_at(cordahip_ctx* ctx, uint32_t id) {
  std::lock_guard<std::mutex> g(ctx->logs_mu);
  const auto it = ctx->logs.find(id);
  return it == ctx->logs.end() ? nullptr : it->second;
}

constexpr uint32_t kCommitMinLog2 = 6, kCommitMaxLog2 = 32;
constexpr size_t kCommitRowBytes = sizeof(cordahip_commit_row), kCommitRefBytes = sizeof(cordahip_state_ref),
                 kCommitByBytes = sizeof(cordahip_consuming_tx);
static_assert(kCommitRefBytes == commit::kRefWords * 4 && kCommitByBytes == commit::kByWords * 4 &&
                  kCommitRowBytes == kCommitRefBytes + kCommitByBytes,
              "commit_core.hpp's rows are the header's");

// would `more` further entries pass 7/8 of the capacity? (mu held)
bool commit_log_full(const CommitLog& L, uint64_t more) {
  const uint64_t room = ((1ull << L.capacity_log2) / 8) * 7;
  return L.bound > room || more > room - L.bound;
}

// the log's host stage of at least `bytes` on both sides (mu held; the previous host
// call has drained, so growing frees nothing in use)
int commit_stage(CommitLog& L, size_t bytes, size_t dev_bytes = 0) {  // dev_bytes: a longer device side
  bytes = std::max<size_t>(bytes, 64);
  if (L.stage_h.ensure(bytes) != hipSuccess || L.stage_d.ensure(std::max(bytes, dev_bytes)) != hipSuccess)
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  return CORDAHIP_SUCCESS;
}

int commit_log_create_impl(cordahip_ctx* ctx, int device, uint32_t capacity_log2, const uint8_t* salt,
                           uint32_t* log_id) {
  Device* d = dev_at(ctx, device);
  if (!d || capacity_log2 < kCommitMinLog2 || capacity_log2 > kCommitMaxLog2) return CORDAHIP_ERR_INVALID_ARG;
  const Activity act(*d);
  if (hipSetDevice(d->id) != hipSuccess) return CORDAHIP_ERR_HIP;
  auto L = std::make_shared<CommitLog>();
  L->dev = d;
  for (DevBuf* b : {&L->tab, &L->counters, &L->scratch, &L->stage_d}) b->dev = d->id;
  L->capacity_log2 = capacity_log2;
  uint8_t k[16];
  if (salt) {
    std::memcpy(k, salt, 16);
  } else {
    std::random_device rd;
    for (int i = 0; i < 16; i += 4) {
      const uint32_t r = rd();
      std::memcpy(k + i, &r, 4);
    }
  }
  std::memcpy(&L->k0, k, 8);
  std::memcpy(&L->k1, k + 8, 8);
  if (L->tab.ensure((size_t)commit::kSlotWords * 4 << capacity_log2) != hipSuccess || L->counters.ensure(16) != hipSuccess)
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  hipError_t e = hipMemsetAsync(L->tab.p, 0, L->tab.cap, d->stream);
  e = e ? e : hipMemsetAsync(L->counters.p, 0, 16, d->stream);
  const hipError_t f = hipStreamSynchronize(d->stream);
  if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
  std::lock_guard<std::mutex> g(ctx->logs_mu);
  L->id = ctx->next_log_id++;
  if (L->id == 0) return CORDAHIP_ERR_OUT_OF_MEMORY;  // 2^32 logs created: ids are never reused
  ctx->logs.emplace(L->id, L);
  *log_id = L->id;
  return CORDAHIP_SUCCESS;
}

int commit_log_destroy_impl(cordahip_ctx* ctx, uint32_t log_id) {
  std::shared_ptr<CommitLog> L;
  {
    std::lock_guard<std::mutex> g(ctx->logs_mu);
    const auto it = ctx->logs.find(log_id);
    if (it == ctx->logs.end()) return CORDAHIP_ERR_INVALID_ARG;
    L = it->second;
    ctx->logs.erase(it);  // no new call finds it; a ticket already queued keeps it alive until it has run
  }
  std::lock_guard<std::mutex> g(L->mu);
  if (hipSetDevice(L->dev->id) != hipSuccess) return CORDAHIP_ERR_HIP;
  return hip_err(L->ev.sync());  // the table goes with the last reference (~CommitLog)
}

int commit_log_reserve_impl(cordahip_ctx* ctx, uint32_t log_id, uint32_t capacity_log2) {
  const auto L = log_at(ctx, log_id);
  if (!L || capacity_log2 > kCommitMaxLog2) return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L->mu);
  if (capacity_log2 <= L->capacity_log2) return CORDAHIP_SUCCESS;  // never shrinks
  Device& d = *L->dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess || L->ev.sync() != hipSuccess) return CORDAHIP_ERR_HIP;
  DevBuf nt;
  nt.dev = d.id;
  if (nt.ensure((size_t)commit::kSlotWords * 4 << capacity_log2) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  const commit::Table from = L->table();
  const commit::Table to{nt.as<uint32_t>(), (1ull << capacity_log2) - 1, L->k0, L->k1};
  hipError_t e = hipMemsetAsync(nt.p, 0, nt.cap, d.stream);
  e = e ? e : launch_commit_rehash(from, to, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  if (e != hipSuccess || f != hipSuccess) {
    nt.release();
    return CORDAHIP_ERR_HIP;
  }
  std::swap(L->tab, nt);
  nt.release();
  L->capacity_log2 = capacity_log2;
  return CORDAHIP_SUCCESS;
}

int commit_log_stats_impl(cordahip_ctx* ctx, uint32_t log_id, uint64_t* entries, uint64_t* capacity,
                          uint64_t* next_seq) {
  const auto L = log_at(ctx, log_id);
  if (!L) return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L->mu);
  if (hipSetDevice(L->dev->id) != hipSuccess || L->ev.sync() != hipSuccess) return CORDAHIP_ERR_HIP;
  uint64_t n = 0;
  if (hipMemcpy(&n, L->counters.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return CORDAHIP_ERR_HIP;
  L->bound = n;  // every call enqueued so far has finished: the count is exact
  if (entries) *entries = n;
  if (capacity) *capacity = 1ull << L->capacity_log2;
  if (next_seq) *next_seq = L->next_seq;
  return CORDAHIP_SUCCESS;
}

int commit_log_load_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                         uint64_t* n_already_present) {
  const auto L = log_at(ctx, log_id);
  if (!L || (n && !rows)) return CORDAHIP_ERR_INVALID_ARG;
  if (n_already_present) *n_already_present = 0;
  if (n == 0) return CORDAHIP_SUCCESS;
  std::lock_guard<std::mutex> g(L->mu);
  if (commit_log_full(*L, n)) return CORDAHIP_ERR_LOG_FULL;
  Device& d = *L->dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (const int rc = commit_stage(*L, n * kCommitRowBytes)) return rc;
  const size_t need = commit_load_scratch_bytes(n);
  if (L->ev.grow(need > L->scratch.cap, [&] { return L->scratch.ensure(need); }) != hipSuccess)
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  std::memcpy(L->stage_h.p, rows, n * kCommitRowBytes);
  hipStream_t s = d.stream;
  unsigned long long* ctr = L->counters.as<unsigned long long>();
  hipError_t e = hipMemcpyAsync(L->stage_d.p, L->stage_h.p, n * kCommitRowBytes, hipMemcpyHostToDevice, s);
  e = e ? e : L->ev.wait(s);
  e = e ? e : launch_commit_load(L->table(), L->stage_d.as<uint32_t>(), n, L->scratch.p, ctr, s);
  e = e ? e : L->ev.record(s);
  e = e ? e : hipMemcpyAsync(L->stage_h.p, ctr + 1, 8, hipMemcpyDeviceToHost, s);
  const hipError_t f = hipStreamSynchronize(s);
  if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
  const uint64_t already = *L->stage_h.as<uint64_t>();
  L->bound += n - std::min(already, n);
  if (n_already_present) *n_already_present = already;
  return CORDAHIP_SUCCESS;
}

int commit_log_lookup_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_state_ref* refs, uint64_t n,
                           uint8_t* present, cordahip_consuming_tx* by) {
  const auto L = log_at(ctx, log_id);
  if (!L || (n && (!refs || !present || !by))) return CORDAHIP_ERR_INVALID_ARG;
  if (n == 0) return CORDAHIP_SUCCESS;
  std::lock_guard<std::mutex> g(L->mu);
  Device& d = *L->dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  const size_t o_by = (n * kCommitRefBytes + 15) & ~(size_t)15, o_pr = o_by + n * kCommitByBytes;
  if (const int rc = commit_stage(*L, o_pr + n)) return rc;
  uint8_t *h = L->stage_h.as<uint8_t>(), *dv = L->stage_d.as<uint8_t>();
  std::memcpy(h, refs, n * kCommitRefBytes);
  hipStream_t s = d.stream;
  hipError_t e = hipMemcpyAsync(dv, h, n * kCommitRefBytes, hipMemcpyHostToDevice, s);
  e = e ? e : L->ev.wait(s);
  e = e ? e
        : launch_commit_lookup(L->table(), reinterpret_cast<const uint32_t*>(dv), n, dv + o_pr,
                               reinterpret_cast<uint32_t*>(dv + o_by), s);
  e = e ? e : L->ev.record(s);
  e = e ? e : hipMemcpyAsync(h + o_by, dv + o_by, n * kCommitByBytes + n, hipMemcpyDeviceToHost, s);
  const hipError_t f = hipStreamSynchronize(s);
  if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
  std::memcpy(by, h + o_by, n * kCommitByBytes);
  std::memcpy(present, h + o_pr, n);
  return CORDAHIP_SUCCESS;
}

// A synchronous call's turn among the log's tickets: taken at construction behind every
// ticket submitted so far, given up at destruction (commit_submit_impl's jobs wait the
// same way, so a later ticket runs after the call).
class CommitTurn {
 public:
  explicit CommitTurn(CommitLog& L) : L_(L) {
    std::unique_lock<std::mutex> w(L_.turn_mu);
    const uint64_t turn = L_.turn_next++;
    L_.turn_cv.wait(w, [&] { return L_.turn_now == turn; });
  }
  ~CommitTurn() {
    {
      std::lock_guard<std::mutex> w(L_.turn_mu);
      L_.turn_now++;
    }
    L_.turn_cv.notify_all();
  }
  CommitTurn(const CommitTurn&) = delete;
  CommitTurn& operator=(const CommitTurn&) = delete;

 private:
  CommitLog& L_;
};

int commit_log_revoke_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                           uint8_t* revoked, uint64_t* n_removed) {
  const auto L = log_at(ctx, log_id);
  if (!L || (n && (!rows || !revoked))) return CORDAHIP_ERR_INVALID_ARG;
  if (n_removed) *n_removed = 0;
  if (n == 0) return CORDAHIP_SUCCESS;
  const CommitTurn turn(*L);
  std::lock_guard<std::mutex> g(L->mu);
  Device& d = *L->dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  const size_t o_rev = (n * kCommitRowBytes + 15) & ~(size_t)15, o_cnt = (o_rev + n + 15) & ~(size_t)15;
  if (const int rc = commit_stage(*L, o_cnt + 8)) return rc;
  const size_t need = commit_revoke_scratch_bytes(n);
  if (L->ev.grow(need > L->scratch.cap, [&] { return L->scratch.ensure(need); }) != hipSuccess)
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t *h = L->stage_h.as<uint8_t>(), *dv = L->stage_d.as<uint8_t>();
  std::memcpy(h, rows, n * kCommitRowBytes);
  hipStream_t s = d.stream;
  unsigned long long* ctr = L->counters.as<unsigned long long>();
  hipError_t e = hipMemcpyAsync(dv, h, n * kCommitRowBytes, hipMemcpyHostToDevice, s);
  e = e ? e : L->ev.wait(s);
  e = e ? e : launch_commit_revoke(L->table(), reinterpret_cast<const uint32_t*>(dv), n, dv + o_rev, L->scratch.p, ctr, s);
  e = e ? e : L->ev.record(s);
  e = e ? e : hipMemcpyAsync(h + o_rev, dv + o_rev, n, hipMemcpyDeviceToHost, s);
  e = e ? e : hipMemcpyAsync(h + o_cnt, ctr + 1, 8, hipMemcpyDeviceToHost, s);
  const hipError_t f = hipStreamSynchronize(s);
  if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
  std::memcpy(revoked, h + o_rev, n);
  if (n_removed) std::memcpy(n_removed, h + o_cnt, 8);
  return CORDAHIP_SUCCESS;  // the bound stays: it remains an upper bound of the live entries
}

int commit_log_export_impl(cordahip_ctx* ctx, uint32_t log_id, uint64_t since_seq, cordahip_commit_row* rows,
                           uint64_t* seq, uint64_t cap, uint64_t* n_total) {
  const auto L = log_at(ctx, log_id);
  if (!L || !n_total || (cap && !rows)) return CORDAHIP_ERR_INVALID_ARG;
  const CommitTurn turn(*L);
  std::lock_guard<std::mutex> g(L->mu);
  Device& d = *L->dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  cap = std::min(cap, L->bound);  // no more entries than the bound are live: slots past it are never written
  const size_t o_seq = (cap * kCommitRowBytes + 15) & ~(size_t)15, o_cnt = o_seq + cap * 8;
  if (const int rc = commit_stage(*L, o_cnt + 8)) return rc;
  uint8_t *h = L->stage_h.as<uint8_t>(), *dv = L->stage_d.as<uint8_t>();
  hipStream_t s = d.stream;
  unsigned long long* total = reinterpret_cast<unsigned long long*>(dv + o_cnt);
  hipError_t e = L->ev.wait(s);
  e = e ? e
        : launch_commit_export(L->table(), since_seq, reinterpret_cast<uint32_t*>(dv),
                               reinterpret_cast<uint64_t*>(dv + o_seq), cap, total, s);
  e = e ? e : L->ev.record(s);
  e = e ? e : hipMemcpyAsync(h + o_cnt, total, 8, hipMemcpyDeviceToHost, s);
  hipError_t f = hipStreamSynchronize(s);
  if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
  uint64_t total_h = 0;
  std::memcpy(&total_h, h + o_cnt, 8);
  const uint64_t m = std::min(total_h, cap);
  if (m) {  // only what was written comes back
    e = hipMemcpyAsync(h, dv, m * kCommitRowBytes, hipMemcpyDeviceToHost, s);
    e = e ? e : hipMemcpyAsync(h + o_seq, dv + o_seq, m * 8, hipMemcpyDeviceToHost, s);
    f = hipStreamSynchronize(s);
    if (e != hipSuccess || f != hipSuccess) return CORDAHIP_ERR_HIP;
    std::memcpy(rows, h, m * kCommitRowBytes);
    if (seq) std::memcpy(seq, h + o_seq, m * 8);
  }
  *n_total = total_h;
  return CORDAHIP_SUCCESS;
}

// The commit kernels on stream s behind the log's previous call, followed by the
// log's fence; the log's counters advance (mu held, device current, the scratch
// grown, the load bound checked).
hipError_t commit_enqueue(CommitLog& L, const commit::Batch& B, uint64_t n_refs, hipStream_t s) {
  hipError_t e = L.ev.wait(s);
  e = e ? e
        : launch_commit_inputs(L.table(), B, n_refs, L.next_seq, L.scratch.p, L.counters.as<unsigned long long>(), s);
  e = e ? e : L.ev.record(s);
  L.next_seq += B.ntx;  // consumed even if an enqueue failed: sequence numbers only ever grow
  L.bound += n_refs;
  return e;
}
hipError_t commit_scratch(CommitLog& L, uint64_t ntx, uint64_t n_refs) {
  const size_t need = commit_scratch_bytes(ntx, n_refs);
  return L.ev.grow(need > L.scratch.cap, [&] { return L.scratch.ensure(need); });
}

// what the host and the device form ask of the scalars and the pointer pairing
bool commit_scalars_ok(const cordahip_commit_batch* b) {
  const cordahip_commit_batch z{0, nullptr, nullptr, nullptr, nullptr, 0, b->tw_from, b->tw_until, b->now_ns,
                                b->tolerance_ns, nullptr, nullptr, nullptr, nullptr, nullptr};
  return check_commit([](uint64_t, uint64_t, auto&&) {}, &z);
}

int commit_on(cordahip_ctx* ctx, CommitLog& L, const cordahip_commit_batch* b) {
  const uint64_t ntx = b->ntx;
  if (!check_commit(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!b->txid || !b->caller || !b->tx_status || !b->committed) return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t r0 = b->tx_ref_off[0], nr = b->tx_ref_off[ntx] - r0;
  if (nr && (!b->refs || !b->ref_state || !b->ref_by)) return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L.mu);
  if (commit_log_full(L, b->n_refs)) return CORDAHIP_ERR_LOG_FULL;
  Device& d = *L.dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  // the stage: inputs, then outputs, every array at a 16-byte boundary
  size_t pos = 0;
  const auto take = [&](size_t bytes) {
    const size_t at = pos;
    pos = (pos + bytes + 15) & ~(size_t)15;
    return at;
  };
  const size_t o_txid = take(ntx * 32), o_caller = take(ntx * 4), o_refs = take(nr * kCommitRefBytes),
               o_off = take((ntx + 1) * 8), o_from = take(b->tw_from ? ntx * 8 : 0),
               o_until = take(b->tw_from ? ntx * 8 : 0), o_gate = take(b->gate ? ntx : 0), in_bytes = pos,
               o_status = take(ntx), o_comm = take(ntx), o_state = take(nr), o_by = take(nr * kCommitByBytes);
  if (const int rc = commit_stage(L, pos)) return rc;
  if (commit_scratch(L, ntx, nr) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t *h = L.stage_h.as<uint8_t>(), *dv = L.stage_d.as<uint8_t>();
  std::memcpy(h + o_txid, b->txid, ntx * 32);
  std::memcpy(h + o_caller, b->caller, ntx * 4);
  if (nr) std::memcpy(h + o_refs, b->refs + r0, nr * kCommitRefBytes);
  uint64_t* off = reinterpret_cast<uint64_t*>(h + o_off);
  for (uint64_t t = 0; t <= ntx; t++) off[t] = b->tx_ref_off[t] - r0;
  if (b->tw_from) {
    std::memcpy(h + o_from, b->tw_from, ntx * 8);
    std::memcpy(h + o_until, b->tw_until, ntx * 8);
  }
  if (b->gate) std::memcpy(h + o_gate, b->gate, ntx);
  commit::Batch B{};
  B.ntx = ntx;
  B.txid = reinterpret_cast<const uint32_t*>(dv + o_txid);
  B.caller = reinterpret_cast<const uint32_t*>(dv + o_caller);
  B.refs = reinterpret_cast<const uint32_t*>(dv + o_refs);
  B.off = reinterpret_cast<const uint64_t*>(dv + o_off);
  B.tw_from = b->tw_from ? reinterpret_cast<const int64_t*>(dv + o_from) : nullptr;
  B.tw_until = b->tw_from ? reinterpret_cast<const int64_t*>(dv + o_until) : nullptr;
  B.now_ns = b->now_ns;
  B.tolerance_ns = b->tolerance_ns;
  B.gate = b->gate ? dv + o_gate : nullptr;
  B.tx_status = dv + o_status;
  B.committed = dv + o_comm;
  B.ref_state = dv + o_state;
  B.ref_by = reinterpret_cast<uint32_t*>(dv + o_by);
  hipStream_t s = d.stream;
  const double t0 = now_ms();
  hipError_t e = hipMemcpyAsync(dv, h, in_bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    e = commit_enqueue(L, B, nr, s);
    L.bound += b->n_refs - nr;  // the bound counts the call's n_refs, as the device form's must
  }
  e = e ? e : hipMemcpyAsync(h + o_status, dv + o_status, pos - o_status, hipMemcpyDeviceToHost, s);
  e = e ? e : L.stage_ev.record(s);
  e = e ? e : L.stage_ev.sync();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);  // no queued work outlives the call
    return CORDAHIP_ERR_HIP;
  }
  std::memcpy(b->tx_status, h + o_status, ntx);
  std::memcpy(b->committed, h + o_comm, ntx);
  if (nr) {
    std::memcpy(b->ref_state + r0, h + o_state, nr);
    std::memcpy(b->ref_by + r0, h + o_by, nr * kCommitByBytes);
  }
  if (tracing())
    fprintf(stderr, "[cordahip] dev %d commit log %u: %llu txs, %llu refs in %.2f ms\n", d.id, L.id,
            (unsigned long long)ntx, (unsigned long long)nr, now_ms() - t0);
  return CORDAHIP_SUCCESS;
}

int commit_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* b) {
  const auto L = log_at(ctx, log_id);
  return L ? commit_on(ctx, *L, b) : CORDAHIP_ERR_INVALID_ARG;
}

// The ticketed form: the call takes the log's next turn at submit, and the queued
// jobs of one log run in turn order whichever worker picks them up (the pool's queue
// is first in, first out, so the job whose turn it is has always been picked up).
template <class F>
int submit_in_turn(cordahip_ctx* ctx, const std::shared_ptr<CommitLog>& L, uint64_t* ticket, F run) {
  if (!L) return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L->turn_mu);
  const uint64_t turn = L->turn_next;
  *ticket = submit_job(ctx, [L, turn, run] {
    {
      std::unique_lock<std::mutex> w(L->turn_mu);
      L->turn_cv.wait(w, [&] { return L->turn_now == turn; });
    }
    const int rc = guarded([&] { return run(*L); });
    {
      std::lock_guard<std::mutex> w(L->turn_mu);
      L->turn_now++;
    }
    L->turn_cv.notify_all();
    return rc;
  });
  L->turn_next++;  // only once the job is queued: a failed submit leaves no gap in the turns
  return CORDAHIP_SUCCESS;
}
int commit_submit_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* b, uint64_t* ticket) {
  return submit_in_turn(ctx, log_at(ctx, log_id), ticket,
                        [ctx, copy = *b](CommitLog& L) { return commit_on(ctx, L, &copy); });
}

// ---- typed notary tear-offs: K21 + K6, then K16 over the same device rows -----------
// What cordahip_notary_tearoff_commit takes beside the batch (by value in a ticket's job).
struct NotaryCommitArgs {
  const uint32_t* caller;
  int64_t now_ns, tolerance_ns;
  const uint8_t* gate;
  uint8_t* committed;
  uint8_t* ref_state;
  cordahip_consuming_tx* ref_by;
};

int notary_commit_on(cordahip_ctx* ctx, CommitLog& L, const cordahip_notary_tearoff_batch* b,
                     const NotaryCommitArgs& a) {
  cordahip_commit_batch scal{};
  scal.now_ns = a.now_ns, scal.tolerance_ns = a.tolerance_ns;
  if (!commit_scalars_ok(&scal) || !check_notary_tearoff(PoolPar{*ctx->host}, b))
    return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  const uint64_t ntx = b->ntx;
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!notary_pointers_ok(b) || !a.caller || !a.committed) return CORDAHIP_ERR_INVALID_ARG;
  NotaryStage st(b, 0, ntx);
  const uint64_t nr = st.nr;
  if (nr && (!a.ref_state || !a.ref_by)) return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L.mu);
  if (commit_log_full(L, b->n_refs)) return CORDAHIP_ERR_LOG_FULL;
  Device& d = *L.dev;
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  // K16's arrays behind the tear-offs': two more inputs, its gate and statuses, its outputs
  const size_t o_caller = st.take(ntx * 4), o_cgate = st.take(a.gate ? ntx : 0), in2_end = st.pos,
               o_gate = st.take(ntx), o_cst = st.take(ntx), o_status = st.take(ntx), o_comm = st.take(ntx),
               o_state = st.take(nr), o_by = st.take(nr * kCommitByBytes), out2_end = st.pos;
  st.scratch();
  if (const int rc = commit_stage(L, st.host_bytes, st.pos)) return rc;
  if (commit_scratch(L, ntx, nr) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t *h = L.stage_h.as<uint8_t>(), *dv = L.stage_d.as<uint8_t>();
  st.fill(b, h);
  std::memcpy(h + o_caller, a.caller, ntx * 4);
  if (a.gate) std::memcpy(h + o_cgate, a.gate, ntx);
  commit::Batch B{};
  B.ntx = ntx;
  B.txid = reinterpret_cast<const uint32_t*>(dv + st.o_root);  // FilteredTransaction.rootHash is the id
  B.caller = reinterpret_cast<const uint32_t*>(dv + o_caller);
  B.refs = reinterpret_cast<const uint32_t*>(dv + st.o_refs);  // the rows K21 hashed
  B.off = reinterpret_cast<const uint64_t*>(dv + st.o_off);
  B.tw_from = reinterpret_cast<const int64_t*>(dv + st.o_twf);
  B.tw_until = reinterpret_cast<const int64_t*>(dv + st.o_twu);
  B.now_ns = a.now_ns;
  B.tolerance_ns = a.tolerance_ns;
  B.gate = dv + o_gate;
  B.tx_status = dv + o_cst;
  B.committed = dv + o_comm;
  B.ref_state = dv + o_state;
  B.ref_by = reinterpret_cast<uint32_t*>(dv + o_by);
  hipStream_t s = d.stream;
  const double t0 = now_ms();
  hipError_t e = hipMemcpyAsync(dv, h, st.in_bytes, hipMemcpyHostToDevice, s);
  e = e ? e : hipMemcpyAsync(dv + o_caller, h + o_caller, in2_end - o_caller, hipMemcpyHostToDevice, s);
  e = e ? e : st.enqueue_verify(dv, b->leaf_hash != nullptr, s);
  e = e ? e : launch_notary_gate(dv + st.o_vst, a.gate ? dv + o_cgate : nullptr, dv + o_gate, ntx, s);
  if (e == hipSuccess) {
    e = commit_enqueue(L, B, nr, s);
    L.bound += b->n_refs - nr;  // the bound counts the call's n_refs, as cordahip_commit_inputs's
  }
  e = e ? e : launch_notary_status(dv + st.o_vst, dv + o_cst, dv + o_status, ntx, s);
  if (b->leaf_hash) e = e ? e : hipMemcpyAsync(h + st.o_lh, dv + st.o_lh, st.out_end - st.o_lh, hipMemcpyDeviceToHost, s);
  e = e ? e : hipMemcpyAsync(h + o_status, dv + o_status, out2_end - o_status, hipMemcpyDeviceToHost, s);
  e = e ? e : L.stage_ev.record(s);
  e = e ? e : L.stage_ev.sync();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);  // no queued work outlives the call
    return CORDAHIP_ERR_HIP;
  }
  std::memcpy(b->tx_status, h + o_status, ntx);
  std::memcpy(a.committed, h + o_comm, ntx);
  if (nr) {
    std::memcpy(a.ref_state + st.r0, h + o_state, nr);
    std::memcpy(a.ref_by + st.r0, h + o_by, nr * kCommitByBytes);
  }
  if (b->leaf_hash) std::memcpy(b->leaf_hash, h + st.o_lh, NotaryStage::leaves_before(b, ntx) * 32);
  if (tracing())
    fprintf(stderr, "[cordahip] dev %d notary tear-offs on log %u: %llu txs, %llu refs in %.2f ms\n", d.id, L.id,
            (unsigned long long)ntx, (unsigned long long)nr, now_ms() - t0);
  return CORDAHIP_SUCCESS;
}

int commit_device_impl(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* b, void* hip_stream) {
  const auto L = log_at(ctx, log_id);
  if (!L || !commit_scalars_ok(b)) return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t ntx = b->ntx;
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!b->txid || !b->caller || !b->tx_ref_off || !b->tx_status || !b->committed ||
      (b->n_refs && (!b->refs || !b->ref_state || !b->ref_by)))
    return CORDAHIP_ERR_INVALID_ARG;
  const auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(b->txid, 4) || mis(b->caller, 4) || mis(b->refs, 4) || mis(b->ref_by, 4) || mis(b->tx_ref_off, 8) ||
      mis(b->tw_from, 8) || mis(b->tw_until, 8))
    return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(L->mu);
  if (commit_log_full(*L, b->n_refs)) return CORDAHIP_ERR_LOG_FULL;
  commit::Batch B{};
  B.ntx = ntx;
  B.txid = reinterpret_cast<const uint32_t*>(b->txid);
  B.caller = b->caller;
  B.refs = reinterpret_cast<const uint32_t*>(b->refs);
  B.off = b->tx_ref_off;
  B.tw_from = b->tw_from;
  B.tw_until = b->tw_until;
  B.now_ns = b->now_ns;
  B.tolerance_ns = b->tolerance_ns;
  B.gate = b->gate;
  B.tx_status = b->tx_status;
  B.committed = b->committed;
  B.ref_state = b->ref_state;
  B.ref_by = reinterpret_cast<uint32_t*>(b->ref_by);
  return device_call(
      *L->dev, hip_stream, [&] { return commit_scratch(*L, ntx, b->n_refs); },
      [&](hipStream_t s) { return commit_enqueue(*L, B, b->n_refs, s); });
}

}  // namespace

extern "C" {

int cordahip_commit_log_create(cordahip_ctx* ctx, int device, uint32_t capacity_log2, const uint8_t salt[16],
                               uint32_t* log_id) {
  if (!ctx || !log_id) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_create_impl(ctx, device, capacity_log2, salt, log_id); });
}

int cordahip_commit_log_destroy(cordahip_ctx* ctx, uint32_t log_id) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_destroy_impl(ctx, log_id); });
}

int cordahip_commit_log_reserve(cordahip_ctx* ctx, uint32_t log_id, uint32_t capacity_log2) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_reserve_impl(ctx, log_id, capacity_log2); });
}

int cordahip_commit_log_stats(cordahip_ctx* ctx, uint32_t log_id, uint64_t* entries, uint64_t* capacity,
                              uint64_t* next_seq) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_stats_impl(ctx, log_id, entries, capacity, next_seq); });
}

int cordahip_commit_log_load(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                             uint64_t* n_already_present) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_load_impl(ctx, log_id, rows, n, n_already_present); });
}

int cordahip_commit_log_lookup(cordahip_ctx* ctx, uint32_t log_id, const cordahip_state_ref* refs, uint64_t n,
                               uint8_t* present, cordahip_consuming_tx* by) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_lookup_impl(ctx, log_id, refs, n, present, by); });
}

int cordahip_commit_log_revoke(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                               uint8_t* revoked, uint64_t* n_removed) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_revoke_impl(ctx, log_id, rows, n, revoked, n_removed); });
}

int cordahip_commit_log_export(cordahip_ctx* ctx, uint32_t log_id, uint64_t since_seq, cordahip_commit_row* rows,
                               uint64_t* seq, uint64_t cap, uint64_t* n_total) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_log_export_impl(ctx, log_id, since_seq, rows, seq, cap, n_total); });
}

int cordahip_commit_inputs(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_impl(ctx, log_id, batch); });
}

int cordahip_commit_inputs_submit(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* batch,
                                  uint64_t* ticket) {
  if (!ctx || !batch || !ticket) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_submit_impl(ctx, log_id, batch, ticket); });
}

int cordahip_commit_inputs_device(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* d_batch,
                                  void* hip_stream) {
  if (!ctx || !d_batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return commit_device_impl(ctx, log_id, d_batch, hip_stream); });
}

int cordahip_notary_tearoff_commit(cordahip_ctx* ctx, uint32_t log_id, const cordahip_notary_tearoff_batch* batch,
                                   const uint32_t* caller, int64_t now_ns, int64_t tolerance_ns, const uint8_t* gate,
                                   uint8_t* committed, uint8_t* ref_state, cordahip_consuming_tx* ref_by) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  const NotaryCommitArgs a{caller, now_ns, tolerance_ns, gate, committed, ref_state, ref_by};
  return guarded([&] {
    const auto L = log_at(ctx, log_id);
    return L ? notary_commit_on(ctx, *L, batch, a) : (int)CORDAHIP_ERR_INVALID_ARG;
  });
}

int cordahip_notary_tearoff_commit_submit(cordahip_ctx* ctx, uint32_t log_id,
                                          const cordahip_notary_tearoff_batch* batch, const uint32_t* caller,
                                          int64_t now_ns, int64_t tolerance_ns, const uint8_t* gate, uint8_t* committed,
                                          uint8_t* ref_state, cordahip_consuming_tx* ref_by, uint64_t* ticket) {
  if (!ctx || !batch || !ticket) return CORDAHIP_ERR_INVALID_ARG;
  const NotaryCommitArgs a{caller, now_ns, tolerance_ns, gate, committed, ref_state, ref_by};
  return guarded([&] {
    return submit_in_turn(ctx, log_at(ctx, log_id), ticket,
                          [ctx, copy = *batch, a](CommitLog& L) { return notary_commit_on(ctx, L, &copy, a); });
  });
}

}  // extern "C"
