// What the files that implement the C-ABI share (cordahip.cpp, keyed.cpp, commit_api.cpp):
// the host pool as a parallel runner, ticketed submission, and the frame of a *_device
// entry point. Internal: not part of include/cordahip.h, and hidden, so the library
// exports what it did when all of this sat in one file's anonymous namespace.
#pragma once
#include <functional>
#include <tuple>

#include "runtime.hpp"
#include "status.hpp"

#pragma GCC visibility push(hidden)
namespace cordahip {
namespace rt {

// the context's host pool as csr_check.hpp's parallel runner
struct PoolPar {
  HostPool& pool;
  template <class F>
  void operator()(uint64_t n, uint64_t grain, F&& fn) const {
    pool.parallel_for(n, grain, std::function<void(uint64_t, uint64_t)>(fn));
  }
};

// cordahip.cpp, beside the thread-local that cordahip_last_kernel_ms reads
uint64_t submit_job(cordahip_ctx* ctx, std::function<int()> fn);
TimedCall* timed_begin(Device& d, hipStream_t s);

// A *_submit call: its descriptors by value (their arrays stay caller-owned) into a
// queued job that runs impl(ctx, &copy...); the ticket.
template <class F, class... D>
int submit(cordahip_ctx* ctx, uint64_t* ticket, F impl, const D*... desc) {
  if (!ctx || !ticket || (... || !desc)) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] {
    *ticket = submit_job(ctx, [ctx, impl, copies = std::make_tuple(*desc...)] {
      return std::apply([&](const D&... c) { return impl(ctx, &c...); }, copies);
    });
    return (int)CORDAHIP_SUCCESS;
  });
}

// A *_device entry point once its arguments are checked: the call counts as activity
// on the device, the device is current, `prepare` grows what the call needs (device
// memory it could not get is CORDAHIP_ERR_OUT_OF_MEMORY), and the call's timing pair
// brackets what `enqueue` puts on the caller's stream (NULL: the device's null stream).
template <class P, class F>
int device_call(Device& d, void* hip_stream, P&& prepare, F&& enqueue) {
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (const hipError_t e = prepare()) return e == hipErrorOutOfMemory ? CORDAHIP_ERR_OUT_OF_MEMORY : CORDAHIP_ERR_HIP;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  TimedCall* tc = timed_begin(d, s);
  if (!tc) return CORDAHIP_ERR_HIP;
  hipError_t e = enqueue(s);
  e = e ? e : hipEventRecord(tc->b, s);
  return hip_err(e);
}
template <class F>
int device_call(Device& d, void* hip_stream, F&& enqueue) {
  return device_call(d, hip_stream, [] { return hipSuccess; }, enqueue);
}

inline Device* dev_at(cordahip_ctx* ctx, int device) {
  if (!ctx || device < 0 || device >= (int)ctx->devs.size()) return nullptr;
  return ctx->devs[device].get();
}

// a *_device entry point's void pointers: p is not a multiple of `align` (a power of
// two; NULL is aligned), and p as the kernels' element type
inline bool misaligned(const void* p, uintptr_t align) { return (reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0; }
template <class T>
const T* ptr(const void* p) {
  return static_cast<const T*>(p);
}
template <class T>
T* ptr(void* p) {
  return static_cast<T*>(p);
}

}  // namespace rt
}  // namespace cordahip
#pragma GCC visibility pop
