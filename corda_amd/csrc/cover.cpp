// cordahip_cover_eval_host: the required-signer coverage rule on the host, with
// no context and no device work (include/cordahip.h; the evaluator is
// cover_core.hpp, the same code the GPU kernel and the covered signed-tx calls
// run). The JVM's fallback path, and the CPU suite's way into the core.
#include "cover_core.hpp"
#include "csr_check.hpp"

namespace {
struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};
}  // namespace

extern "C" int cordahip_cover_eval_host(const cordahip_cover* cover, uint64_t ntx, uint8_t* tx_status,
                                        const uint64_t* tx_sig_off, const uint8_t* scheme, const uint8_t* key,
                                        const uint64_t* key_off, uint64_t nsig, uint64_t key_bytes) {
  using namespace cordahip;
  if (!cover) return CORDAHIP_ERR_INVALID_ARG;
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!tx_status || !tx_sig_off) return CORDAHIP_ERR_INVALID_ARG;
  const SerialPar par;
  if (!rt::check_cover(par, cover, ntx)) return CORDAHIP_ERR_INVALID_ARG;
  // the signature level: tx_sig_off within nsig, the keys it spans within key_bytes
  if (!rt::csr_ok(par, tx_sig_off, 0, ntx, nsig)) return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t s0 = tx_sig_off[0], s1 = tx_sig_off[ntx];
  if (s0 != s1 && (!scheme || !key_off || !rt::csr_ok(par, key_off, s0, s1, key_bytes) || (key_off[s1] && !key)))
    return CORDAHIP_ERR_INVALID_ARG;
  const cover::SigKeysCsr sig{scheme, key, key_off};
  cover::LocalStack stack;
  for (uint64_t t = 0; t < ntx; t++) cover::tx_eval(*cover, t, tx_status, tx_sig_off, sig, stack);
  return stack.failed ? CORDAHIP_ERR_OUT_OF_MEMORY : CORDAHIP_SUCCESS;
}
