// The typed rows of a batch of notary tear-offs as K21 (kryo_device.hip) takes them:
// device pointers to cordahip_notary_tearoff_batch's input arrays.
#pragma once
#include <stdint.h>

#include "../../include/cordahip.h"

namespace cordahip {

struct NotaryRows {
  uint64_t ntx, n_refs;
  const cordahip_state_ref* refs;  // [n_refs]
  const uint64_t* tx_ref_off;      // [ntx + 1]
  const uint8_t* tw_flags;         // [ntx]; nullptr: no windows
  const int64_t* tw_from_s;
  const int32_t* tw_from_nano;
  const int64_t* tw_until_s;
  const int32_t* tw_until_nano;
};

}  // namespace cordahip
