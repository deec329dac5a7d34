// Per-lane verdict statuses — the data half of the C-ABI contract
// (include/cordahip.h CORDAHIP_STATUS_*). Mapping to the reference's
// exceptions: SURVEY.md §8(b) "Per-lane status -> Kotlin semantics".
#pragma once
#include <stdint.h>

namespace cordahip {
static constexpr uint8_t kStatusOk = 0;           // isValid true / doVerify true
static constexpr uint8_t kStatusBadSig = 1;       // isValid false / doVerify SignatureException
static constexpr uint8_t kStatusMalformedSig = 2; // engine SignatureException
static constexpr uint8_t kStatusBadKey = 3;       // key decode IllegalArgumentException
static constexpr uint8_t kStatusUnsupported = 4;  // IllegalArgumentException (scheme)
static constexpr uint8_t kStatusEmpty = 5;        // IllegalArgumentException (empty input)
// signing lanes (CORDAHIP_SIGN_*)
static constexpr uint8_t kSignUnknownKey = 14;    // no such key in the registry (KMS lookup fails)
static constexpr uint8_t kSignSkipped = 15;       // the lane's gate byte was nonzero
static constexpr uint8_t kSignFailed = 16;        // ECDSA: every nonce candidate of the bounded loop was rejected; RSA: the fault check failed
// keyed verification lanes (CORDAHIP_VERIFY_UNKNOWN_KEY)
static constexpr uint8_t kVerifyUnknownKey = 16;  // no such key in the verification-key registry
}  // namespace cordahip
