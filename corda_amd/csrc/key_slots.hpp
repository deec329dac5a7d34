// The slots of a key registry (the signer's, cordahip_signer_*; the verification keys',
// cordahip_vkey_*): which slots hold a live key and each slot's reuse counter. A key id
// is slot | counter << SlotBits; a slot's counter moves on with every add, so the id of
// a removed key never matches the key that took its slot. No key material, and no HIP
// on the host: tools/key_slots_check.cpp runs this on the CPU.
#pragma once
#include <stdint.h>

#include <mutex>

#include "ed25519_comb.hpp"
#include "ed25519_vkey.hpp"

namespace cordahip {
namespace rt {

// NextGen: the counter of a slot's next key, given its last one (0: never used)
template <uint32_t SlotBits, uint32_t (*NextGen)(uint32_t)>
struct KeySlots {
  static constexpr uint32_t kSlots = 1u << SlotBits;
  std::mutex mu;  // held for an add's or a remove's whole run
  uint32_t gen[kSlots] = {};
  uint8_t live[kSlots] = {};
  uint32_t count = 0;

  static constexpr uint32_t make_id(uint32_t slot, uint32_t g) { return slot | (g << SlotBits); }
  // the first free slot and the id of its next key (false: every slot is live); the
  // counter is consumed even if the add then fails. commit(slot) makes the key live.
  bool acquire(uint32_t& slot, uint32_t& id) {
    if (count >= kSlots) return false;
    slot = 0;
    while (live[slot]) slot++;
    gen[slot] = NextGen(gen[slot]);
    id = make_id(slot, gen[slot]);
    return true;
  }
  void commit(uint32_t slot) {
    live[slot] = 1;
    count++;
  }
  // the slot of live key `id`, free from here on (false: no live key has that id)
  bool release(uint32_t id, uint32_t& slot) {
    slot = id & (kSlots - 1);
    if (!live[slot] || make_id(slot, gen[slot]) != id) return false;
    live[slot] = 0;
    count--;
    return true;
  }
};

// The verification keys' registry (cordahip_vkey_add_ed25519 / _add_ecdsa / _remove):
// one pool of slots for both families, counters 1 .. kVkeyGenMax, never 0
// (ed25519_vkey.hpp).
using VkeySlots = KeySlots<kVkeySlotBits, vkey_next_gen>;
// The signer's registry (cordahip_signer_add_ed25519 / _remove). Its counter counts up
// modulo 2^20 and so, unlike the verification keys', passes through 0: ids differ across
// a slot's keys until it wraps (2^20 adds into one slot). The signer's ids have always
// been issued this way and stay as they are.
constexpr uint32_t sign_next_gen(uint32_t gen) { return (gen + 1) & ((1u << (32 - kSignSlotBits)) - 1); }
using SignerSlots = KeySlots<kSignSlotBits, sign_next_gen>;

}  // namespace rt
}  // namespace cordahip
