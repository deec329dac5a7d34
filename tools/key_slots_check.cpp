// The key registries' slot bookkeeping (corda_amd/csrc/key_slots.hpp KeySlots) in both
// geometries the library uses -- the verification keys' (6 slot bits, counters 1 ..
// kVkeyGenMax, never 0) and the signer's (12 slot bits, counters modulo 2^20, through 0)
// (VkeySlots, SignerSlots) -- host only, no GPU: tests/test_key_slots.py builds this with
// g++ -fsanitize=address,undefined and runs it.
//  a  adds fill the registry to its capacity, then it reports full; every id is distinct
//  b  release followed by acquire reuses the slot under a new id
//  c  a released id, kVkeyNoId and an id whose counter is stale are rejected, count unchanged
//  d  a failed add (acquire without commit) consumes the counter and leaves the slot free
//  e  the counter's wrap: after kVkeyGenMax comes 1; after 2^20 - 1 the signer's comes 0
// prints one JSON line; exit status 1 and a message on the first failed check
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../corda_amd/csrc/key_slots.hpp"

using namespace cordahip;

namespace {
void fail(const char* what, const char* name) {
  fprintf(stderr, "key_slots_check (%s): %s\n", name, what);
  exit(1);
}
#define CHECK(x) \
  if (!(x)) fail(#x, name)

// gen_max: the largest counter; after_max: the one that follows it
template <class Slots>
uint32_t run(const char* name, uint32_t bits, uint32_t gen_max, uint32_t after_max) {
  Slots r;
  const uint32_t cap = 1u << bits;
  CHECK(Slots::kSlots == cap);
  uint32_t slot = 0, id = 0, s2 = 0;
  CHECK(!r.release(0, slot) && !r.release(kVkeyNoId, slot) && r.count == 0);  // before the first add
  // a
  std::set<uint32_t> ids;
  for (uint32_t i = 0; i < cap; i++) {
    CHECK(r.acquire(slot, id) && slot == i && id == Slots::make_id(i, 1) && (id & (cap - 1)) == i);
    r.commit(slot);
    CHECK(r.count == i + 1 && ids.insert(id).second);
  }
  CHECK(!r.acquire(slot, id) && r.count == cap);  // full
  CHECK(!r.release(kVkeyNoId, slot) && r.count == cap);  // c: slot cap - 1 is live, under another counter
  // b, c
  const uint32_t victim = cap / 2 + 1, old_id = Slots::make_id(victim, 1);
  CHECK(r.release(old_id, slot) && slot == victim && r.count == cap - 1);
  CHECK(!r.release(old_id, slot) && r.count == cap - 1);  // released
  CHECK(r.acquire(slot, id) && slot == victim && id == Slots::make_id(victim, 2) && ids.insert(id).second);
  r.commit(slot);
  CHECK(r.count == cap);
  CHECK(!r.release(old_id, slot) && r.count == cap);                      // a stale counter
  CHECK(!r.release(Slots::make_id(victim, 3), slot) && r.count == cap);  // one not issued yet
  // d
  CHECK(r.release(id, slot) && slot == victim && r.count == cap - 1);
  CHECK(r.acquire(slot, id) && slot == victim && id == Slots::make_id(victim, 3));  // never committed
  CHECK(r.count == cap - 1 && !r.release(id, s2) && r.count == cap - 1);
  CHECK(r.acquire(slot, id) && slot == victim && id == Slots::make_id(victim, 4) && r.count == cap - 1);
  r.commit(slot);
  CHECK(r.count == cap && r.release(id, slot) && slot == victim);
  // e
  r.gen[victim] = gen_max;
  CHECK(r.acquire(slot, id) && slot == victim && id == Slots::make_id(victim, after_max));
  CHECK((id >> bits) == after_max && r.gen[victim] == after_max);
  r.commit(slot);
  CHECK(!r.release(Slots::make_id(victim, gen_max), s2) && r.count == cap);
  CHECK(r.release(id, slot) && slot == victim && r.count == cap - 1);
  return (uint32_t)ids.size();
}
}  // namespace

int main() {
  static_assert(kVkeySlotBits == 6 && kSignSlotBits == 12 && kSignKeySlots == 1u << kSignSlotBits, "the two geometries");
  const uint32_t nv = run<rt::VkeySlots>("vkey", 6, kVkeyGenMax, 1u);
  const uint32_t ns = run<rt::SignerSlots>("signer", 12, (1u << 20) - 1, 0u);
  printf("{\"vkey_ids\": %u, \"signer_ids\": %u}\n", nv, ns);
  return 0;
}
