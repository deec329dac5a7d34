// Host check of the keyed ECDSA verifier's window geometry
// (corda_amd/csrc/ecdsa_vkey.hpp) and of its host packing (pack_rows.hpp
// keyed_ec_pack_rows), built with ASan + UBSan by tests/test_ec_vkey_windows.py.
// For both curves' n and every scalar u < n below:
//   the sign flag is (u >= 2^255) and the magnitude u' = flag ? n - u : u is < 2^255,
//   the biased sum has no carry out, the 32 signed digits satisfy |d_j| <= 128,
//   sum_j d_j 256^j == u' (compared as 256-bit integers),
//   the byte-by-byte form (vkey_step) yields the same digits,
//   every nonzero digit's entry offset, plus an entry, stays inside the key's table.
//   fixed: 1, n - 1, 2^255 - 1, 2^255, 2^255 + 1; bytes all 0x80, all 0x81, all 0xff
//   (reduced mod n); random: <count> seeded 256-bit values reduced mod n.
// Then the table and record offsets, and keyed_ec_pack_rows over CSR batches whose
// every input and output lives in a heap block of exactly its size: signatures of 0,
// 8, 72, 73 and 300 bytes (the long ones well-formed DER and not), dense and
// ragged messages, both flags values.
// Usage: ec_vkey_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/ecdsa_vkey.hpp"
#include "../corda_amd/csrc/pack_rows.hpp"

using namespace cordahip;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct scalar {
  uint32_t w[8];
};

static bool geq(const uint32_t a[8], const uint32_t b[8]) {
  for (int i = 7; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}
static void sub(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)a[i] - b[i] - br;
    r[i] = (uint32_t)t;
    br = (t >> 32) & 1u;
  }
}
static scalar reduced(scalar s, const uint32_t n[8]) {  // n > 2^255: one subtraction
  if (geq(s.w, n)) sub(s.w, s.w, n);
  return s;
}

// acc += d * 256^j over 9 words of two's complement (room for the intermediate sign)
static void add_digit(uint32_t acc[9], int d, int j) {
  int64_t carry = 0;
  const int word = j >> 2, sh = 8 * (j & 3);
  const int64_t v = (int64_t)d * ((int64_t)1 << sh);  // |v| <= 2^31
  for (int i = word; i < 9; i++) {
    int64_t t = (int64_t)acc[i] + carry;
    if (i == word) t += v;
    acc[i] = (uint32_t)((uint64_t)t & 0xffffffffu);
    carry = t >> 32;  // arithmetic shift: floor division
  }
}

static uint64_t checked = 0, max_abs = 0, min_digit = 0, max_digit = 0, zero_digits = 0, negated = 0;

static bool check(const scalar& s, const uint32_t n[8], const char* what) {
  if (geq(s.w, n)) {
    fprintf(stderr, "%s: not below n\n", what);
    return false;
  }
  int16_t d[kVkeyDigits];
  bool neg;
  if (ec_vkey_recode(d, neg, s.w, n)) {
    fprintf(stderr, "%s: carry out of the biased sum\n", what);
    return false;
  }
  if (neg != ((s.w[7] >> 31) != 0)) {
    fprintf(stderr, "%s: sign flag\n", what);
    return false;
  }
  uint32_t mag[8], up[8], t[8];
  if (neg) sub(mag, n, s.w);
  else memcpy(mag, s.w, 32);
  if (mag[7] >> 31) {
    fprintf(stderr, "%s: magnitude not below 2^255\n", what);
    return false;
  }
  if (ec_vkey_split_sign(up, s.w, n) != neg || memcmp(up, mag, 32) != 0) {
    fprintf(stderr, "%s: split_sign\n", what);
    return false;
  }
  ec_vkey_bias(t, up);
  negated += neg;
  uint32_t acc[9] = {0}, c = 0;
  for (int j = 0; j < kVkeyDigits; j++) {
    const int a = d[j] < 0 ? -d[j] : d[j];
    if (a > kVkeyEntries) {
      fprintf(stderr, "%s: digit %d is %d\n", what, j, d[j]);
      return false;
    }
    if ((uint64_t)a > max_abs) max_abs = a;
    if (d[j] < 0 && (uint64_t)-d[j] > min_digit) min_digit = -d[j];
    if (d[j] > 0 && (uint64_t)d[j] > max_digit) max_digit = d[j];
    zero_digits += a == 0;
    if (vkey_digit(t[j >> 2], j) != d[j]) {  // the kernel's form
      fprintf(stderr, "%s: the biased-word form differs at digit %d\n", what, j);
      return false;
    }
    if (vkey_step((mag[j >> 2] >> (8 * (j & 3))) & 0xffu, c) != d[j]) {  // byte plus carry
      fprintf(stderr, "%s: the byte-by-byte form differs at digit %d\n", what, j);
      return false;
    }
    if (a && (uint64_t)ec_vkey_entry_word(j, a) + kEcVkeyEntryWords > kEcVkeyTableWords) {
      fprintf(stderr, "%s: digit %d = %d reads outside the table\n", what, j, d[j]);
      return false;
    }
    add_digit(acc, d[j], j);
  }
  if (c != 0 || acc[8] != 0 || memcmp(acc, mag, 32) != 0) {
    fprintf(stderr, "%s: digits do not sum to the magnitude\n", what);
    return false;
  }
  checked++;
  return true;
}

static bool check_geometry() {
  if (ec_vkey_entry_word(0, 1) != 0) return false;
  if (ec_vkey_entry_word(kVkeyDigits - 1, kVkeyEntries) + kEcVkeyEntryWords != kEcVkeyTableWords) return false;
  if (kEcVkeyEntryWords % 4 != 0 || kEcVkeyTableWords % 4 != 0) return false;  // 16-byte loads
  // the keys' tables, then the two base points', then the records, then the scratch
  if (kEcVkeyBaseSlotK1 != kVkeySlots || kEcVkeyBaseSlotR1 != kVkeySlots + 1 || kEcVkeyTables != kVkeySlots + 2) return false;
  if (ec_vkey_base_slot(2) != kEcVkeyBaseSlotK1 || ec_vkey_base_slot(3) != kEcVkeyBaseSlotR1) return false;
  if ((uint64_t)kEcVkeyTables * kEcVkeyTableWords != kEcVkeyRecBase) return false;
  if (kEcVkeyRecBase + kVkeySlots * kEcVkeyRecWords != kEcVkeyKeyWord) return false;
  if ((kEcVkeyOkWord - kEcVkeyKeyWord) * 4 < kEcVkeyMaxKeyBytes || kEcVkeyOkWord + 4 != kEcVkeyAllWords) return false;
  if ((uint64_t)kEcVkeyAllWords * 4 > 0xffffffffull) return false;
  // the order of additions: 64 of them, positions 31..0, base point before key
  int seen[2][kVkeyDigits] = {};
  for (int k = 0; k < 2 * kVkeyDigits; k++) {
    const int j = ec_vkey_add_pos(k);
    if (j < 0 || j >= kVkeyDigits || (k && j > ec_vkey_add_pos(k - 1))) return false;
    if (ec_vkey_add_is_key(k) != (k % 2 == 1)) return false;
    seen[ec_vkey_add_is_key(k)][j]++;
  }
  for (int j = 0; j < kVkeyDigits; j++)
    if (seen[0][j] != 1 || seen[1][j] != 1) return false;
  return ec_vkey_add_pos(0) == 31 && !ec_vkey_add_is_key(0);
}

// ---- keyed_ec_pack_rows -----------------------------------------------------
template <class T>
static std::unique_ptr<T[]> exact(size_t n) {  // exactly n elements: ASan sees any access past them
  return std::unique_ptr<T[]>(new T[n ? n : 1]);
}

static std::vector<uint8_t> der_long(size_t total, bool well_formed) {
  std::vector<uint8_t> s;
  if (total == 73) {
    s = {0x30, 0x47, 0x02, 0x21, 0x00, 0x80};
    s.resize(2 + 2 + 33, 0x11);
    s.insert(s.end(), {0x02, 0x22, 0x00, 0xff});
    s.resize(73, 0x22);
  } else {  // 300
    s = {0x30, 0x82, 0x01, 0x28, 0x02, 0x81, 0x90, 0x01};
    s.resize(4 + 3 + 144, 0x33);
    s.insert(s.end(), {0x02, 0x81, 0x92, 0x01});
    s.resize(300, 0x44);
  }
  if (!well_formed) s[1] ^= 1;  // the SEQUENCE length no longer matches
  return s;
}

static uint64_t pack_lanes = 0;

static bool check_pack(bool is_valid, bool dense) {
  struct Lane {
    std::vector<uint8_t> sig, msg;
    uint8_t want_pre;
    uint8_t want_len;
  };
  const bool dv = !is_valid;
  std::vector<Lane> lanes;
  auto msg = [&](size_t i) { return std::vector<uint8_t>(dense ? 32 : (i * 7) % 45, (uint8_t)(i + 1)); };
  size_t i = 0;
  for (size_t sl : {(size_t)0, (size_t)8, (size_t)72}) {
    Lane l{std::vector<uint8_t>(sl, (uint8_t)(0x50 + i)), msg(i), CORDAHIP_STATUS_OK, (uint8_t)sl};
    lanes.push_back(l);
    i++;
  }
  for (size_t total : {(size_t)73, (size_t)300})
    for (bool wf : {true, false}) {
      Lane l{der_long(total, wf), msg(i), 0, 72};
      l.want_pre = (l.msg.empty() && dv) ? CORDAHIP_STATUS_EMPTY
                   : wf                  ? CORDAHIP_STATUS_BAD_SIG
                                         : CORDAHIP_STATUS_MALFORMED_SIG;
      lanes.push_back(l);
      i++;
    }
  if (!dense) {  // a long signature over an empty message: EMPTY under doVerify only
    Lane l{der_long(73, true), {}, dv ? (uint8_t)CORDAHIP_STATUS_EMPTY : (uint8_t)CORDAHIP_STATUS_BAD_SIG, 72};
    lanes.push_back(l);
  }
  const uint64_t n = lanes.size();
  size_t sb = 0, mb = 0;
  for (const Lane& l : lanes) sb += l.sig.size(), mb += l.msg.size();
  auto sig = exact<uint8_t>(sb), m = exact<uint8_t>(mb);
  auto so = exact<uint64_t>(n + 1), mo = exact<uint64_t>(n + 1);
  auto ids = exact<uint32_t>(n);
  so[0] = mo[0] = 0;
  for (uint64_t k = 0; k < n; k++) {
    if (!lanes[k].sig.empty()) memcpy(sig.get() + so[k], lanes[k].sig.data(), lanes[k].sig.size());
    if (!lanes[k].msg.empty()) memcpy(m.get() + mo[k], lanes[k].msg.data(), lanes[k].msg.size());
    so[k + 1] = so[k] + lanes[k].sig.size();
    mo[k + 1] = mo[k] + lanes[k].msg.size();
    ids[k] = (uint32_t)(1000 + k);
  }
  cordahip_keyed_sig_batch b;
  memset(&b, 0, sizeof b);
  b.n = n;
  b.key_id = ids.get();
  b.sig = sig.get();
  b.sig_off = so.get();
  b.msg = m.get();
  b.msg_off = mo.get();
  b.flags = is_valid ? CORDAHIP_FLAG_IS_VALID : 0;
  b.sig_bytes = sb;
  b.msg_bytes = mb;
  auto poff = exact<uint64_t>(n);
  const rt::SignLayout lay = rt::msg_chunk_layout(b.msg_off, 0, n, poff.get());
  if (lay.dense != dense) return false;
  auto hid = exact<uint32_t>(n);
  auto hsig = exact<uint8_t>(n * 72), hsl = exact<uint8_t>(n), hpre = exact<uint8_t>(n);
  auto hm = exact<uint8_t>(lay.bytes);
  auto ho = exact<uint64_t>(dense ? 0 : n);
  auto hl = exact<uint32_t>(dense ? 0 : n);
  // two pieces, as the pool's workers take them
  rt::keyed_ec_pack_rows(&b, 0, 0, n / 2, lay, poff.get(), hid.get(), hsig.get(), hsl.get(), hpre.get(), hm.get(),
                         ho.get(), hl.get());
  rt::keyed_ec_pack_rows(&b, 0, n / 2, n, lay, poff.get(), hid.get(), hsig.get(), hsl.get(), hpre.get(), hm.get(),
                         ho.get(), hl.get());
  for (uint64_t k = 0; k < n; k++) {
    const Lane& l = lanes[k];
    if (hid[k] != 1000 + k || hpre[k] != l.want_pre || hsl[k] != l.want_len) {
      fprintf(stderr, "pack lane %llu: id %u pre %u len %u\n", (unsigned long long)k, hid[k], hpre[k], hsl[k]);
      return false;
    }
    const uint8_t* slot = hsig.get() + k * 72;
    const size_t kept = l.sig.size() <= 72 ? l.sig.size() : 0;
    if (kept && memcmp(slot, l.sig.data(), kept) != 0) return false;
    for (size_t q = kept; q < 72; q++)
      if (slot[q]) return false;
    const uint64_t p = dense ? k * 32 : poff[k];
    if (!l.msg.empty() && memcmp(hm.get() + p, l.msg.data(), l.msg.size()) != 0) return false;
    if (!dense && (ho[k] != p || hl[k] != l.msg.size() || p % 16)) return false;
    pack_lanes++;
  }
  return true;
}

int main(int argc, char** argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  bool ok = check_geometry();
  if (!ok) fprintf(stderr, "geometry\n");
  uint64_t randoms = 0, fixed = 0;
  for (const uint32_t* n : {kEcVkeyNK1, kEcVkeyNR1}) {
    scalar s;
    memset(&s, 0, sizeof s);
    s.w[0] = 1;
    ok &= check(s, n, "1"), fixed++;
    memcpy(s.w, n, 32);
    s.w[0] -= 1;
    ok &= check(s, n, "n - 1"), fixed++;
    for (int i = 0; i < 8; i++) s.w[i] = 0xffffffffu;
    s.w[7] = 0x7fffffffu;
    ok &= check(s, n, "2^255 - 1"), fixed++;
    memset(&s, 0, sizeof s);
    s.w[7] = 0x80000000u;
    ok &= check(s, n, "2^255"), fixed++;
    s.w[0] = 1;
    ok &= check(s, n, "2^255 + 1"), fixed++;
    for (uint32_t v : {0x80u, 0x81u, 0xffu}) {
      for (int i = 0; i < 8; i++) s.w[i] = v * 0x01010101u;
      ok &= check(reduced(s, n), n, "equal bytes"), fixed++;
    }
    for (uint64_t k = 0; k < count; k++) {
      for (int i = 0; i < 8; i += 2) {
        const uint64_t r = rng();
        s.w[i] = (uint32_t)r;
        s.w[i + 1] = (uint32_t)(r >> 32);
      }
      ok &= check(reduced(s, n), n, "random");
      randoms++;
    }
  }
  bool pack_ok = true;
  for (bool is_valid : {false, true})
    for (bool dense : {true, false}) pack_ok &= check_pack(is_valid, dense);
  if (!pack_ok) fprintf(stderr, "keyed_ec_pack_rows\n");
  ok &= pack_ok;
  printf("{\"scalars\": %llu, \"fixed\": %llu, \"randoms\": %llu, \"negated\": %llu, \"max_abs\": %llu, "
         "\"most_negative\": %llu, \"most_positive\": %llu, \"zero_digits\": %llu, \"pack_lanes\": %llu, \"ok\": %s}\n",
         (unsigned long long)checked, (unsigned long long)fixed, (unsigned long long)randoms,
         (unsigned long long)negated, (unsigned long long)max_abs, (unsigned long long)min_digit,
         (unsigned long long)max_digit, (unsigned long long)zero_digits, (unsigned long long)pack_lanes,
         ok ? "true" : "false");
  return ok ? 0 : 1;
}
