// CPU check of the registered RSA keys' record and schedule (corda_amd/csrc/rsa_vkey.hpp,
// no HIP), built by tests/test_rsa_vkey_record.py with -fsanitize=address,undefined.
//
// It reads commands from standard input, one per line, and answers each with one JSON line:
//   key <hex DER>            a key in its wire form (the SPKI BIT STRING payload)
//   mod <words> <hex n> <e>  a modulus given as a number, in the width class `words`
// For a key that decodes (and for every `mod`) it builds the record, prints n', K, the bit
// length and the class, and runs modexp_keyed against rsa::modexp on in = 0, 1, n - 1 and
// random values below n ("mismatch": how many outputs differ), prints one random input with
// its output, and checks that in = n and in > n are refused with a zero row. For a key that
// does not decode it prints parse_public_key's status and whether the record, filled with a
// pattern beforehand, was left untouched.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../corda_amd/csrc/rsa_vkey.hpp"

using namespace cordahip;

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out(h.size() / 2);
  for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return out;
}

static std::string hex_words(const uint32_t* w, uint32_t n) {  // most significant digit first
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint32_t i = n; i-- > 0;)
    for (int q = 7; q >= 0; q--) s.push_back(d[(w[i] >> (4 * q)) & 15]);
  return s;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

// a random value below n (w words; n's top bit is bit `bits - 1`)
static void random_below(const rsa::VkeyRecord& rec, uint32_t* x) {
  const uint32_t w = rec.words;
  do {
    std::memset(x, 0, 4 * (size_t)rsa::kMaxWords);
    for (uint32_t i = 0; i < (rec.bits + 31) / 32; i++) x[i] = rnd32();
    if (rec.bits & 31) x[(rec.bits - 1) >> 5] &= (1u << (rec.bits & 31)) - 1;
  } while (rsa::cmp_words(x, rec.n, w) >= 0);
}

static void report(const rsa::VkeyRecord& rec) {
  const uint32_t w = rec.words;
  uint32_t in[rsa::kMaxWords], a[rsa::kMaxWords], b[rsa::kMaxWords], shown_in[rsa::kMaxWords], shown_out[rsa::kMaxWords];
  int mismatch = 0, refused = 0;
  for (int t = 0; t < 7; t++) {
    std::memset(in, 0, sizeof in);
    if (t == 1) in[0] = 1;
    if (t == 2) {
      std::memcpy(in, rec.n, 4 * (size_t)w);
      in[0] -= 1;  // n is odd
    }
    if (t >= 3) random_below(rec, in);
    const bool ra = rsa::modexp_keyed(rec, in, a), rb = rsa::modexp(rec.n, rec.e, in, w, b);
    if (!ra || !rb || std::memcmp(a, b, 4 * (size_t)w) != 0) mismatch++;
    if (t == 3) {
      std::memcpy(shown_in, in, sizeof in);
      std::memcpy(shown_out, a, sizeof a);
    }
  }
  // in = n, and in = n + 2 where it fits the row
  std::memset(in, 0, sizeof in);
  std::memcpy(in, rec.n, 4 * (size_t)w);
  for (int t = 0; t < 2; t++) {
    bool fits = true;
    if (t == 1) {
      uint64_t c = 2;
      for (uint32_t i = 0; i < w && c; i++) {
        c += in[i];
        in[i] = (uint32_t)c;
        c >>= 32;
      }
      fits = c == 0;
    }
    if (!fits) {
      refused++;  // n + 2 needs more than the row: not an operand at all
      continue;
    }
    std::memset(a, 0xff, sizeof a);
    bool zero = !rsa::modexp_keyed(rec, in, a);
    for (uint32_t i = 0; i < w; i++) zero = zero && a[i] == 0;
    refused += zero;
  }
  std::printf("{\"status\": 0, \"np\": %u, \"e\": %u, \"bits\": %u, \"words\": %u, \"n\": \"%s\", \"K\": \"%s\", "
              "\"mismatch\": %d, \"refused\": %d, \"in\": \"%s\", \"out\": \"%s\"}\n",
              rec.np, rec.e, rec.bits, rec.words, hex_words(rec.n, rsa::kMaxWords).c_str(),
              hex_words(rec.K, rsa::kMaxWords).c_str(), mismatch, refused, hex_words(shown_in, w).c_str(),
              hex_words(shown_out, w).c_str());
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    rsa::VkeyRecord rec, pattern;
    std::memset(&pattern, 0xA5, sizeof pattern);
    rec = pattern;
    if (cmd == "key") {
      std::string h;
      std::cin >> h;
      if (h == "-") h.clear();  // the empty key
      const std::vector<uint8_t> der = unhex(h);
      const uint8_t ks = rsa::vkey_record_from_der(der.data(), der.size(), rec);
      if (ks != rsa::kOk) {
        std::printf("{\"status\": %u, \"untouched\": %s}\n", ks,
                    std::memcmp(&rec, &pattern, sizeof rec) == 0 ? "true" : "false");
        continue;
      }
      report(rec);
    } else if (cmd == "mod") {
      uint32_t words, e;
      std::string h;
      std::cin >> words >> h >> e;
      std::vector<uint8_t> be = unhex(h.size() & 1 ? "0" + h : h);
      rsa::PublicKey pk;
      if (!rsa::os2ip(be.data(), be.size(), pk.n, rsa::kMaxWords)) return 2;
      pk.e = e;
      pk.words = words;
      uint32_t hi = rsa::kMaxWords;
      while (hi > 0 && pk.n[hi - 1] == 0) hi--;
      if (hi == 0 || hi > words) return 2;
      pk.bits = (hi - 1) * 32;
      for (uint32_t v = pk.n[hi - 1]; v; v >>= 1) pk.bits++;
      rsa::build_vkey_record(pk, rec);
      report(rec);
    } else {
      return 2;
    }
  }
  return 0;
}
