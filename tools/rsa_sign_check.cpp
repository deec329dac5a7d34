// CPU check of the RSA signer's record and schedule (corda_amd/csrc/rsa_sign.hpp, no
// HIP), built by tests/test_rsa_sign_record.py with -fsanitize=address,undefined.
//
// It reads commands from standard input, one per line, and answers each with one JSON line.
// Every command starts with a key: <p> <q> <dP> <dQ> <qInv> as hex big-endian bytes (an odd
// number of digits gets a leading zero; "-" is a zero-length component) and <e> in decimal.
//   key  <key>                  build_sign_record's status; for a key it takes, every field of
//                               the record and whether sign_consistent() holds (what an add
//                               asks of a device)
//   raw  <key> <hex EM>         sign_raw on EM (at most the class's words): ok and s
//   half <key> <hex EM>         EM of up to 2 Wp words, any value (neither half need be below a
//                               prime): EM^dP mod p and EM^dQ mod q by half_exp, in plain form
//   sign <key> <hex msg> <hex salt>   the whole lane: ok and the k signature bytes
// A key that is declined answers {"status": ...} to every command.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../corda_amd/csrc/rsa_sign.hpp"

using namespace cordahip;

static std::vector<uint8_t> unhex(std::string h) {
  if (h == "-") return {};
  if (h.size() & 1) h = "0" + h;
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

static std::string hex_bytes(const uint8_t* b, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++) {
    s.push_back(d[b[i] >> 4]);
    s.push_back(d[b[i] & 15]);
  }
  return s;
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    std::string h[5];
    uint64_t e64;
    for (auto& x : h) std::cin >> x;
    std::cin >> e64;
    if (!std::cin || e64 > 0xffffffffull) return 2;
    std::vector<uint8_t> c[5];
    for (int i = 0; i < 5; i++) c[i] = unhex(h[i]);
    static const uint8_t none = 0;  // a zero-length component still has an address
    const auto at = [&](int i) { return c[i].empty() ? &none : c[i].data(); };
    const rsa::PrivateKeyIn in{at(0), at(1), at(2), at(3), at(4), (uint32_t)c[0].size(), (uint32_t)c[1].size(),
                               (uint32_t)c[2].size(), (uint32_t)c[3].size(), (uint32_t)c[4].size(), (uint32_t)e64};
    rsa::SignRecord rec;
    std::memset(&rec, 0xA5, sizeof rec);
    const uint8_t ks = rsa::build_sign_record(in, rec);
    std::string a, b;
    if (cmd == "raw" || cmd == "half") std::cin >> a;
    if (cmd == "sign") std::cin >> a >> b;
    if (ks != rsa::kOk) {
      bool zero = true;
      for (size_t i = 0; i < sizeof rec; i++) zero = zero && reinterpret_cast<const uint8_t*>(&rec)[i] == 0;
      std::printf("{\"status\": %u, \"zeroed\": %s}\n", ks, zero ? "true" : "false");
      continue;
    }
    const uint32_t W = rec.words;
    if (cmd == "key") {
      std::printf("{\"status\": 0, \"id\": %u, \"e\": %u, \"bits\": %u, \"words\": %u, \"np\": %u, \"npp\": %u, "
                  "\"npq\": %u, \"pbits\": %u, \"n\": \"%s\", \"K\": \"%s\", \"qR\": \"%s\", \"p\": \"%s\", "
                  "\"q\": \"%s\", \"dp\": \"%s\", \"dq\": \"%s\", \"qinv\": \"%s\", \"r2p\": \"%s\", \"r2q\": \"%s\", "
                  "\"consistent\": %s}\n",
                  rec.id, rec.e, rec.bits, rec.words, rec.np, rec.npp, rec.npq, rec.pbits,
                  hex_words(rec.n, rsa::kMaxWords).c_str(), hex_words(rec.K, rsa::kMaxWords).c_str(),
                  hex_words(rec.qR, rsa::kMaxWords).c_str(), hex_words(rec.p, rsa::kHalfWords).c_str(),
                  hex_words(rec.q, rsa::kHalfWords).c_str(), hex_words(rec.dp, rsa::kHalfWords).c_str(),
                  hex_words(rec.dq, rsa::kHalfWords).c_str(), hex_words(rec.qinv, rsa::kHalfWords).c_str(),
                  hex_words(rec.r2p, rsa::kHalfWords).c_str(), hex_words(rec.r2q, rsa::kHalfWords).c_str(),
                  rsa::sign_consistent(rec) ? "true" : "false");
    } else if (cmd == "raw") {
      const std::vector<uint8_t> em = unhex(a);
      uint32_t emw[rsa::kMaxWords], s[rsa::kMaxWords];
      if (!rsa::os2ip(em.data(), em.size(), emw, W)) return 2;
      const bool ok = rsa::sign_raw(rec, emw, s);
      std::printf("{\"status\": 0, \"ok\": %s, \"s\": \"%s\"}\n", ok ? "true" : "false", hex_words(s, W).c_str());
    } else if (cmd == "half") {
      const std::vector<uint8_t> em = unhex(a);
      uint32_t emw[rsa::kMaxWords], m1[rsa::kHalfWords], m2[rsa::kHalfWords], one[rsa::kHalfWords] = {1};
      if (!rsa::os2ip(em.data(), em.size(), emw, W)) return 2;
      rsa::half_exp(emw, rec.p, rec.npp, rec.r2p, rec.dp, W / 2, rec.pbits, m1);
      rsa::half_exp(emw, rec.q, rec.npq, rec.r2q, rec.dq, W / 2, rec.pbits, m2);
      rsa::mont_mul(m1, one, rec.p, rec.npp, W / 2, m1);
      rsa::mont_mul(m2, one, rec.q, rec.npq, W / 2, m2);
      std::printf("{\"status\": 0, \"m1\": \"%s\", \"m2\": \"%s\"}\n", hex_words(m1, W / 2).c_str(),
                  hex_words(m2, W / 2).c_str());
    } else if (cmd == "sign") {
      const std::vector<uint8_t> msg = unhex(a), salt = unhex(b);
      if (salt.size() != 32) return 2;
      const uint32_t k = (rec.bits + 7) / 8;
      std::vector<uint8_t> sig(k);
      const bool ok = rsa::sign(rec, msg.empty() ? &none : msg.data(), msg.size(), salt.data(), sig.data());
      std::printf("{\"status\": 0, \"ok\": %s, \"sig\": \"%s\"}\n", ok ? "true" : "false",
                  hex_bytes(sig.data(), k).c_str());
    } else {
      return 2;
    }
  }
  return 0;
}
