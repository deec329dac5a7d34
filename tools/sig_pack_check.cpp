// K23's packer on the CPU (tests/test_sig_pack_check.py builds this with g++
// -fsanitize=address,undefined): the count, scan and pack passes of sig_pack.hip replayed
// tile by tile -- in order and shuffled -- with the functions of sig_pack.hpp, the wave
// ballots emulated, into buffers of exactly the sizes the layout names, and compared row
// for row with a plain sequential run of the host packer (pack_rows.hpp classify /
// pack_ed_row / pack_ec_row / rsa_lane_pre / pack_rsa_row) over the same batch. The lane
// rule is also checked against a restatement of it written out here (ref_rule: the host
// packer's decisions as they stood before the rule moved to sig_pack.hpp).
// Prints one JSON line; exit status 0 when nothing differed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../corda_amd/csrc/pack_rows.hpp"
#include "../corda_amd/csrc/sig_pack.hpp"

using namespace cordahip;
using namespace cordahip::sigpack;

namespace {

std::mt19937_64 rng;
uint32_t rnd(uint32_t m) { return (uint32_t)(rng() % m); }
std::vector<uint8_t> rbytes(size_t n) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = (uint8_t)rng();
  return v;
}

struct Stats {
  uint64_t cases = 0, shuffled = 0, lanes = 0, failures = 0, cls[kClasses] = {}, empty_class_cases[kClasses] = {},
           single_class_cases[kClasses] = {}, key_len_seen[7] = {}, ec_sig_len_seen[5] = {}, ec_long_wf = 0,
           ec_long_garbage = 0, rsa_class_rows[3] = {}, rsa_even_n = 0, rsa_e_even = 0, rsa_e_lt3 = 0, rsa_e_big = 0,
           rsa_1016 = 0, rsa_4104 = 0, rsa_trunc = 0, rsa_sig_long = 0, rsa_off = 0, bad_first = 0, bad_mid = 0,
           bad_last = 0, bad_reversed = 0, bad_overrun = 0, bad_msg_row = 0, key_align[16] = {}, sig_align[16] = {},
           over_cap = 0, overlap_cases = 0, direct_status[6] = {}, multi_tile = 0, n0 = 0, rule_checks = 0;
} st;

void fail(const char* what, uint64_t a = 0, uint64_t b = 0) {
  if (st.failures++ < 20) fprintf(stderr, "FAIL %s (%llu, %llu) case %llu\n", what, (unsigned long long)a,
                                  (unsigned long long)b, (unsigned long long)st.cases);
}

// ---- lanes -----------------------------------------------------------------------------
struct LaneSrc {
  uint8_t scheme;
  std::vector<uint8_t> key, sig;
};

void der_len(std::vector<uint8_t>& o, size_t n) {
  if (n < 128) o.push_back((uint8_t)n);
  else if (n < 256) o.push_back(0x81), o.push_back((uint8_t)n);
  else o.push_back(0x82), o.push_back((uint8_t)(n >> 8)), o.push_back((uint8_t)n);
}
void der_int(std::vector<uint8_t>& o, std::vector<uint8_t> mag) {
  if (mag[0] >= 0x80) mag.insert(mag.begin(), 0);
  o.push_back(0x02);
  der_len(o, mag.size());
  o.insert(o.end(), mag.begin(), mag.end());
}
std::vector<uint8_t> rsa_key(std::vector<uint8_t> nmag, std::vector<uint8_t> emag) {
  std::vector<uint8_t> body, o;
  der_int(body, nmag);
  der_int(body, emag);
  o.push_back(0x30);
  der_len(o, body.size());
  o.insert(o.end(), body.begin(), body.end());
  return o;
}
std::vector<uint8_t> modulus(uint32_t bits, bool odd = true) {
  std::vector<uint8_t> m = rbytes((bits + 7) / 8);
  const uint32_t top = (bits - 1) % 8;
  m[0] = (uint8_t)((m[0] & ((1u << (top + 1)) - 1)) | (1u << top));
  m.back() = odd ? (m.back() | 1) : (m.back() & 0xfe);
  return m;
}
std::vector<uint8_t> long_der(uint32_t total) {  // a well-formed ECDSA signature of 73 or 80 bytes
  const uint32_t rl = 33, sl = total - 2 - 2 - rl - 2;
  std::vector<uint8_t> o = {0x30, (uint8_t)(total - 2), 0x02, (uint8_t)rl};
  std::vector<uint8_t> r = rbytes(rl), s = rbytes(sl);
  r[0] = 0, r[1] |= 0x80, s[0] = 0x01;
  o.insert(o.end(), r.begin(), r.end());
  o.push_back(0x02), o.push_back((uint8_t)sl);
  o.insert(o.end(), s.begin(), s.end());
  return o;
}

static const uint32_t kKeyLens[7] = {0, 31, 32, 33, 64, 65, 66};
static const uint32_t kEcSigLens[5] = {0, 8, 72, 73, 80};

LaneSrc gen_lane() {
  LaneSrc l;
  const uint32_t k = rnd(100);
  if (k < 30) {  // Ed25519, the key and signature lengths of the rule
    l.scheme = kSchemeEd;
    l.key = rbytes(rnd(5) ? 32 : kKeyLens[rnd(7)]);
    const uint32_t s = rnd(8);
    l.sig = rbytes(s == 0 ? 0 : s == 1 ? 63 : s == 2 ? 65 : 64);
  } else if (k < 60) {  // ECDSA
    l.scheme = rnd(2) ? kSchemeK1 : kSchemeR1;
    l.key = rbytes(rnd(6) ? (rnd(2) ? 33 : 65) : kKeyLens[rnd(7)]);
    const uint32_t s = rnd(10);
    if (s < 5) {
      const uint32_t len = kEcSigLens[s];
      if (len > 72 && rnd(2)) l.sig = long_der(len);
      else l.sig = rbytes(len);
    } else {
      l.sig = rbytes(60 + rnd(13));
    }
  } else if (k < 90) {  // RSA
    l.scheme = kSchemeRsa;
    const uint32_t v = rnd(16);
    std::vector<uint8_t> e = {1, 0, 1};
    uint32_t bits = v % 4 == 0 ? 1024 : v % 4 == 1 ? 2048 : v % 4 == 2 ? 3072 : 4096;
    bool odd = true, trunc = false;
    if (v == 4) bits = 2049;
    if (v == 5) bits = 3073;
    if (v == 8) odd = false;
    if (v == 9) e = {1, 0, 0};
    if (v == 10) e = {1};
    if (v == 11) e = {1, 0, 0, 0, 1};
    if (v == 12) bits = 1016;
    if (v == 13) bits = 4104;
    if (v == 14) trunc = true;
    l.key = rsa_key(modulus(bits, odd), e);
    if (trunc) l.key.pop_back();
    const uint32_t kb = (bits + 7) / 8, s = rnd(8);
    l.sig = rbytes(s == 0 ? kb + 1 : s == 1 ? 0 : s == 2 ? kb - 1 : kb);
  } else {  // schemes the GPU has no verifier for
    static const uint8_t other[4] = {0, 5, 6, 200};
    l.scheme = other[rnd(4)];
    l.key = rbytes(rnd(70));
    l.sig = rbytes(rnd(80));
  }
  return l;
}

// ---- the rule, restated ------------------------------------------------------------------
// class and direct status of a lane whose ranges are in order (the host packer before K23)
void ref_rule(const LaneSrc& l, uint32_t L, bool dv, bool rsa_on, uint32_t& cls, uint8_t& status) {
  cls = kDirect, status = 0;
  const uint64_t kl = l.key.size(), sl = l.sig.size();
  if (l.scheme == 2 || l.scheme == 3) {
    if (kl != 33 && kl != 65) status = 3;
    else cls = kEc;
    return;
  }
  if (l.scheme == 1 && rsa_on) {
    rsa::PublicKey pk;
    const uint8_t ks = rsa::parse_public_key(l.key.data(), kl, pk);
    if (ks != rsa::kOk) status = ks;
    else if (dv && (sl == 0 || L == 0)) status = 5;
    else if (sl > (pk.bits + 7) / 8) status = 1;
    else cls = kRsa0 + (pk.words / 32 - 2);
    return;
  }
  if (l.scheme != 4) status = 4;
  else if (kl != 32) status = 3;
  else cls = kEd;
}

// ---- a case --------------------------------------------------------------------------------
struct MV {  // pack_rows.hpp's message view of a batch whose messages are indexed rows
  const uint64_t* tx_of;
  const uint64_t* off = nullptr;
  uint32_t L;
  uint64_t len(uint64_t) const { return L; }
  const uint8_t* ptr(uint64_t) const { return nullptr; }
};

enum BadKind { kNoBad = 0, kRevKey, kOverKey, kRevSig, kOverSig, kBadMsgRow, kOverlap };

template <class T>
std::unique_ptr<T[]> exact(size_t n) {  // exactly n elements: the sanitizer sees the first byte past them
  return std::unique_ptr<T[]>(new T[n ? n : 1]);
}

void run_case(uint64_t n, int only_cls, int no_cls, bool shuffle, uint32_t L, bool dv, bool rsa_on, uint32_t pad,
              BadKind bad, int bad_where) {
  st.cases++;
  st.shuffled += shuffle;
  if (n == 0) st.n0++;
  // lanes by pattern
  std::vector<LaneSrc> lanes(n);
  for (uint64_t i = 0; i < n; i++) {
    for (int tries = 0;; tries++) {
      lanes[i] = gen_lane();
      uint32_t c;
      uint8_t s;
      ref_rule(lanes[i], L, dv, rsa_on, c, s);
      if (only_cls >= 0 && only_cls != (int)kBad && (int)c != only_cls) continue;
      if (no_cls >= 0 && (int)c == no_cls) continue;
      break;
    }
  }
  // overlapping key ranges: every even lane an RSA-2048 lane over the same key bytes, every odd
  // lane reversed -- more lanes of the class than key_bytes can hold keys for
  if (bad == kOverlap) {
    const std::vector<uint8_t> k = rsa_key(modulus(2048), {1, 0, 1});
    for (uint64_t i = 0; i < n; i++) lanes[i] = LaneSrc{kSchemeRsa, i == 0 ? k : std::vector<uint8_t>(), rbytes(256)};
    st.overlap_cases++;
  }
  // CSR with `pad` bytes in front, buffers of exactly their declared sizes
  std::vector<uint64_t> koff(n + 1), soff(n + 1), txof(n);
  std::vector<uint32_t> mrow(n);
  uint64_t kb = pad, sb = (pad * 7 + 3) % 16;
  for (uint64_t i = 0; i < n; i++) {
    koff[i] = kb, soff[i] = sb;
    kb += lanes[i].key.size(), sb += lanes[i].sig.size();
  }
  koff[n] = kb, soff[n] = sb;
  if (bad == kOverlap)
    for (uint64_t i = 0; i <= n; i++) koff[i] = i % 2 == 0 ? pad : kb;
  auto key = exact<uint8_t>(kb);
  auto sig = exact<uint8_t>(sb);
  std::vector<uint8_t> scheme(n);
  const uint64_t msg_rows = n ? std::max<uint64_t>(1, n / 3) : 0;
  for (uint64_t i = 0; i < n; i++) {
    if (!lanes[i].key.empty()) memcpy(key.get() + koff[i], lanes[i].key.data(), lanes[i].key.size());
    if (!lanes[i].sig.empty()) memcpy(sig.get() + soff[i], lanes[i].sig.data(), lanes[i].sig.size());
    scheme[i] = lanes[i].scheme;
    mrow[i] = rnd((uint32_t)msg_rows);
  }
  // bad ranges: one lane (its neighbours follow from the same offsets on both sides)
  const uint64_t bp = bad_where == 0 ? 0 : bad_where == 1 ? n / 2 : n ? n - 1 : 0;
  if (only_cls == (int)kBad) {
    for (uint64_t i = 0; i < n; i++) mrow[i] = (uint32_t)msg_rows + rnd(5);
  } else if (bad != kNoBad && bad != kOverlap && n) {
    if (bad == kRevKey) koff[bp] = koff[bp + 1] + 5;
    if (bad == kOverKey) koff[bp + 1] = kb + 7;
    if (bad == kRevSig) soff[bp] = soff[bp + 1] + 3;
    if (bad == kOverSig) soff[bp + 1] = sb + 1;
    if (bad == kBadMsgRow) mrow[bp] = (uint32_t)msg_rows;
    (bad_where == 0 ? st.bad_first : bad_where == 1 ? st.bad_mid : st.bad_last)++;
    if (bad == kRevKey || bad == kRevSig) st.bad_reversed++;
    if (bad == kOverKey || bad == kOverSig) st.bad_overrun++;
    if (bad == kBadMsgRow) st.bad_msg_row++;
  }
  for (uint64_t i = 0; i < n; i++) txof[i] = mrow[i];

  // ---- the sequential reference: the host packer, lane by lane ----
  std::vector<uint8_t> want_status(n, 0xEE);
  cordahip_sig_batch b{};
  b.n = n, b.scheme = scheme.data(), b.key = key.get(), b.key_off = koff.data(), b.sig = sig.get();
  b.sig_off = soff.data(), b.status = want_status.data(), b.key_bytes = kb, b.sig_bytes = sb;
  b.flags = (dv ? 0u : CORDAHIP_FLAG_IS_VALID) | (rsa_on ? CORDAHIP_FLAG_RSA_ON_DEVICE : 0u);
  MV mv{txof.data(), nullptr, L};
  struct Rows {
    std::vector<uint8_t> ed_key, ed_sig, ed_pre, ec_scheme, ec_key, ec_kl, ec_sig, ec_sl, ec_pre;
    std::vector<uint32_t> ed_lane, ed_msg, ec_lane, ec_msg, ec_sub, rsa_lane[3], rsa_msg[3], rsa_mod[3], rsa_exp[3];
    std::vector<uint8_t> rsa_sig[3];
    std::vector<uint16_t> rsa_sl[3];
  } W;
  uint64_t want_cnt[kClasses] = {}, cap[3] = {};
  for (uint32_t c = 0; c < 3 && rsa_on; c++) cap[c] = rsa_cap_rows(kRsa0 + c, n, kb);
  for (uint64_t i = 0; i < n; i++) {
    uint64_t mlen = 0;
    uint32_t rc = 0;
    uint16_t c = rt::classify(&b, mv, i, mlen, &rc);
    if (c != rt::kBadCsr && mrow[i] >= msg_rows) c = rt::kBadCsr, want_status[i] = 0xEE;
    if (c == rt::kBadCsr) {
      want_status[i] = kStBadRange;
      want_cnt[kBad]++;
      continue;
    }
    {  // the restated rule agrees
      LaneSrc l{scheme[i], std::vector<uint8_t>(key.get() + koff[i], key.get() + koff[i + 1]),
                std::vector<uint8_t>(sig.get() + soff[i], sig.get() + soff[i + 1])};
      uint32_t cls;
      uint8_t s;
      ref_rule(l, L, dv, rsa_on, cls, s);
      st.rule_checks++;
      const uint16_t hc = cls == kDirect ? rt::kDirect : cls == kEd ? rt::kEdBase : cls == kEc ? rt::kEc : rt::kRsa;
      if (hc != c || (cls == kDirect && s != want_status[i]) || (cls >= kRsa0 && cls - kRsa0 != rc))
        fail("rule", i, c);
    }
    if (c == rt::kDirect) {
      want_cnt[kDirect]++;
      if (want_status[i] < 6) st.direct_status[want_status[i]]++;
      if (scheme[i] == 1 && !rsa_on) st.rsa_off++;
    } else if (c == rt::kEdBase) {
      const uint64_t r = want_cnt[kEd]++;
      W.ed_key.resize(32 * (r + 1)), W.ed_sig.resize(64 * (r + 1)), W.ed_pre.resize(r + 1);
      rt::pack_ed_row(&b, mv, dv, i, L, &W.ed_key[32 * r], &W.ed_sig[64 * r], (uint8_t*)nullptr, &W.ed_pre[r]);
      W.ed_lane.push_back((uint32_t)i), W.ed_msg.push_back(mrow[i]);
    } else if (c == rt::kEc) {
      const uint64_t r = want_cnt[kEc]++;
      W.ec_scheme.resize(r + 1), W.ec_key.resize(65 * (r + 1)), W.ec_kl.resize(r + 1), W.ec_sig.resize(72 * (r + 1));
      W.ec_sl.resize(r + 1), W.ec_pre.resize(r + 1), W.ec_msg.resize(r + 1);
      std::vector<uint64_t> hmo(r + 1);
      uint64_t mo = 0;
      rt::pack_ec_row(&b, mv, dv, i, r, W.ec_scheme.data(), W.ec_key.data(), W.ec_kl.data(), W.ec_sig.data(),
                      W.ec_sl.data(), (uint8_t*)nullptr, hmo.data(), W.ec_pre.data(), mo, W.ec_msg.data());
      W.ec_lane.push_back((uint32_t)i);
      W.ec_sub.push_back((scheme[i] == 2 ? 0u : 2u) + (koff[i + 1] - koff[i] == 33 ? 1u : 0u));
      const uint64_t sl = soff[i + 1] - soff[i];
      for (int q = 0; q < 5; q++)
        if (sl == kEcSigLens[q]) st.ec_sig_len_seen[q]++;
      if (sl > 72) (W.ec_pre[r] == kStBadSig ? st.ec_long_wf : st.ec_long_garbage)++;
    } else if (want_cnt[kRsa0 + rc] >= cap[rc]) {  // a lane its class has no row for
      want_status[i] = kStBadRange;
      want_cnt[kBad]++;
      st.over_cap++;
      if (bad != kOverlap) fail("over the bound with disjoint ranges", i);
    } else {
      rsa::PublicKey pk;
      if (rt::rsa_lane_pre(&b, mv, dv, i, pk) != rt::kRsaToDevice) fail("rsa_lane_pre", i);
      const uint32_t Wd = pk.words;
      const uint64_t r = want_cnt[kRsa0 + rc]++;
      W.rsa_mod[rc].resize(Wd * (r + 1)), W.rsa_exp[rc].resize(r + 1), W.rsa_sig[rc].resize(4 * Wd * (r + 1));
      W.rsa_sl[rc].resize(r + 1);
      rt::pack_rsa_row(&b, i, pk, Wd, r, W.rsa_mod[rc].data(), W.rsa_exp[rc].data(), W.rsa_sig[rc].data(),
                       W.rsa_sl[rc].data());
      W.rsa_lane[rc].push_back((uint32_t)i), W.rsa_msg[rc].push_back(mrow[i]);
      st.rsa_class_rows[rc]++;
    }
    {
      const uint64_t kl = koff[i + 1] - koff[i];
      for (int q = 0; q < 7; q++)
        if (kl == kKeyLens[q] && (scheme[i] == 4 || scheme[i] == 2 || scheme[i] == 3)) st.key_len_seen[q]++;
      if (c != rt::kDirect) {
        st.key_align[(uintptr_t)(key.get() + koff[i]) & 15]++;
        st.sig_align[(uintptr_t)(sig.get() + soff[i]) & 15]++;
      }
    }
  }
  // corners of the RSA rule met (from the sources: an injected bad range may have moved a lane's bytes)
  if (rsa_on && bad == kNoBad && only_cls != (int)kBad)
    for (uint64_t i = 0; i < n; i++) {
      if (scheme[i] != 1) continue;
      rsa::KeyView kv;
      const uint8_t ks = rsa::parse_public_key_view(lanes[i].key.data(), lanes[i].key.size(), kv);
      if (ks == rsa::kOk && lanes[i].sig.size() == (kv.bits + 7) / 8 + 1) st.rsa_sig_long++;
    }
  for (uint32_t c = 0; c < kClasses; c++) {
    st.cls[c] += want_cnt[c];
    if (n && !want_cnt[c]) st.empty_class_cases[c]++;
    if (n && want_cnt[c] == n) st.single_class_cases[c]++;
  }
  st.lanes += n;
  if (n == 0) return;  // nothing is launched for an empty batch

  // ---- the replay: buffers of exactly the sizes the layout names ----
  const uint64_t nt = tiles(n);
  if (nt > 1) st.multi_tile++;
  In in{scheme.data(), key.get(), koff.data(), kb, sig.get(), soff.data(), sb, mrow.data(), msg_rows, L, n,
        dv ? 1u : 0u, rsa_on ? 1u : 0u};
  auto hdr = exact<uint32_t>(kHdrWords + n);
  auto code = exact<uint8_t>(n);
  auto btot = exact<uint32_t>(kCounts * nt);
  auto boff = exact<uint32_t>(kCounts * nt);
  auto status = exact<uint8_t>(n);
  memset(status.get(), 0xEE, n);
  auto ed_key = exact<uint32_t>(8 * n), ed_sig = exact<uint32_t>(16 * n), ed_lane = exact<uint32_t>(n),
       ed_msg = exact<uint32_t>(n), ec_lane = exact<uint32_t>(n), ec_msg = exact<uint32_t>(n),
       ec_perm = exact<uint32_t>(n);
  auto ed_pre = exact<uint8_t>(n), ec_scheme = exact<uint8_t>(n), ec_key = exact<uint8_t>(65 * n),
       ec_kl = exact<uint8_t>(n), ec_sig = exact<uint8_t>(72 * n), ec_sl = exact<uint8_t>(n), ec_pre = exact<uint8_t>(n);
  std::unique_ptr<uint32_t[]> rmod[3], rexp[3], rsig[3], rlane[3], rmsg[3];
  std::unique_ptr<uint16_t[]> rsl[3];
  std::unique_ptr<uint8_t[]> rpre[3];
  Out out{};
  out.hdr = hdr.get(), out.code = code.get(), out.btot = btot.get(), out.boff = boff.get(), out.status = status.get();
  out.ed_key = ed_key.get(), out.ed_sig = ed_sig.get(), out.ed_pre = ed_pre.get(), out.ed_lane = ed_lane.get();
  out.ed_msg = ed_msg.get(), out.ec_scheme = ec_scheme.get(), out.ec_key = ec_key.get(), out.ec_key_len = ec_kl.get();
  out.ec_sig = ec_sig.get(), out.ec_sig_len = ec_sl.get(), out.ec_pre = ec_pre.get(), out.ec_lane = ec_lane.get();
  out.ec_msg = ec_msg.get(), out.ec_perm = ec_perm.get();
  for (uint32_t c = 0; c < 3 && rsa_on; c++) {
    const uint64_t cap = out.rsa_cap[c] = rsa_cap_rows(kRsa0 + c, n, kb), Wd = rsa_words(kRsa0 + c);
    rmod[c] = exact<uint32_t>(Wd * cap), rexp[c] = exact<uint32_t>(cap), rsig[c] = exact<uint32_t>(Wd * cap);
    rlane[c] = exact<uint32_t>(cap), rmsg[c] = exact<uint32_t>(cap), rsl[c] = exact<uint16_t>(cap);
    rpre[c] = exact<uint8_t>(cap);
    out.rsa_mod[c] = rmod[c].get(), out.rsa_exp[c] = rexp[c].get(), out.rsa_sig[c] = rsig[c].get();
    out.rsa_lane[c] = rlane[c].get(), out.rsa_msg[c] = rmsg[c].get(), out.rsa_sig_len[c] = rsl[c].get();
    out.rsa_pre[c] = rpre[c].get();
  }
  std::vector<uint64_t> order(nt);
  for (uint64_t t = 0; t < nt; t++) order[t] = t;
  // count
  if (shuffle) std::shuffle(order.begin(), order.end(), rng);
  for (uint64_t tile : order) {
    uint32_t tot[kCounts] = {};
    for (int it = 0; it < kIter; it++)
      for (uint32_t t = 0; t < 256; t++) {
        const uint64_t i = tile_lane(tile, it, t);
        if (i >= n) continue;
        code[i] = count_lane(in, i);
        tot[code_count(code[i])]++;
      }
    for (uint32_t k = 0; k < kCounts; k++) btot[k * nt + tile] = tot[k];
  }
  // scan
  for (uint32_t k = 0; k < kCounts; k++) {
    uint32_t acc = 0;
    for (uint64_t t = 0; t < nt; t++) boff[k * nt + t] = acc, acc += btot[k * nt + t];
    hdr[kHdrRaw + k] = acc;
  }
  // pack: segment totals, their prefix, ranks within the wave's ballot
  if (shuffle) std::shuffle(order.begin(), order.end(), rng);
  bool header_done = false;
  for (uint64_t tile : order) {
    if (tile == 0) derive_header(hdr.get(), out.rsa_cap), header_done = true;
    uint32_t seg[kCounts][kSegs + 1] = {};
    for (int it = 0; it < kIter; it++)
      for (uint32_t t = 0; t < 256; t++) {
        const uint64_t i = tile_lane(tile, it, t);
        if (i < n) seg[code_count(code[i])][seg_of(it, t)]++;
      }
    for (uint32_t k = 0; k < kCounts; k++) {
      uint32_t acc = 0;
      for (int s = 0; s <= kSegs; s++) {
        const uint32_t v = s < kSegs ? seg[k][s] : 0;
        seg[k][s] = acc, acc += v;
      }
    }
    for (int it = 0; it < kIter; it++)
      for (uint32_t wv = 0; wv < 4; wv++) {
        uint32_t below[kCounts] = {};  // the ballots' bits below the lane, lane by lane
        for (uint32_t ln = 0; ln < 64; ln++) {
          const uint32_t t = wv * 64 + ln;
          const uint64_t i = tile_lane(tile, it, t);
          if (i >= n) continue;
          const uint32_t ci = code_count(code[i]);
          const int s = seg_of(it, t);
          uint64_t row = (uint64_t)boff[ci * nt + tile] + seg[ci][s] + below[ci], perm_pos = 0;
          if (class_of_count(ci) == kEc) {
            perm_pos = row;
            for (uint32_t k = kCntEc0; k < ci; k++) perm_pos += hdr[kHdrRaw + k];
            row = 0;
            for (uint32_t k = kCntEc0; k < kCntRsa0; k++) row += (uint64_t)boff[k * nt + tile] + seg[k][s] + below[k];
          }
          if (!pack_lane(in, out, i, code[i], row, perm_pos) && want_status[i] != kStBadRange) fail("rsa cap", i, row);
          below[ci]++;
        }
      }
  }
  if (!header_done) fail("header");

  // ---- compare ----
  for (uint32_t c = 0; c < kClasses; c++)
    if (hdr[kHdrClass + c] != want_cnt[c]) fail("count", c, hdr[kHdrClass + c]);
  for (uint64_t i = 0; i < n; i++) {
    if (hdr[kHdrWords + i] != i) fail("iota", i);
    if (status[i] != want_status[i]) fail("status", i, status[i]);
  }
  for (uint32_t k = 0; k < 16; k++)
    if (hdr[kHdrEd + k] != (k == 1 ? want_cnt[kEd] : 0)) fail("ed header", k);
  {
    uint64_t sub[4] = {};
    for (uint32_t s : W.ec_sub) sub[s]++;
    for (uint32_t k = 0; k < 14; k++)
      if (hdr[kHdrEc + k] != (k < 4 ? sub[k] : 0)) fail("ec counters", k);
    std::vector<uint32_t> want_perm;
    for (uint32_t s = 0; s < 4; s++)
      for (uint64_t r = 0; r < W.ec_sub.size(); r++)
        if (W.ec_sub[r] == s) want_perm.push_back((uint32_t)r);
    if (want_cnt[kEc] && memcmp(want_perm.data(), ec_perm.get(), 4 * want_cnt[kEc])) fail("ec perm");
  }
  const auto same = [&](const char* what, const void* a, const void* bb, size_t bytes) {
    if (bytes && memcmp(a, bb, bytes)) fail(what);
  };
  const uint64_t ne = want_cnt[kEd], nc = want_cnt[kEc];
  same("ed key", W.ed_key.data(), ed_key.get(), 32 * ne), same("ed sig", W.ed_sig.data(), ed_sig.get(), 64 * ne);
  same("ed pre", W.ed_pre.data(), ed_pre.get(), ne), same("ed lane", W.ed_lane.data(), ed_lane.get(), 4 * ne);
  same("ed msg", W.ed_msg.data(), ed_msg.get(), 4 * ne);
  same("ec scheme", W.ec_scheme.data(), ec_scheme.get(), nc), same("ec key", W.ec_key.data(), ec_key.get(), 65 * nc);
  same("ec key_len", W.ec_kl.data(), ec_kl.get(), nc), same("ec sig", W.ec_sig.data(), ec_sig.get(), 72 * nc);
  same("ec sig_len", W.ec_sl.data(), ec_sl.get(), nc), same("ec pre", W.ec_pre.data(), ec_pre.get(), nc);
  same("ec lane", W.ec_lane.data(), ec_lane.get(), 4 * nc), same("ec msg", W.ec_msg.data(), ec_msg.get(), 4 * nc);
  for (uint32_t c = 0; c < 3 && rsa_on; c++) {
    const uint64_t r = want_cnt[kRsa0 + c], Wd = rsa_words(kRsa0 + c);
    if (r > out.rsa_cap[c]) fail("rsa cap bound", c, r);
    same("rsa mod", W.rsa_mod[c].data(), rmod[c].get(), 4 * Wd * r);
    same("rsa exp", W.rsa_exp[c].data(), rexp[c].get(), 4 * r);
    same("rsa sig", W.rsa_sig[c].data(), rsig[c].get(), 4 * Wd * r);
    same("rsa sig_len", W.rsa_sl[c].data(), rsl[c].get(), 2 * r);
    same("rsa lane", W.rsa_lane[c].data(), rlane[c].get(), 4 * r);
    same("rsa msg", W.rsa_msg[c].data(), rmsg[c].get(), 4 * r);
    for (uint64_t q = 0; q < r; q++)
      if (rpre[c][q] != kStOk) fail("rsa pre", c, q);
  }
}

// the RSA corners as the generator makes them, counted once per kind (the rule's answers)
void rsa_corners() {
  const auto pre = [](const std::vector<uint8_t>& k, uint64_t sl) {
    rsa::KeyView kv;
    return rsa_pre(k.data(), k.size(), sl, 32, true, kv);
  };
  if (pre(rsa_key(modulus(2048, false), {1, 0, 1}), 256) == kStUnsupported) st.rsa_even_n++;
  if (pre(rsa_key(modulus(2048), {1, 0, 0}), 256) == kStUnsupported) st.rsa_e_even++;
  if (pre(rsa_key(modulus(2048), {1}), 256) == kStUnsupported) st.rsa_e_lt3++;
  if (pre(rsa_key(modulus(2048), {1, 0, 0, 0, 1}), 256) == kStUnsupported) st.rsa_e_big++;
  if (pre(rsa_key(modulus(1016), {1, 0, 1}), 127) == kStUnsupported) st.rsa_1016++;
  if (pre(rsa_key(modulus(4104), {1, 0, 1}), 513) == kStUnsupported) st.rsa_4104++;
  std::vector<uint8_t> t = rsa_key(modulus(2048), {1, 0, 1});
  t.pop_back();
  if (pre(t, 256) == kStBadKey) st.rsa_trunc++;
  if (pre(rsa_key(modulus(2048), {1, 0, 1}), 257) != kStBadSig) fail("sig longer than the modulus");
  if (pre(rsa_key(modulus(2041), {1, 0, 1}), 256) != kRsaToDevice) fail("sig as long as the modulus");
}

}  // namespace

int main(int argc, char** argv) {
  rng.seed(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  rsa_corners();
  static const uint64_t ns[9] = {0, 1, 63, 64, 65, 255, 256, 257, 2 * kTile + 1};
  uint32_t v = 0;
  for (uint64_t n : ns)
    for (int pat = 0; pat < 1 + 2 * (int)kClasses; pat++)
      for (int sh = 0; sh < 2; sh++, v++) {
        const int only = pat >= 1 && pat <= (int)kClasses ? pat - 1 : -1;
        const int none = pat > (int)kClasses ? pat - 1 - (int)kClasses : -1;
        // the flags and the buffers' misalignment cycle with the case; RSA-class patterns need the flag
        const bool rsa_on = (only >= (int)kRsa0 && only <= (int)kRsa2) || (v % 4 != 3);
        const bool dv = only >= (int)kRsa0 && only <= (int)kRsa2 ? v % 2 == 0 : v % 3 != 0;
        const uint32_t L = (only == (int)kDirect || only < 0) && v % 7 == 0 ? 0 : 32;
        run_case(n, only, none, sh != 0, L, dv, rsa_on, v % 16, kNoBad, 0);
      }
  for (uint64_t n : {(uint64_t)65, (uint64_t)257, (uint64_t)(2 * kTile + 1)})
    for (int where = 0; where < 3; where++)
      for (int kind = kRevKey; kind <= kBadMsgRow; kind++, v++)
        run_case(n, -1, -1, v % 2 != 0, 32, v % 3 != 0, true, v % 16, (BadKind)kind, where);
  // overlapping key ranges: a class with more lanes than rows, within one tile and over several
  for (uint64_t n : {(uint64_t)9, (uint64_t)300, (uint64_t)(2 * kTile + 1)})
    for (int sh = 0; sh < 2; sh++, v++) run_case(n, -1, -1, sh != 0, 32, true, true, v % 16, kOverlap, 0);
  // every source misalignment with a batch large enough to hold every class
  for (uint32_t pad = 0; pad < 16; pad++) run_case(300, -1, -1, pad % 2 != 0, 32, true, true, pad, kNoBad, 0);

  std::string j = "{";
  const auto num = [&](const char* k, uint64_t x) { j += std::string("\"") + k + "\": " + std::to_string(x) + ", "; };
  const auto arr = [&](const char* k, const uint64_t* a, int m) {
    j += std::string("\"") + k + "\": [";
    for (int q = 0; q < m; q++) j += std::to_string(a[q]) + (q + 1 < m ? ", " : "");
    j += "], ";
  };
  num("cases", st.cases), num("shuffled", st.shuffled), num("lanes", st.lanes), num("failures", st.failures);
  num("n0", st.n0), num("multi_tile", st.multi_tile), num("rule_checks", st.rule_checks);
  arr("class_lanes", st.cls, kClasses), arr("empty_class_cases", st.empty_class_cases, kClasses);
  arr("single_class_cases", st.single_class_cases, kClasses), arr("key_len_seen", st.key_len_seen, 7);
  arr("ec_sig_len_seen", st.ec_sig_len_seen, 5), num("ec_long_wellformed", st.ec_long_wf);
  num("ec_long_garbage", st.ec_long_garbage), arr("rsa_class_rows", st.rsa_class_rows, 3);
  num("rsa_even_n", st.rsa_even_n), num("rsa_e_even", st.rsa_e_even), num("rsa_e_lt3", st.rsa_e_lt3);
  num("rsa_e_big", st.rsa_e_big), num("rsa_1016", st.rsa_1016), num("rsa_4104", st.rsa_4104);
  num("rsa_trunc", st.rsa_trunc), num("rsa_sig_long", st.rsa_sig_long), num("rsa_flag_off_lanes", st.rsa_off);
  num("bad_first", st.bad_first), num("bad_mid", st.bad_mid), num("bad_last", st.bad_last);
  num("bad_reversed", st.bad_reversed), num("bad_overrun", st.bad_overrun), num("bad_msg_row", st.bad_msg_row);
  arr("key_align", st.key_align, 16), arr("sig_align", st.sig_align, 16), arr("direct_status", st.direct_status, 6);
  num("over_cap", st.over_cap), num("overlap_cases", st.overlap_cases);
  j += std::string("\"ok\": ") + (st.failures ? "false" : "true") + "}";
  printf("%s\n", j.c_str());
  return st.failures ? 1 : 0;
}
