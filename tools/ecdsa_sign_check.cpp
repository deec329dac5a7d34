// Host check of corda_amd/csrc/ecdsa_sign_core.hpp (kernel K17's scalar side), built
// with -fsanitize=address,undefined by tests/test_ecdsa_sign_core.py.
//
//   ecdsa_sign_check <vectors> <randoms> <seed>
//
// <vectors>: lines "q bound x h1 k tries" (hex but bound and tries): the nonce core
// under modulus q and try bound `bound`, for the private key x and the SHA-256 digest
// h1, must answer the nonce k after `tries` candidates; k = 0: it must report
// exhaustion. The test writes these lines from the Python model.
// Then the split k' = min(k, n - k) and the signed 4-bit recoding for both group
// orders: |d_j| <= 8, sum d_j 16^j == k', no carry out of digit 63, for k' = 1,
// (n - 1) / 2 and 2^255 - 1, the full carry chains, and <randoms> seeded scalars
// below each n. Prints one JSON line.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../corda_amd/csrc/ecdsa_sign_core.hpp"

using namespace cordahip;

static const uint32_t kNK1[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u,
                                 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
static const uint32_t kNR1[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu,
                                 0xffffffffu, 0xffffffffu, 0u,          0xffffffffu};

static bool hex_le(uint32_t out[8], const char* s) {  // up to 64 hex digits -> little-endian words
  const size_t n = strlen(s);
  if (n == 0 || n > 64) return false;
  memset(out, 0, 32);
  for (size_t i = 0; i < n; i++) {
    const char c = s[n - 1 - i];
    uint32_t v;
    if (c >= '0' && c <= '9') v = (uint32_t)(c - '0');
    else if (c >= 'a' && c <= 'f') v = (uint32_t)(c - 'a' + 10);
    else if (c >= 'A' && c <= 'F') v = (uint32_t)(c - 'A' + 10);
    else return false;
    out[i / 8] |= v << (4 * (i % 8));
  }
  return true;
}
static ecs_w8 be_of(const uint32_t le[8]) {
  ecs_w8 r;
  for (int i = 0; i < 8; i++) r.v[i] = le[7 - i];
  return r;
}
static int cmp(const uint32_t a[8], const uint32_t b[8]) {
  for (int i = 7; i >= 0; i--)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
static void sub(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - br;
    r[i] = (uint32_t)d;
    br = (d >> 63) & 1u;
  }
}

struct Stats {
  uint64_t scalars = 0, nonces = 0, retried = 0, exhausted = 0;
  uint32_t max_tries = 0;
  int max_abs = 0, most_negative = 0, most_positive = 0;
  bool ok = true;
};
static Stats st;

static void fail(const char* what) {
  if (st.ok) fprintf(stderr, "ecdsa_sign_check: %s\n", what);
  st.ok = false;
}

// the digits of enc rebuilt into a value, from the top: v = 16 v + d_j (never negative
// on the way: the highest non-zero digit of a positive value is positive)
static bool rebuild(uint32_t v[8], const uint32_t enc[8]) {
  memset(v, 0, 32);
  for (int j = 63; j >= 0; j--) {
    if (v[7] >> 28) return false;
    for (int i = 7; i > 0; i--) v[i] = (v[i] << 4) | (v[i - 1] >> 28);
    v[0] <<= 4;
    const int d = ecs_digit(enc, j);
    if (d < -7 || d > 8) return false;
    if (d > st.most_positive) st.most_positive = d;
    if (-d > st.most_negative) st.most_negative = -d;
    const int ad = d < 0 ? -d : d;
    if (ad > st.max_abs) st.max_abs = ad;
    int64_t c = d;
    for (int i = 0; i < 8 && c; i++) {
      const int64_t s = (int64_t)v[i] + c;
      v[i] = (uint32_t)s;
      c = s >> 32;
    }
    if (c) return false;
  }
  return true;
}

// kp < 2^255: digits, sum, carry
static void check_recode(const uint32_t kp[8]) {
  st.scalars++;
  uint32_t enc[8], v[8];
  if (ecs_recode(enc, kp) != 0) return fail("carry out of digit 63");
  if (!rebuild(v, enc)) return fail("digit out of range or negative partial sum");
  if (cmp(v, kp) != 0) return fail("sum of digits differs from the scalar");
  int8_t ref[64];  // the Ed25519 signer's recoding is the same function
  if (comb_recode(ref, kp) != 0) return fail("comb_recode carries out");
  for (int j = 0; j < 64; j++)
    if (ref[j] != ecs_digit(enc, j)) return fail("digits differ from comb_recode's");
}

// 0 < k < n: the split, then the recoding of k'
static void check_scalar(const uint32_t k[8], const uint32_t n[8]) {
  uint32_t kp[8], t[8], u[8];
  const uint32_t flip = ecs_split_min(kp, k, n);
  sub(t, n, k);
  if (flip > 1) return fail("flip is not 0 / 1");
  if (cmp(kp, flip ? t : k) != 0) return fail("k' is neither k nor n - k as flagged");
  sub(u, n, kp);
  if (cmp(kp, u) >= 0) return fail("k' is not the smaller of k and n - k");  // n odd: never equal
  if (kp[7] >> 31) return fail("k' >= 2^255");
  check_recode(kp);
}

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static void check_order(const uint32_t n[8], uint64_t randoms) {
  uint32_t k[8], one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  check_scalar(one, n);                      // k' = 1
  sub(k, n, one);
  check_scalar(k, n);                        // n - 1 -> k' = 1, flipped
  for (int i = 0; i < 8; i++) k[i] = (n[i] >> 1) | (i < 7 ? n[i + 1] << 31 : 0u);
  check_scalar(k, n);                        // (n - 1) / 2: the largest k'
  uint32_t k2[8];
  sub(k2, n, k);
  check_scalar(k2, n);                       // (n + 1) / 2: flips to (n - 1) / 2
  for (int i = 0; i < 8; i++) k[i] = i < 7 ? 0xffffffffu : 0x7fffffffu;
  check_recode(k);                           // 2^255 - 1: the longest carry chain
  // full carry chains: nibbles 0..62 all c under every top nibble 0..7
  for (uint32_t c : {7u, 8u, 9u, 0xfu})
    for (uint32_t top = 0; top < 8; top++) {
      for (int i = 0; i < 8; i++) k[i] = c * 0x11111111u;
      k[7] = (k[7] & 0x0fffffffu) | (top << 28);
      check_recode(k);
    }
  for (uint64_t r = 0; r < randoms;) {
    for (int i = 0; i < 4; i++) {
      const uint64_t x = rng();
      k[2 * i] = (uint32_t)x;
      k[2 * i + 1] = (uint32_t)(x >> 32);
    }
    uint32_t nz = 0;
    for (int i = 0; i < 8; i++) nz |= k[i];
    if (!nz || cmp(k, n) >= 0) continue;
    check_scalar(k, n);
    r++;
  }
}

static void check_vectors(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return fail("cannot open the vectors file");
  char q[80], x[80], h[80], kx[80];
  unsigned bound, tries;
  while (fscanf(f, "%79s %u %79s %79s %79s %u", q, &bound, x, h, kx, &tries) == 6) {
    uint32_t ql[8], xl[8], hl[8], kl[8], hr[8], k[8];
    if (!hex_le(ql, q) || !hex_le(xl, x) || !hex_le(hl, h) || !hex_le(kl, kx)) {
      fail("bad hex in the vectors file");
      break;
    }
    ecs_reduce_once(hr, hl, ql);
    ecs_drbg g;
    ecs_drbg_init(g, be_of(xl), be_of(hr));
    const bool got = ecs_next_nonce(g, k, ql, bound);
    uint32_t nz = 0;
    for (int i = 0; i < 8; i++) nz |= kl[i];
    st.nonces++;
    if (!nz) {  // the model ran out of candidates
      st.exhausted++;
      if (got) fail("a nonce where the model reports exhaustion");
      if (g.tries != bound) fail("exhaustion before the bound");
      continue;
    }
    if (!got) {
      fail("exhaustion where the model has a nonce");
      continue;
    }
    if (cmp(k, kl) != 0) fail("nonce differs from the model's");
    if (g.tries != tries) fail("number of candidates differs from the model's");
    if (g.tries > 1) st.retried++;
    if (g.tries > st.max_tries) st.max_tries = g.tries;
  }
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: ecdsa_sign_check <vectors> <randoms> <seed>\n");
    return 2;
  }
  const uint64_t randoms = strtoull(argv[2], nullptr, 10);
  rng_state = strtoull(argv[3], nullptr, 10);
  check_vectors(argv[1]);
  check_order(kNK1, randoms);
  check_order(kNR1, randoms);
  printf("{\"ok\": %s, \"nonces\": %" PRIu64 ", \"retried\": %" PRIu64 ", \"exhausted\": %" PRIu64
         ", \"max_tries\": %u, \"scalars\": %" PRIu64 ", \"max_abs\": %d, \"most_positive\": %d, \"most_negative\": %d}\n",
         st.ok ? "true" : "false", st.nonces, st.retried, st.exhausted, st.max_tries, st.scalars, st.max_abs,
         st.most_positive, st.most_negative);
  return st.ok ? 0 : 1;
}
