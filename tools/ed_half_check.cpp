// Host driver of the Ed25519 prep's vector choice (corda_amd/csrc/ed25519_half.hpp),
// built with ASan + UBSan by tests/test_ed_half_choice.py. Reads Euclid states
// from stdin, one per line as four 64-digit hexadecimal words of 256 bits
// (two's complement): rp rc tp tc; runs half_choose on each, the exact division
// step for the next Euclid vector included, and prints one line per state:
//   <0|1: c0 negative> <|c0| hex> <c1 hex>
// The test recomputes the choice with big integers (tools/proto/half_scalar_windows.py).
// Exit 0 = every line parsed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../corda_amd/csrc/ed25519_half.hpp"

using namespace cordahip;

static bool parse256(const char* s, uint32_t w[8]) {
  if (strlen(s) != 64) return false;
  for (int i = 0; i < 8; i++) {
    uint32_t v = 0;
    for (int k = 0; k < 8; k++) {
      const char c = s[8 * (7 - i) + k];
      int d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else return false;
      v = v << 4 | (uint32_t)d;
    }
    w[i] = v;
  }
  return true;
}

static void print256(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--) printf("%08x", w[i]);
}

int main() {
  char a[4][80];
  long n = 0;
  while (scanf("%79s %79s %79s %79s", a[0], a[1], a[2], a[3]) == 4) {
    uint32_t st[4][8];
    for (int k = 0; k < 4; k++)
      if (!parse256(a[k], st[k])) {
        fprintf(stderr, "line %ld: bad word %d\n", n + 1, k);
        return 2;
      }
    uint32_t c0abs[8], c1[8];
    bool c0neg = false;
    half_choose(c0abs, c0neg, c1, st[0], st[1], st[2], st[3]);
    printf("%d ", c0neg ? 1 : 0);
    print256(c0abs);
    printf(" ");
    print256(c1);
    printf("\n");
    n++;
  }
  fprintf(stderr, "states: %ld\n", n);
  return 0;
}
