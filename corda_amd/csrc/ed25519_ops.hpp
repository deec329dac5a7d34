// Ed25519 pieces shared by the verification prep / corpus signer (ed25519.hip)
// and the keyed signer (ed25519_sign.hip): the base point, an affine niels
// table entry from a point, SHA-512 over register segments plus a message, and
// (a b + c) mod L.
#pragma once
#include "ed25519_ws.hpp"
#include "sha2_device.hpp"

namespace cordahip {

CDEV void ge_base(ge_p3& b) {
  const uint32_t bx[10] = {0x325d51a, 0x18b5823, 0xf6592a, 0x104a92d, 0x1a4b31d,
                           0x1d6dc5c, 0x27118fe, 0x7fd814, 0x13cd6e5, 0x85a4db};
  const uint32_t by[10] = {0x2666658, 0x1999999, 0xcccccc, 0x1333333, 0x1999999,
                           0x666666, 0x3333333, 0xcccccc, 0x2666666, 0x1999999};
  const uint32_t bt[10] = {0x1b7dda3, 0x1a2ace9, 0x25eadbb, 0x3ba8a, 0x83c27e,
                           0xabe37d, 0x1274732, 0xccacdd, 0xfd78b7, 0x19e1d7c};
#pragma unroll
  for (int i = 0; i < 10; i++) {
    b.X.v[i] = bx[i];
    b.Y.v[i] = by[i];
    b.T.v[i] = bt[i];
  }
  fe_set(b.Z, 1);
}

// P as an affine niels table entry (y+x, y-x, 2d*x*y; 30 limbs + 2 pad words)
CDEV void store_niels_entry(uint32_t* __restrict__ o, const ge_p3& P) {
  fe zi, x, y, t, d2;
  fe_invert(zi, P.Z);
  fe_mul(x, P.X, zi);
  fe_mul(y, P.Y, zi);
  fe_const_d2(d2);
  ge_niels n;
  fe_add(n.ypx, y, x);
  fe_carry(n.ypx);
  fe_sub(n.ymx, y, x);
  fe_mul(t, x, y);
  fe_mul(n.xy2d, t, d2);
#pragma unroll
  for (int i = 0; i < 10; i++) {
    o[i] = n.ypx.v[i];
    o[10 + i] = n.ymx.v[i];
    o[20 + i] = n.xy2d.v[i];
  }
  o[30] = 0;
  o[31] = 0;
}

// ---------------------------------------------------------------------------
// SHA-512 over  seg0(32 B, registers) || seg1(32 B, registers, optional) || msg
// (global, msg_len bytes). Fast path: everything fits one block with msg_len
// a multiple of 8 bytes' worth of whole words read as registers.
CDEV uint32_t byte_of(const uint32_t w[8], int idx) { return (word_sel(w, idx >> 2) >> (8 * (idx & 3))) & 0xffu; }

CDEV void sha512_segments(uint32_t out_le[16], const uint32_t s0[8], const uint32_t s1[8], bool has_s1,
                          const uint8_t* __restrict__ msg, uint32_t msg_len) {
  uint64_t h[8];
  sha512_init(h);
  const uint32_t pre = has_s1 ? 64u : 32u;
  const uint64_t total = (uint64_t)pre + msg_len;
  uint64_t w[16];
  if (has_s1 && msg_len == 32) {
    // hot shape: R || A || txId = 96 bytes, one block
    const uint4* m4 = reinterpret_cast<const uint4*>(msg);
    const uint4 ma = m4[0], mb = m4[1];
    const uint32_t m[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      w[q] = ((uint64_t)bswap32(s0[2 * q]) << 32) | bswap32(s0[2 * q + 1]);
      w[4 + q] = ((uint64_t)bswap32(s1[2 * q]) << 32) | bswap32(s1[2 * q + 1]);
      w[8 + q] = ((uint64_t)bswap32(m[2 * q]) << 32) | bswap32(m[2 * q + 1]);
    }
    w[12] = 0x8000000000000000ULL;
    w[13] = 0;
    w[14] = 0;
    w[15] = total * 8;
    sha512_block(h, w);
  } else {
#ifndef ED_NO_GENERIC_SHA
    const uint64_t nblocks = (total + 17 + 127) / 128;
    for (uint64_t b = 0; b < nblocks; b++) {
      for (int q = 0; q < 16; q++) {
        uint64_t word = 0;
        for (int k = 0; k < 8; k++) {
          const uint64_t pos = b * 128 + (uint64_t)q * 8 + k;
          uint32_t byte;
          if (pos < 32) byte = byte_of(s0, (int)pos);
          else if (pos < pre) byte = byte_of(s1, (int)(pos - 32));
          else if (pos < total) byte = msg[pos - pre];
          else if (pos == total) byte = 0x80;
          else if (b == nblocks - 1 && q == 15) byte = (uint32_t)(((total * 8) >> (8 * (7 - k))) & 0xff);
          else byte = 0;
          word = (word << 8) | byte;
        }
        w[q] = word;
      }
      sha512_block(h, w);
    }
#endif
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out_le[2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out_le[2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

// out = (a b + c) mod L. SELECT: the reduction's final subtractions are selects
// (sc_reduce512), for scalars that are secret.
template <bool SELECT = false>
CDEV void sc_muladd(uint32_t out[8], const uint32_t a[8], const uint32_t b[8], const uint32_t c[8]) {
  uint32_t x[16];
#pragma unroll
  for (int i = 0; i < 16; i++) x[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)a[i] * b[j] + x[i + j] + carry;
      x[i + j] = (uint32_t)t;
      carry = t >> 32;
    }
    x[i + 8] = (uint32_t)carry;
  }
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint64_t t = (uint64_t)x[i] + (i < 8 ? c[i] : 0u) + carry;
    x[i] = (uint32_t)t;
    carry = t >> 32;
  }
  sc_reduce512<SELECT>(out, x);
}

}  // namespace cordahip
