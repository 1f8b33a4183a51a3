// sig_slot.h -- signature slots (edverify.h EDV_SIG_SLOT96): the authenticator's base58 decode
// of the request signature (client_authn.py:89) moved off the host.  A slot is 96 bytes (24
// little-endian words); byte 95 = t > 0: bytes 0..t-1 are the base58 text of a signature that
// the host checked decodes to exactly 64 bytes (hostpack.cpp b58_len64), so its value is < 2^512
// and the decode is the 512-bit big-endian value of the text; t == 0: bytes 0..63 are R || S
// (decoded on the host: other lengths, which move bytes across the split at 64).
//
// The body of edv_b58_sig_kernel (edverify.hip), shared with the lane op sig_slot of
// csrc/ed_probe_ops.h.
#pragma once
#include <stdint.h>

#include "fe25519.h"

namespace edv {

EDV_HD uint32_t b58_digit(uint32_t c) {
  // '1'-'9' 0-8, 'A'-'H' 9-16, 'J'-'N' 17-21, 'P'-'Z' 22-32, 'a'-'k' 33-43, 'm'-'z' 44-57
  uint32_t d = c - '1';
  d = c >= 'A' ? c - 'A' + 9 - (c > 'H') - (c > 'N') : d;
  d = c >= 'a' ? c - 'a' + 33 - (c > 'k') : d;
  return d;
}

constexpr uint32_t kPow58[6] = {1u, 58u, 3364u, 195112u, 11316496u, 656356768u};

// out = the 64 signature bytes (16 words) of the slot w
EDV_HD void sig_slot_decode(uint32_t out[16], const uint32_t w[24]) {
  const uint32_t t = w[23] >> 24;
  if (t == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = w[j];
  } else {
    // Horner over groups of five digits (58^5 < 2^32): acc = acc * 58^k + chunk,
    // k = the group's digits inside the text (0..5, per lane)
    uint32_t acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
#pragma unroll
    for (int g = 0; g < 19; ++g) {
      uint32_t chunk = 0, k = 0;
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const int p = 5 * g + q;
        if (p < 95 && (uint32_t)p < t) {
          chunk = chunk * 58u + b58_digit((w[p >> 2] >> (8 * (p & 3))) & 0xffu);
          ++k;
        }
      }
      const uint32_t mul = k == 5 ? kPow58[5] : k == 4 ? kPow58[4] : k == 3 ? kPow58[3] : k == 2 ? kPow58[2]
                         : k == 1 ? kPow58[1] : kPow58[0];
      uint64_t carry = chunk;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const uint64_t v = (uint64_t)acc[j] * mul + carry;
        acc[j] = (uint32_t)v;
        carry = v >> 32;
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) out[j] = __builtin_bswap32(acc[15 - j]);  // big-endian bytes
  }
}

}  // namespace edv
