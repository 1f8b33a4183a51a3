// wire_scan.h -- one request's wire JSON text -> what the verify kernels need:
// the decoded 64-byte signature, the span of the identifier inside the text,
// and the signing serialization (SigningSerializer over the message with the
// top-level key "signature" dropped; plenum_amd/serialization.py).
//
// Compiled for the device (edv_wire_scan_kernel: text and output in LDS) and
// for the host (host_check.cpp hc_wire_scan, tools' sanitizer corpus runner).
//
// The scanner accepts a strict subset of JSON and never reports an error: any
// text outside the subset gets kWireHost ("the host decides": json.loads and
// the dict path).  The subset (DESIGN.md "Wire scan"):
//   whitespace  space \t \n \r between tokens; one top-level object, only
//               whitespace after it; text of at most kWireMaxText bytes
//   strings     bytes 0x20-0x7f; in values the escapes \" \\ \/ \b \f \n \r \t
//               are decoded, \u -> host; any backslash in a key -> host
//   numbers     -?(0|[1-9][0-9]*), at most kWireMaxDigits digits, emitted as
//               their text; -0, leading zeros, fractions, exponents -> host
//   literals    true -> True, false -> False, null -> ""
//   objects     "key:value" joined by "|" in ascending byte order of the keys;
//               at most kWireMaxMembers members; a duplicate key -> host; an
//               empty top-level object -> host
//   arrays      item texts joined by ","
//   nesting     at most kWireMaxDepth containers deep (explicit stack)
//   signature   top level: a non-empty string of at most kWireMaxSigChars
//               base58 characters, no backslash, whose b58decode is exactly 64
//               bytes (leading '1's + byte length of the value)
//   identifier  top level: a non-empty string, no backslash
// The serialization of an accepted text is never longer than the text (every
// emitted byte stands for a distinct text byte), so the caller may give `out`
// the size of the text; every write is bounds-checked against len all the same.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EDV_WS_HD __host__ __device__ __forceinline__
#else
#define EDV_WS_HD inline
#endif

namespace edv {

constexpr uint32_t kWireMaxText = 4096;    // longer items go to the host
constexpr int kWireMaxDepth = 8;
constexpr int kWireMaxMembers = 32;
constexpr int kWireMaxDigits = 18;
constexpr int kWireMaxSigChars = 95;
constexpr int kWireOk = 0;    // edverify.h EDV_WIRE_OK
constexpr int kWireHost = 1;  // edverify.h EDV_WIRE_HOST
constexpr uint32_t kWireFail = 0xffffffffu;

struct WireItem {
  uint32_t msg_len;    // bytes written to out
  uint32_t idr_start;  // the identifier's characters, relative to the text
  uint32_t idr_len;
  uint32_t sig[16];    // R || S as little-endian words of the byte stream
};

EDV_WS_HD bool ws_space(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
EDV_WS_HD bool ws_delim(uint32_t c) { return ws_space(c) || c == ',' || c == '}' || c == ']'; }

// base58 digit of c (Bitcoin alphabet), 255 outside it
EDV_WS_HD uint32_t ws_b58(uint32_t c) {
  if (c >= '1' && c <= '9') return c - '1';
  if (c >= 'A' && c <= 'Z') return (c == 'I' || c == 'O') ? 255u : c - 'A' + 9 - (c > 'I') - (c > 'O');
  if (c >= 'a' && c <= 'z') return c == 'l' ? 255u : c - 'a' + 33 - (c > 'l');
  return 255u;
}

template <class T>
EDV_WS_HD uint32_t ws_skip_space(T text, uint32_t p, uint32_t len) {
  while (p < len && ws_space(text[p])) ++p;
  return p;
}

// The end of the string whose opening quote is at p (lenient: the strict pass
// over the same bytes comes later), or kWireFail.
template <class T>
EDV_WS_HD uint32_t ws_skip_string(T text, uint32_t p, uint32_t len) {
  ++p;
  while (p < len) {
    const uint32_t c = text[p];
    if (c == '"') return p + 1;
    p += c == '\\' ? 2 : 1;
  }
  return kWireFail;
}

// The end of the value starting at p < len: structure only (strings, balanced
// brackets, a scalar up to its delimiter); every byte of it is checked when
// the value is emitted.
template <class T>
EDV_WS_HD uint32_t ws_skip_value(T text, uint32_t p, uint32_t len) {
  const uint32_t c0 = text[p];
  if (c0 == '"') return ws_skip_string(text, p, len);
  if (c0 == '{' || c0 == '[') {
    uint32_t depth = 0;
    while (p < len) {
      const uint32_t c = text[p];
      if (c == '"') {
        p = ws_skip_string(text, p, len);
        if (p == kWireFail) return kWireFail;
        continue;
      }
      if (c == '{' || c == '[') ++depth;
      if (c == '}' || c == ']') {
        if (--depth == 0) return p + 1;
      }
      ++p;
    }
    return kWireFail;
  }
  const uint32_t s = p;
  while (p < len && !ws_delim(text[p])) ++p;
  return p > s ? p : kWireFail;
}

// Keys at a and b (first character after the opening quote, no backslashes,
// closing quote inside the text): < 0, 0, > 0 in byte order.
template <class T>
EDV_WS_HD int ws_key_cmp(T text, uint32_t a, uint32_t b) {
  for (;; ++a, ++b) {
    const uint32_t ca = text[a], cb = text[b];
    if (ca == '"') return cb == '"' ? 0 : -1;
    if (cb == '"') return 1;
    if (ca != cb) return ca < cb ? -1 : 1;
  }
}

template <class T>
EDV_WS_HD bool ws_key_is(T text, uint32_t k, const char* name, uint32_t n) {
  for (uint32_t j = 0; j < n; ++j)
    if (text[k + j] != (uint8_t)name[j]) return false;  // (a shorter key stops at its quote)
  return text[k + n] == '"';
}

// The top-level signature string (opening quote at p) -> it.sig; false = host.
template <class T>
EDV_WS_HD bool ws_signature(T text, uint32_t p, uint32_t len, WireItem& it) {
  uint32_t q = p + 1, nz = 0;
  while (q < len && text[q] == '1') ++q, ++nz;
  // Horner over groups of up to five digits (58^5 < 2^32); 95 digits < 2^557
  uint32_t acc[18];
  for (int j = 0; j < 18; ++j) acc[j] = 0;
  uint32_t count = nz;
  for (;;) {
    uint32_t chunk = 0, mul = 1;
    bool closed = false;
    for (int k = 0; k < 5; ++k) {
      if (q >= len) return false;
      const uint32_t c = text[q];
      if (c == '"') {
        closed = true;
        break;
      }
      const uint32_t d = ws_b58(c);
      if (d == 255u) return false;
      if (++count > (uint32_t)kWireMaxSigChars) return false;
      chunk = chunk * 58u + d;
      mul *= 58u;
      ++q;
    }
    uint64_t carry = chunk;
    for (int j = 0; j < 18; ++j) {
      const uint64_t v = (uint64_t)acc[j] * mul + carry;
      acc[j] = (uint32_t)v;
      carry = v >> 32;
    }
    if (closed) break;
  }
  if (count == 0 || nz > 64) return false;
  // byte length of the value + the leading '1's (one zero byte each) == 64
  if (acc[16] | acc[17]) return false;
  uint32_t bytes = 0;
  for (int j = 15; j >= 0; --j)
    if (acc[j]) {
      bytes = 4 * (uint32_t)j + (acc[j] >> 24 ? 4 : acc[j] >> 16 ? 3 : acc[j] >> 8 ? 2 : 1);
      break;
    }
  if (bytes + nz != 64) return false;
  for (int j = 0; j < 16; ++j) {
    const uint32_t w = acc[15 - j];  // big-endian bytes of the 512-bit value
    it.sig[j] = (w >> 24) | ((w >> 8) & 0xff00u) | ((w << 8) & 0xff0000u) | (w << 24);
  }
  return true;
}

// Scan text[0 .. len) into out[0 .. it.msg_len) (out has room for len bytes)
// and it; kWireOk or kWireHost.  On kWireHost out and it hold no result.
template <class T, class O>
EDV_WS_HD int wire_scan_one(T text, uint32_t len, O out, WireItem& it) {
  if (len > kWireMaxText) return kWireHost;
  // the explicit stack: per open container its kind, for an object the
  // positions of its keys (sorted) and the one emitted next, the position
  // after its closing brace; for an array the position scanned so far
  uint16_t keys[kWireMaxDepth][kWireMaxMembers];
  uint16_t endp[kWireMaxDepth];  // object: after '}'; array: the cursor
  uint8_t count[kWireMaxDepth], next[kWireMaxDepth];
  uint32_t is_obj = 0, started = 0;  // bit per level: an object; something of it emitted / scanned
  int sp = -1;
  uint32_t o = 0;
  bool have_sig = false, have_idr = false;
#define EDV_WS_PUT(ch)               \
  do {                               \
    if (o >= len) return kWireHost;  \
    out[o++] = (uint8_t)(ch);        \
  } while (0)

  uint32_t vp = ws_skip_space(text, 0, len);
  if (vp >= len || text[vp] != '{') return kWireHost;
  for (;;) {
    // ---- emit the value at vp (< len); `e` = the position after it
    const uint32_t c = text[vp];
    uint32_t e = 0;
    bool opened = false;
    if (c == '{') {
      if (++sp >= kWireMaxDepth) return kWireHost;
      uint32_t q = ws_skip_space(text, vp + 1, len), n = 0;
      if (q >= len) return kWireHost;
      if (text[q] == '}') {
        if (sp == 0) return kWireHost;
        ++q;
      } else {
        for (;;) {
          q = ws_skip_space(text, q, len);
          if (q >= len || text[q] != '"') return kWireHost;
          if (n == (uint32_t)kWireMaxMembers) return kWireHost;
          keys[sp][n++] = (uint16_t)(++q);
          for (;; ++q) {
            if (q >= len) return kWireHost;
            const uint32_t k = text[q];
            if (k == '"') break;
            if (k == '\\' || k < 0x20 || k >= 0x80) return kWireHost;
          }
          q = ws_skip_space(text, q + 1, len);
          if (q >= len || text[q] != ':') return kWireHost;
          q = ws_skip_space(text, q + 1, len);
          if (q >= len) return kWireHost;
          q = ws_skip_value(text, q, len);
          if (q == kWireFail) return kWireHost;
          q = ws_skip_space(text, q, len);
          if (q >= len) return kWireHost;
          const uint32_t d = text[q++];
          if (d == '}') break;
          if (d != ',') return kWireHost;
        }
        for (uint32_t i = 1; i < n; ++i) {  // insertion sort by key bytes
          const uint16_t x = keys[sp][i];
          uint32_t j = i;
          while (j > 0) {
            const int cmp = ws_key_cmp(text, keys[sp][j - 1], x);
            if (cmp == 0) return kWireHost;  // duplicate key
            if (cmp < 0) break;
            keys[sp][j] = keys[sp][j - 1];
            --j;
          }
          keys[sp][j] = x;
        }
      }
      count[sp] = (uint8_t)n;
      next[sp] = 0;
      endp[sp] = (uint16_t)q;
      is_obj |= 1u << sp;
      started &= ~(1u << sp);
      opened = true;
    } else if (c == '[') {
      if (++sp >= kWireMaxDepth) return kWireHost;
      endp[sp] = (uint16_t)(vp + 1);
      is_obj &= ~(1u << sp);
      started &= ~(1u << sp);
      opened = true;
    } else if (c == '"') {
      uint32_t q = vp + 1;
      for (;; ++q) {
        if (q >= len) return kWireHost;
        uint32_t k = text[q];
        if (k == '"') break;
        if (k < 0x20 || k >= 0x80) return kWireHost;
        if (k == '\\') {
          if (++q >= len) return kWireHost;
          k = text[q];
          if (k == 'b') k = '\b';
          else if (k == 'f') k = '\f';
          else if (k == 'n') k = '\n';
          else if (k == 'r') k = '\r';
          else if (k == 't') k = '\t';
          else if (k != '"' && k != '\\' && k != '/') return kWireHost;
        }
        EDV_WS_PUT(k);
      }
      e = q + 1;
    } else if (c == '-' || (c >= '0' && c <= '9')) {
      uint32_t q = vp + (c == '-' ? 1 : 0);
      if (q >= len) return kWireHost;
      const uint32_t d0 = text[q];
      if (d0 < '0' || d0 > '9') return kWireHost;
      uint32_t digits = 0;
      while (q < len && text[q] >= '0' && text[q] <= '9') ++q, ++digits;
      if (digits > (uint32_t)kWireMaxDigits) return kWireHost;
      if (d0 == '0' && (digits > 1 || c == '-')) return kWireHost;  // leading zero, -0
      for (uint32_t j = vp; j < q; ++j) EDV_WS_PUT(text[j]);
      e = q;
    } else if (c == 't') {
      if (vp + 4 > len || text[vp + 1] != 'r' || text[vp + 2] != 'u' || text[vp + 3] != 'e') return kWireHost;
      EDV_WS_PUT('T');
      EDV_WS_PUT('r');
      EDV_WS_PUT('u');
      EDV_WS_PUT('e');
      e = vp + 4;
    } else if (c == 'f') {
      if (vp + 5 > len || text[vp + 1] != 'a' || text[vp + 2] != 'l' || text[vp + 3] != 's' || text[vp + 4] != 'e')
        return kWireHost;
      EDV_WS_PUT('F');
      EDV_WS_PUT('a');
      EDV_WS_PUT('l');
      EDV_WS_PUT('s');
      EDV_WS_PUT('e');
      e = vp + 5;
    } else if (c == 'n') {
      if (vp + 4 > len || text[vp + 1] != 'u' || text[vp + 2] != 'l' || text[vp + 3] != 'l') return kWireHost;
      e = vp + 4;
    } else {
      return kWireHost;
    }
    if (!opened) {
      // a scalar ends at a delimiter (it is always inside a container); its array goes on from there
      if (c != '"' && (e >= len || !ws_delim(text[e]))) return kWireHost;
      if (!(is_obj >> sp & 1)) endp[sp] = (uint16_t)e;
    }
    // ---- the next value: of the innermost open container, closing those that are done
    bool more = false;
    while (sp >= 0) {
      if (is_obj >> sp & 1) {
        if (next[sp] == count[sp]) {
          const uint32_t after = endp[sp];
          if (--sp >= 0 && !(is_obj >> sp & 1)) endp[sp] = (uint16_t)after;
          if (sp < 0 && ws_skip_space(text, after, len) != len) return kWireHost;  // only whitespace follows
          continue;
        }
        const uint32_t k = keys[sp][next[sp]++];
        uint32_t q = k;
        while (text[q] != '"') ++q;  // (checked when the key was collected, as the ':' is)
        const uint32_t kend = q;
        q = ws_skip_space(text, q + 1, len);
        q = ws_skip_space(text, q + 1, len);
        if (sp == 0 && ws_key_is(text, k, "signature", 9)) {
          if (text[q] != '"' || !ws_signature(text, q, len, it)) return kWireHost;
          have_sig = true;
          continue;
        }
        if (sp == 0 && ws_key_is(text, k, "identifier", 10)) {
          if (text[q] != '"') return kWireHost;
          uint32_t z = q + 1;
          for (;; ++z) {
            if (z >= len) return kWireHost;
            const uint32_t ch = text[z];
            if (ch == '"') break;
            if (ch == '\\' || ch < 0x20 || ch >= 0x80) return kWireHost;
          }
          if (z == q + 1) return kWireHost;
          it.idr_start = q + 1;
          it.idr_len = z - q - 1;
          have_idr = true;
        }
        if (started >> sp & 1) EDV_WS_PUT('|');
        started |= 1u << sp;
        for (uint32_t j = k; j < kend; ++j) EDV_WS_PUT(text[j]);
        EDV_WS_PUT(':');
        vp = q;
        more = true;
        break;
      }
      uint32_t q = ws_skip_space(text, endp[sp], len);
      if (q >= len) return kWireHost;
      const uint32_t d = text[q];
      if (d == ']') {
        if (--sp >= 0 && !(is_obj >> sp & 1)) endp[sp] = (uint16_t)(q + 1);
        continue;  // (sp < 0 cannot happen: the top level is an object)
      }
      if (started >> sp & 1) {
        if (d != ',') return kWireHost;
        q = ws_skip_space(text, q + 1, len);
        if (q >= len) return kWireHost;
        EDV_WS_PUT(',');
      }
      started |= 1u << sp;
      vp = q;
      more = true;
      break;
    }
    if (!more) break;
  }
#undef EDV_WS_PUT
  if (!have_sig || !have_idr) return kWireHost;
  it.msg_len = o;
  return kWireOk;
}

}  // namespace edv
