// wire_digest.h -- which items of a scanned wire batch have their Request.digest
// in the bytes the scan already wrote.
//
// Compiled for the device (edv_wire_digest_kernel, edverify.hip: one lane per
// item) and for the host (host_check.cpp hc_wire_digests and
// wire_corpus_check.cpp: the same code run serially, every read asserted inside
// the item's text).
//
// Request.digest is sha256(serialize_msg_for_signing(signingState))
// (plenum/common/request.py:51-52), signingState = {identifier, reqId,
// operation[, protocolVersion if not None]} (request.py:61-71).  The scan wrote
// serialize(request without "signature") -- the bytes the signature covers.  The
// two are the same bytes exactly when
//   every top-level key is one of identifier / reqId / operation /
//     protocolVersion / signature  (any other key is signed but not in the state),
//   reqId and operation are present  (the state always has both, None for a
//     missing one -- "reqId:" -- where the signed bytes have no such member; a
//     null VALUE serializes to the same "reqId:"),
//   protocolVersion is absent or not null  (the state drops a None, the signed
//     bytes keep "protocolVersion:").
// wd_eligible decides that from the TOP LEVEL of the item's text alone.
//
// The text is one the scanner gave status 0, so it is inside the scanner's
// grammar (wire_scan.h): one object, no backslash in a key, no duplicate keys,
// depth <= 8, string bytes 0x20-0x7f, a backslash in a value followed by one
// byte of its escape.  The walk therefore needs whitespace, an in-string state
// that steps over the byte after a backslash, a depth counter, a byte-exact
// compare of the depth-1 keys with the five names, and the first byte of
// protocolVersion's value.  It reads text[at .. at + len) only, front to back,
// each byte once (the device accessor keeps the current 16 bytes in registers);
// a text that ends before its object closes returns 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EDV_WD_HD __host__ __device__ __forceinline__
#else
#define EDV_WD_HD inline
#endif

namespace edv {

// the five names back to back; a name is found by its first byte (all differ)
constexpr uint32_t kWdIdentifier = 0, kWdReqId = 1, kWdOperation = 2, kWdProtocol = 3, kWdSignature = 4, kWdNone = 5;

EDV_WD_HD uint32_t wd_name_of(uint32_t first_byte) {
  return first_byte == 'i' ? kWdIdentifier
       : first_byte == 'r' ? kWdReqId
       : first_byte == 'o' ? kWdOperation
       : first_byte == 'p' ? kWdProtocol
       : first_byte == 's' ? kWdSignature
                           : kWdNone;
}
EDV_WD_HD uint32_t wd_name_at(uint32_t name) {  // where the name starts in wd_name_byte's string
  return name == kWdIdentifier ? 0u : name == kWdReqId ? 10u : name == kWdOperation ? 15u : name == kWdProtocol ? 24u : 39u;
}
EDV_WD_HD uint32_t wd_name_len(uint32_t name) {
  return name == kWdIdentifier ? 10u : name == kWdReqId ? 5u : name == kWdOperation ? 9u : name == kWdProtocol ? 15u : 9u;
}
EDV_WD_HD uint32_t wd_name_byte(uint32_t k) {
  return (uint32_t)(uint8_t)"identifierreqIdoperationprotocolVersionsignature"[k];
}

EDV_WD_HD bool wd_space(uint32_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }

// 1: the item's serialization (what the scan wrote) is its signingState's.
// T: text[b] = byte b, asked for in ascending order.
template <class T>
EDV_WD_HD uint32_t wd_eligible(T text, uint64_t at, uint32_t len) {
  uint32_t p = 0;
  while (p < len && wd_space(text[at + p])) ++p;
  if (p >= len || text[at + p] != '{') return 0;
  ++p;
  uint32_t depth = 1, seen = 0;
  bool want_key = true;  // at depth 1, before a member's key
  while (p < len) {
    const uint32_t c = text[at + p];
    ++p;
    if (c == '"') {
      if (depth == 1 && want_key) {
        // the key, byte for byte against the one name that starts like it
        uint32_t name = kWdNone, k = 0, j = 0, end = 0;
        bool same = true, closed = false;
        while (p < len) {
          const uint32_t b = text[at + p];
          ++p;
          if (b == '"') {
            closed = true;
            break;
          }
          if (b == '\\') {  // (never: the scan sends such a key to the host)
            same = false;
            ++p;
            continue;
          }
          if (j == 0) {
            name = wd_name_of(b);
            k = wd_name_at(name);
            end = name == kWdNone ? 0u : wd_name_len(name);
          }
          same = same && j < end && b == wd_name_byte(k + j);
          ++j;
        }
        if (!closed) return 0;
        if (!same || j != end || j == 0) return 0;  // a key of its own: signed, not in the state
        seen |= 1u << name;
        want_key = false;
        while (p < len && wd_space(text[at + p])) ++p;
        if (p >= len || text[at + p] != ':') return 0;
        ++p;
        while (p < len && wd_space(text[at + p])) ++p;
        if (p >= len) return 0;
        if (name == kWdProtocol && text[at + p] == 'n') return 0;  // null: dropped from the state
      } else {
        bool closed = false;
        while (p < len) {
          const uint32_t b = text[at + p];
          ++p;
          if (b == '"') {
            closed = true;
            break;
          }
          if (b == '\\') ++p;
        }
        if (!closed) return 0;
      }
    } else if (c == '{' || c == '[') {
      ++depth;
    } else if (c == '}' || c == ']') {
      if (--depth == 0) {
        const uint32_t need = (1u << kWdReqId) | (1u << kWdOperation);
        return (seen & need) == need ? 1u : 0u;
      }
    } else if (c == ',' && depth == 1) {
      want_key = true;
    }
  }
  return 0;  // the text ended inside its object
}

}  // namespace edv
