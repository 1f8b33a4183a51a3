// wire_unwrap.h -- one node message's wire text -> a text wire_scan.h accepts: the bytes of the
// signed request object it carries, at their own positions, and spaces everywhere else (the
// scanner allows whitespace around its one top-level object, and unescaping a JSON string body
// never lengthens it, so the result fits the message's own span: no compaction, no new offsets).
//
// Compiled for the device (edv_wire_unwrap_kernel: text and output in LDS) and for the host
// (host_check.cpp hc_wire_unwrap, the sanitizer corpus runner).  tests/wire_unwrap_model.py
// restates it in Python.
//
// A message is a client request, a PROPAGATE or anything else a node receives, either as the
// bytes of an rxMsgs entry (esc = 0) or as the body of a string of a BATCH's `messages` (esc = 1:
// still escaped, _hostpack.gather_node_texts cut it out of the BATCH).  The classes mirror
// plenum_amd/batching.py _collect:
//   kUnwrapRequest  out holds the request object: scan it
//   kUnwrapHost     "the host decides": the caller decodes the message itself (never an error)
//   kUnwrapNone     the message holds no signed request, whatever else it is
// Rules (DESIGN.md "Node messages"):
//   unescape    esc = 1: bytes 0x20-0x7e; the escapes \" \\ \/ \b \f \n \r \t; anything else -> host
//   top level   one object, only whitespace around it; keys without backslashes, bytes 0x20-0x7f;
//               values skipped structurally (ws_skip_value); at most kWireMaxMembers members;
//               a second "op", "request" or "signature" -> host; at most kWireMaxText bytes
//   op          a string with a backslash -> host; "BATCH" -> host (nested, or declined by the
//               splitter); "PROPAGATE" -> the request is the value of "request":
//                 not an object -> none; no key "signature" in it -> none (its keys are walked
//                 like the top level's); every other member of the PROPAGATE a scalar of the
//                 scanner's grammar, strictly checked (the scan never sees the envelope) -> else host
//               anything else, or no "op": with a top-level "signature" the whole object is the
//               request (the scanner validates all of it), without one -> none
// kUnwrapNone is only claimed where json.loads either fails or yields no signed request; where
// that is not certain the class is kUnwrapHost.
#pragma once
#include "wire_scan.h"

namespace edv {

constexpr int kUnwrapRequest = 0;  // edverify.h EDV_NODE_REQUEST
constexpr int kUnwrapHost = 1;     // edverify.h EDV_NODE_HOST
constexpr int kUnwrapNone = 2;     // edverify.h EDV_NODE_NONE

struct UnwrapWalk {
  uint32_t end;           // the position after the object's closing brace
  uint32_t op_v, op_e;    // the value of "op" (kWireFail: no such key) and the position after it
  uint32_t req_v, req_e;  // the value of "request"
  bool sig;               // a key "signature"
};

// A scalar of the scanner's grammar exactly filling t[v .. e): a string with the simple escapes,
// -?(0|[1-9][0-9]*) of at most kWireMaxDigits digits, true / false / null.
template <class T>
EDV_WS_HD bool wu_scalar(T t, uint32_t v, uint32_t e) {
  const uint32_t c = t[v];
  if (c == '"') {
    for (uint32_t q = v + 1; q < e; ++q) {
      uint32_t k = t[q];
      if (k == '"') return q + 1 == e;
      if (k < 0x20 || k >= 0x80) return false;
      if (k == '\\') {
        if (++q >= e) return false;
        k = t[q];
        if (k != '"' && k != '\\' && k != '/' && k != 'b' && k != 'f' && k != 'n' && k != 'r' && k != 't') return false;
      }
    }
    return false;
  }
  if (c == '-' || (c >= '0' && c <= '9')) {
    uint32_t q = v + (c == '-' ? 1 : 0);
    if (q >= e) return false;
    const uint32_t d0 = t[q];
    uint32_t digits = 0;
    while (q < e && t[q] >= '0' && t[q] <= '9') ++q, ++digits;
    if (q != e || digits == 0 || digits > (uint32_t)kWireMaxDigits) return false;
    return !(d0 == '0' && (digits > 1 || c == '-'));  // leading zero, -0
  }
  if (e - v == 4)
    return (c == 't' && t[v + 1] == 'r' && t[v + 2] == 'u' && t[v + 3] == 'e') ||
           (c == 'n' && t[v + 1] == 'u' && t[v + 2] == 'l' && t[v + 3] == 'l');
  if (e - v == 5) return c == 'f' && t[v + 1] == 'a' && t[v + 2] == 'l' && t[v + 3] == 's' && t[v + 4] == 'e';
  return false;
}

// The members of the object opening at p (t[p] == '{') inside t[0 .. m): false = the host
// decides.  strict: every value but the one at `except` must be a scalar (wu_scalar).
template <class T>
EDV_WS_HD bool wu_walk(T t, uint32_t p, uint32_t m, bool strict, uint32_t except, UnwrapWalk& w) {
  w.op_v = w.req_v = kWireFail;
  w.op_e = w.req_e = 0;
  w.sig = false;
  uint32_t q = ws_skip_space(t, p + 1, m), members = 0;
  if (q >= m) return false;
  if (t[q] == '}') {
    w.end = q + 1;
    return true;
  }
  for (;;) {
    q = ws_skip_space(t, q, m);
    if (q >= m || t[q] != '"') return false;
    if (members++ == (uint32_t)kWireMaxMembers) return false;
    const uint32_t k = ++q;
    for (;; ++q) {
      if (q >= m) return false;
      const uint32_t c = t[q];
      if (c == '"') break;
      if (c == '\\' || c < 0x20 || c >= 0x80) return false;
    }
    q = ws_skip_space(t, q + 1, m);
    if (q >= m || t[q] != ':') return false;
    q = ws_skip_space(t, q + 1, m);
    if (q >= m) return false;
    const uint32_t v = q;
    q = ws_skip_value(t, q, m);
    if (q == kWireFail) return false;
    if (strict && v != except && !wu_scalar(t, v, q)) return false;
    if (ws_key_is(t, k, "op", 2)) {
      if (w.op_v != kWireFail) return false;
      w.op_v = v;
      w.op_e = q;
    } else if (ws_key_is(t, k, "request", 7)) {
      if (w.req_v != kWireFail) return false;
      w.req_v = v;
      w.req_e = q;
    } else if (ws_key_is(t, k, "signature", 9)) {
      if (w.sig) return false;
      w.sig = true;
    }
    q = ws_skip_space(t, q, m);
    if (q >= m) return false;
    const uint32_t d = t[q++];
    if (d == '}') break;
    if (d != ',') return false;
  }
  w.end = q;
  return true;
}

// text[0 .. len) -> out[0 .. len) and the class.  kUnwrapRequest: out holds the request object at
// the place it has in the (unescaped) text and ' ' elsewhere; any other class: ' ' throughout.  A
// text longer than kWireMaxText is kUnwrapHost with out untouched (wire_scan_one leaves such an
// item to the host unread).  out is read back, so O indexes to something assignable and readable.
template <class T, class O>
EDV_WS_HD int wire_unwrap_one(T text, uint32_t len, uint32_t esc, O out) {
  if (len > kWireMaxText) return kUnwrapHost;
  uint32_t m = 0;  // bytes of the copy
  bool bad = false;
  if (esc) {
    for (uint32_t p = 0; p < len; ++p) {
      uint32_t c = text[p];
      if (c < 0x20 || c > 0x7e) bad = true;
      if (c == '\\') {
        c = ++p < len ? (uint32_t)text[p] : 0u;
        if (c == 'b') c = '\b';
        else if (c == 'f') c = '\f';
        else if (c == 'n') c = '\n';
        else if (c == 'r') c = '\r';
        else if (c == 't') c = '\t';
        else if (c != '"' && c != '\\' && c != '/') bad = true;
      }
      if (bad) break;
      if (m < len) out[m++] = (uint8_t)c;
    }
  } else {
    for (; m < len; ++m) out[m] = (uint8_t)text[m];
  }
  uint32_t a = 0, b = 0;  // the request object, [a, b) of out
  int cls = kUnwrapHost;
  do {
    if (bad) break;
    const uint32_t p = ws_skip_space(out, 0, m);
    if (p >= m || out[p] != '{') break;
    UnwrapWalk top;
    if (!wu_walk(out, p, m, false, kWireFail, top)) break;
    if (ws_skip_space(out, top.end, m) != m) break;  // only whitespace follows
    int op = 0;                                      // 1 PROPAGATE, 2 BATCH
    if (top.op_v != kWireFail && out[top.op_v] == '"') {
      bool slash = false;
      for (uint32_t q = top.op_v + 1; q + 1 < top.op_e; ++q) slash |= out[q] == '\\';
      if (slash) break;
      if (ws_key_is(out, top.op_v + 1, "PROPAGATE", 9)) op = 1;
      if (ws_key_is(out, top.op_v + 1, "BATCH", 5)) op = 2;
    }
    if (op == 2) break;
    if (op == 0) {
      cls = top.sig ? kUnwrapRequest : kUnwrapNone;
      a = p;
      b = top.end;
      break;
    }
    if (top.req_v == kWireFail || out[top.req_v] != '{') {
      cls = kUnwrapNone;
      break;
    }
    UnwrapWalk req;
    if (!wu_walk(out, top.req_v, top.req_e, false, kWireFail, req) || req.end != top.req_e) break;
    if (!req.sig) {
      cls = kUnwrapNone;
      break;
    }
    UnwrapWalk again;
    if (!wu_walk(out, p, m, true, top.req_v, again)) break;  // the envelope, strictly
    cls = kUnwrapRequest;
    a = top.req_v;
    b = top.req_e;
  } while (0);
  if (cls != kUnwrapRequest) a = b = 0;
  for (uint32_t q = 0; q < a; ++q) out[q] = ' ';
  for (uint32_t q = b; q < len; ++q) out[q] = ' ';
  return cls;
}

}  // namespace edv
