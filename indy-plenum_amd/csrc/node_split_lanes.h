// node_split_lanes.h -- the BATCH split of node_split.h as lane code: what a lane of
// edv_node_split_count_kernel / edv_node_split_emit_kernel (edverify.hip) does with its 16 bytes
// of an rxMsgs entry, and the two short serial walks around the member array.  Compiled for the
// device and for the host (host_check.cpp hc_node_split_lanes: the same functions as an emulated
// wave; the sanitizer corpus runner).  The definition is node_split.h's: for every entry the same
// verdict and the same member spans, nothing else.
//
// The entry is  head [ members ] tail  with
//   head   { "op" : "BATCH" , "messages" : [        nsl_head, serial
//   tail   (, key : scalar)* } and whitespace       nsl_tail, serial
// and the member array between them is a seven-state automaton over its bytes:
//   START  after the '[' (whitespace stays; '"' -> IN; ']' -> DONE)
//   IN     inside a member ('"' -> AFTER; '\' -> ESC)
//   ESC    after a backslash in a member (one of " \ / b f n r t -> IN)
//   AFTER  after a member's closing quote (whitespace stays; ',' -> COMMA; ']' -> DONE)
//   COMMA  after a comma (whitespace stays; '"' -> IN)
//   DONE   after the ']' (absorbing)      ERR  anything else (absorbing)
// A lane folds its 16 bytes into the map state -> state (3 bits per state in a uint32); the wave
// composes the maps with an exclusive scan and carries the running state from one 1,024-byte
// step to the next; each lane then replays its bytes from its true entry state and meets the
// member starts ('"' taken in START or COMMA), the member ends ('"' taken in IN) and the ']'.
// With D = (sum of the ends met so far) - (sum of the starts met so far), a member's bytes lie
// D bytes into the entry's bodies when its start is met: the same exclusive scan over the lanes'
// (members, D) gives every member its message index and its place among the bodies.
#pragma once
#include "wire_scan.h"

namespace edv {

constexpr uint32_t kNslStart = 0, kNslIn = 1, kNslEsc = 2, kNslAfter = 3, kNslComma = 4, kNslDone = 5, kNslErr = 6;
constexpr uint32_t kNslStates = 7;
constexpr uint32_t kNslLanes = 64, kNslLaneBytes = 16, kNslStep = kNslLanes * kNslLaneBytes;
constexpr uint64_t kNslFail = ~0ull;

EDV_WS_HD constexpr uint32_t nsl_next(uint32_t s, uint32_t c) {
  const bool sp = c == ' ' || c == '\t' || c == '\n' || c == '\r';
  switch (s) {
    case kNslStart: return sp ? kNslStart : c == '"' ? kNslIn : c == ']' ? kNslDone : kNslErr;
    case kNslIn: return c == '"' ? kNslAfter : c == '\\' ? kNslEsc : kNslIn;
    case kNslEsc:
      return (c == '"' || c == '\\' || c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't') ? kNslIn
                                                                                                           : kNslErr;
    case kNslAfter: return sp ? kNslAfter : c == ',' ? kNslComma : c == ']' ? kNslDone : kNslErr;
    case kNslComma: return sp ? kNslComma : c == '"' ? kNslIn : kNslErr;
    case kNslDone: return kNslDone;
    default: return kNslErr;
  }
}

// a map: state s goes to (map >> 3 s) & 7
EDV_WS_HD constexpr uint32_t nsl_apply(uint32_t map, uint32_t s) { return (map >> (3 * s)) & 7u; }
EDV_WS_HD constexpr uint32_t nsl_map_of(uint32_t c) {
  uint32_t m = 0;
  for (uint32_t s = 0; s < kNslStates; ++s) m |= nsl_next(s, c) << (3 * s);
  return m;
}
constexpr uint32_t kNslIdentity = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12 | 5u << 15 | 6u << 18;

// f first, then g
EDV_WS_HD uint32_t nsl_compose(uint32_t f, uint32_t g) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t s = 0; s < kNslStates; ++s) m |= nsl_apply(g, nsl_apply(f, s)) << (3 * s);
  return m;
}

// one byte's map: seven classes of bytes
EDV_WS_HD uint32_t nsl_byte_map(uint32_t c) {
  constexpr uint32_t space = nsl_map_of(' '), quote = nsl_map_of('"'), slash = nsl_map_of('\\'),
                     comma = nsl_map_of(','), close = nsl_map_of(']'), letter = nsl_map_of('n'), other = nsl_map_of('x');
  if (c == '"') return quote;
  if (c == '\\') return slash;
  if (c == ',') return comma;
  if (c == ']') return close;
  if (c == ' ' || c == '\t' || c == '\n' || c == '\r') return space;
  if (c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't') return letter;
  return other;
}

// A lane's 16 bytes, the bytes at q0 .. q0 + 16 of the buffer (q0 a multiple of 16): byte k is the
// entry's for lo <= k < hi.
struct NslBytes {
  uint32_t w[4];
  uint32_t lo, hi;
  EDV_WS_HD uint32_t at(uint32_t k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
};

// [lo, hi) for the block at q0 of the entry at [ea, eb) of the buffer
EDV_WS_HD void nsl_bounds(uint64_t q0, uint64_t ea, uint64_t eb, uint32_t& lo, uint32_t& hi) {
  const uint64_t a = ea > q0 ? ea : q0, b = eb < q0 + kNslLaneBytes ? eb : q0 + kNslLaneBytes;
  lo = a < b ? (uint32_t)(a - q0) : 0u;
  hi = a < b ? (uint32_t)(b - q0) : 0u;
}

// The lane's bytes read one at a time through t (t[i] = byte i of the entry): only the entry's own.
template <class T>
EDV_WS_HD NslBytes nsl_load_bytes(T t, uint64_t q0, uint64_t ea, uint64_t eb) {
  NslBytes x;
  x.w[0] = x.w[1] = x.w[2] = x.w[3] = 0;
  nsl_bounds(q0, ea, eb, x.lo, x.hi);
  for (uint32_t k = x.lo; k < x.hi; ++k) x.w[k >> 2] |= (uint32_t)t[q0 + k - ea] << (8 * (k & 3));
  return x;
}

// The map of the lane's bytes at or after arr (the first byte after the '['); bad: a byte of the
// entry outside 0x20-0x7e, wherever it lies.
EDV_WS_HD uint32_t nsl_lane_map(const NslBytes& x, uint64_t q0, uint64_t arr, bool& bad) {
  uint32_t s0 = kNslStart, s1 = kNslIn, s2 = kNslEsc, s3 = kNslAfter, s4 = kNslComma;
#pragma unroll
  for (uint32_t k = 0; k < kNslLaneBytes; ++k) {
    if (k < x.lo || k >= x.hi) continue;
    const uint32_t c = x.at(k);
    bad |= c < 0x20 || c > 0x7e;
    if (q0 + k < arr) continue;
    const uint32_t m = nsl_byte_map(c);
    s0 = nsl_apply(m, s0);
    s1 = nsl_apply(m, s1);
    s2 = nsl_apply(m, s2);
    s3 = nsl_apply(m, s3);
    s4 = nsl_apply(m, s4);
  }
  return s0 | s1 << 3 | s2 << 6 | s3 << 9 | s4 << 12 | kNslDone << 15 | kNslErr << 18;
}

// What a lane carries through its bytes: the state, the members started and D before its first
// byte (in) and after its last (out), and the position of the ']' if it met it.
struct NslRun {
  uint32_t state;
  uint64_t members, delta, close;
};

struct NslNoEmit {
  EDV_WS_HD void operator()(uint64_t, uint64_t, uint64_t) const {}
};

// The lane's bytes again from its true state.  emit(index, body, first): the member with that
// index among the entry's starts at byte `first` of the buffer, `body` bytes into the entry's bodies.
template <class E>
EDV_WS_HD void nsl_lane_replay(const NslBytes& x, uint64_t q0, uint64_t arr, NslRun& r, E emit) {
#pragma unroll
  for (uint32_t k = 0; k < kNslLaneBytes; ++k) {
    if (k < x.lo || k >= x.hi || q0 + k < arr) continue;
    const uint32_t s = r.state, t = nsl_apply(nsl_byte_map(x.at(k)), s);
    const uint64_t q = q0 + k;
    if (t == kNslIn && (s == kNslStart || s == kNslComma)) {
      emit(r.members, r.delta, q + 1);
      r.members += 1;
      r.delta -= q + 1;
    } else if (t == kNslAfter && s == kNslIn) {
      r.delta += q;
    } else if (t == kNslDone && s != kNslDone) {
      r.close = q;
    }
    r.state = t;
  }
}

// ---- the head and the tail, serial, by node_split.h's rules; t[i] = byte i of the entry of n bytes
template <class T>
EDV_WS_HD uint64_t nsl_space(T t, uint64_t p, uint64_t n) {
  while (p < n && ws_space(t[p])) ++p;
  return p;
}

// t[p .. p + k) == word, with the closing quote after it
template <class T>
EDV_WS_HD bool nsl_word(T t, uint64_t p, uint64_t n, const char* word, uint64_t k) {
  if (!(p + k < n)) return false;
  for (uint64_t j = 0; j < k; ++j)
    if (t[p + j] != (uint8_t)word[j]) return false;
  return t[p + k] == '"';
}

// The position after the '[' of { "op" : "BATCH" , "messages" : [, or kNslFail.
template <class T>
EDV_WS_HD uint64_t nsl_head(T t, uint64_t n) {
  uint64_t p = nsl_space(t, 0, n);
  if (p >= n || t[p] != '{') return kNslFail;
  p = nsl_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !nsl_word(t, p + 1, n, "op", 2)) return kNslFail;
  p = nsl_space(t, p + 4, n);
  if (p >= n || t[p] != ':') return kNslFail;
  p = nsl_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !nsl_word(t, p + 1, n, "BATCH", 5)) return kNslFail;
  p = nsl_space(t, p + 7, n);
  if (p >= n || t[p] != ',') return kNslFail;
  p = nsl_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !nsl_word(t, p + 1, n, "messages", 8)) return kNslFail;
  p = nsl_space(t, p + 10, n);
  if (p >= n || t[p] != ':') return kNslFail;
  p = nsl_space(t, p + 1, n);
  if (p >= n || t[p] != '[') return kNslFail;
  return p + 1;
}

// From p, the position after the ']': (, key : null | true | false | integer | plain string)* }
// and only whitespace to the end.
template <class T>
EDV_WS_HD bool nsl_tail(T t, uint64_t p, uint64_t n) {
  for (;;) {
    p = nsl_space(t, p, n);
    if (p >= n) return false;
    const uint32_t d = t[p++];
    if (d == '}') break;
    if (d != ',') return false;
    p = nsl_space(t, p, n);
    if (p >= n || t[p] != '"') return false;
    const uint64_t k = ++p;
    for (;; ++p) {
      if (p >= n) return false;
      const uint32_t c = t[p];
      if (c == '"') break;
      if (c == '\\') return false;
    }
    if (p - k == 2 && t[k] == 'o' && t[k + 1] == 'p') return false;
    if (p - k == 8 && nsl_word(t, k, n, "messages", 8)) return false;
    p = nsl_space(t, p + 1, n);
    if (p >= n || t[p] != ':') return false;
    p = nsl_space(t, p + 1, n);
    if (p >= n) return false;
    const uint32_t c = t[p];
    if (c == '"') {
      for (++p;; ++p) {
        if (p >= n) return false;
        const uint32_t e = t[p];
        if (e == '\\') return false;
        if (e == '"') break;
      }
      ++p;
      continue;
    }
    const uint64_t v = p;
    while (p < n && t[p] != ' ' && t[p] != ',' && t[p] != '}' && t[p] != ']') ++p;
    const uint64_t w = p - v;
    if (w == 4 && ((c == 'n' && t[v + 1] == 'u' && t[v + 2] == 'l' && t[v + 3] == 'l') ||
                   (c == 't' && t[v + 1] == 'r' && t[v + 2] == 'u' && t[v + 3] == 'e')))
      continue;
    if (w == 5 && c == 'f' && t[v + 1] == 'a' && t[v + 2] == 'l' && t[v + 3] == 's' && t[v + 4] == 'e') continue;
    const uint64_t q = v + (c == '-' ? 1 : 0), digits = p - q;
    if (digits == 0 || digits > 18) return false;
    for (uint64_t j = q; j < p; ++j)
      if (t[j] < '0' || t[j] > '9') return false;
    if (t[q] == '0' && (digits > 1 || c == '-')) return false;  // leading zero, -0
  }
  return nsl_space(t, p, n) == n;
}

}  // namespace edv
