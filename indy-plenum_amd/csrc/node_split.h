// node_split.h -- the strict parse that cuts a BATCH's member strings out of an rxMsgs entry
// (_hostpack.gather_node_texts; also compiled into the sanitizer corpus runner).  Host only.
//
// A BATCH ({"op":"BATCH","messages":["<json text>", ...],"signature":null}; Batched._make_batch,
// plenum/common/batched.py:141-144) carries its messages as JSON strings.  node_split cuts the
// string bodies out -- still escaped: the GPU unescapes them (csrc/wire_unwrap.h) -- when the entry
// parses strictly as
//   { "op" : "BATCH" , "messages" : [ string (, string)* | empty ]
//     (, key : null | true | false | -?(0|[1-9][0-9]*) of at most 18 digits | string without backslash)* }
// with JSON whitespace between tokens and only whitespace after the brace; every byte 0x20-0x7e;
// no backslash in a key, no later key "op" or "messages"; every escape in a member one of
// \" \\ \/ \b \f \n \r \t.  Such an entry is one json.loads accepts, and the unescaped bodies are
// the strings its "messages" holds.  Correctness never depends on the recognition: any other entry
// goes to the GPU whole, where a BATCH is classed "the host decides".
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace edv {

struct NodeSpan {
  uint64_t at, len;
};

inline size_t ns_space(const uint8_t* t, size_t p, size_t n) {
  while (p < n && (t[p] == ' ' || t[p] == '\t' || t[p] == '\n' || t[p] == '\r')) ++p;
  return p;
}

// t[p .. p + k) == word, with the closing quote after it
inline bool ns_word(const uint8_t* t, size_t p, size_t n, const char* word, size_t k) {
  return p + k < n && memcmp(t + p, word, k) == 0 && t[p + k] == '"';
}

// The member bodies of the BATCH t[0 .. n) appended to out; false (out as it was): not split.
inline bool node_split(const uint8_t* t, size_t n, std::vector<NodeSpan>& out) {
  const size_t mark = out.size();
  const auto no = [&] {
    out.resize(mark);
    return false;
  };
  for (size_t i = 0; i < n; ++i)
    if (t[i] < 0x20 || t[i] > 0x7e) return false;
  size_t p = ns_space(t, 0, n);
  if (p >= n || t[p] != '{') return false;
  p = ns_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !ns_word(t, p + 1, n, "op", 2)) return false;
  p = ns_space(t, p + 4, n);
  if (p >= n || t[p] != ':') return false;
  p = ns_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !ns_word(t, p + 1, n, "BATCH", 5)) return false;
  p = ns_space(t, p + 7, n);
  if (p >= n || t[p] != ',') return false;
  p = ns_space(t, p + 1, n);
  if (p >= n || t[p] != '"' || !ns_word(t, p + 1, n, "messages", 8)) return false;
  p = ns_space(t, p + 10, n);
  if (p >= n || t[p] != ':') return false;
  p = ns_space(t, p + 1, n);
  if (p >= n || t[p] != '[') return false;
  p = ns_space(t, p + 1, n);
  if (p < n && t[p] == ']') {
    ++p;
  } else {
    for (;;) {
      if (p >= n || t[p] != '"') return no();
      const size_t a = ++p;
      for (;; ++p) {
        if (p >= n) return no();
        const uint8_t c = t[p];
        if (c == '"') break;
        if (c == '\\') {
          if (++p >= n) return no();
          const uint8_t e = t[p];
          if (e != '"' && e != '\\' && e != '/' && e != 'b' && e != 'f' && e != 'n' && e != 'r' && e != 't') return no();
        }
      }
      out.push_back(NodeSpan{a, p - a});
      p = ns_space(t, p + 1, n);
      if (p >= n) return no();
      const uint8_t d = t[p];
      p = ns_space(t, p + 1, n);
      if (d == ']') break;
      if (d != ',') return no();
    }
  }
  for (;;) {  // p: after the value and its whitespace
    p = ns_space(t, p, n);
    if (p >= n) return no();
    const uint8_t d = t[p++];
    if (d == '}') break;
    if (d != ',') return no();
    p = ns_space(t, p, n);
    if (p >= n || t[p] != '"') return no();
    const size_t k = ++p;
    for (;; ++p) {
      if (p >= n) return no();
      if (t[p] == '"') break;
      if (t[p] == '\\') return no();
    }
    if ((p - k == 2 && memcmp(t + k, "op", 2) == 0) || (p - k == 8 && memcmp(t + k, "messages", 8) == 0)) return no();
    p = ns_space(t, p + 1, n);
    if (p >= n || t[p] != ':') return no();
    p = ns_space(t, p + 1, n);
    if (p >= n) return no();
    const uint8_t c = t[p];
    if (c == '"') {
      for (++p;; ++p) {
        if (p >= n || t[p] == '\\') return no();
        if (t[p] == '"') break;
      }
      ++p;
      continue;
    }
    const size_t v = p;
    while (p < n && t[p] != ' ' && t[p] != ',' && t[p] != '}' && t[p] != ']') ++p;
    const size_t w = p - v;
    if ((w == 4 && (memcmp(t + v, "null", 4) == 0 || memcmp(t + v, "true", 4) == 0)) ||
        (w == 5 && memcmp(t + v, "false", 5) == 0))
      continue;
    size_t q = v + (c == '-' ? 1 : 0);
    const size_t digits = p - q;
    if (digits == 0 || digits > 18) return no();
    for (size_t j = q; j < p; ++j)
      if (t[j] < '0' || t[j] > '9') return no();
    if (t[q] == '0' && (digits > 1 || c == '-')) return no();  // leading zero, -0
  }
  if (ns_space(t, p, n) != n) return no();
  return true;
}

}  // namespace edv
