// wire_corpus_check.cpp -- TEST INFRASTRUCTURE: the wire scanner (wire_scan.h, the lane code of
// edv_wire_scan_kernel) over a corpus file on the host CPU, as a stand-alone program meant to
// be built with -fsanitize=address,undefined (Makefile target wire-corpus-check).  Every text is
// copied into a heap block of exactly its length and scanned into another of the same length, so
// a read or write one byte outside either is reported.  Then the corpus as one wire batch -- the
// texts back to back in a heap block of exactly their total length -- through the identifier pass
// (wire_idents.h, the lane code of edv_wire_ident_*_kernel) with a table of 2 n slots and again
// with one just large enough, whose chains wrap.
//
// --node: the corpus is rxMsgs entries of a node stack.  Every entry, in a heap block of exactly
// its length, goes through the BATCH parse (node_split.h); every message that yields -- a member
// body, or the entry whole -- is copied into a block of exactly its length and unwrapped
// (wire_unwrap.h, the lane code of edv_wire_unwrap_kernel) into another, and the result is
// scanned.  Every entry is also unwrapped whole both as plain text and as an escaped body, and goes
// through the device split's lane code as an emulated wave (node_split_lanes.h,
// node_split_wave_host.h: what edv_node_split_count_kernel and edv_node_split_emit_kernel run), at
// the place in the buffer the entries before it give it; the verdict, the member count, the body
// bytes and every member's span must equal node_split's.
//
// Corpus file: per text a little-endian uint32 length, then the bytes
// (tools/wire_probe.py --write-corpus FILE / --write-node-corpus FILE write the test corpora).
// Prints the counts; exit status 0 unless the file is malformed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "node_split.h"
#include "node_split_wave_host.h"
#include "wire_idents.h"
#include "wire_scan.h"
#include "wire_unwrap.h"

namespace {
struct SerialTable {  // the device's atomics, one item at a time
  uint32_t* owner;
  uint32_t* first;
  uint32_t owner_load(uint32_t s) const { return owner[s]; }
  uint32_t owner_cas(uint32_t s, uint32_t i) const {
    const uint32_t was = owner[s];
    if (was == edv::kIdentEmpty) owner[s] = i;
    return was;
  }
  uint32_t first_load(uint32_t s) const { return first[s]; }
  void first_min(uint32_t s, uint32_t i) const {
    if (i < first[s]) first[s] = i;
  }
};

// The number of distinct identifiers of the status-0 items, or -1 when the table is too small.
long idents(const uint8_t* text, const std::vector<uint64_t>& off, const std::vector<uint8_t>& status,
            const std::vector<uint32_t>& span, uint64_t cap) {
  const uint64_t n = status.size();
  uint32_t* owner = (uint32_t*)malloc(cap * 4);  // (heap blocks of the exact size, as the texts)
  uint32_t* first = (uint32_t*)malloc(cap * 4);
  uint32_t* slot = (uint32_t*)malloc((n ? n : 1) * 4);
  memset(owner, 0xff, cap * 4);
  memset(first, 0xff, cap * 4);
  long nu = 0;
  for (uint64_t k = 0; k < n && nu >= 0; ++k) {
    const uint64_t i = n - 1 - k;  // (any order gives the same answer: the last item first)
    slot[i] = edv::kIdentEmpty;
    if (status[i] != 0 || !edv::wi_span_ok(off.data(), span.data(), i)) continue;
    slot[i] = edv::wi_insert(text, off.data(), span.data(), SerialTable{owner, first}, (uint32_t)cap, (uint32_t)i);
    if (slot[i] == edv::kIdentEmpty) nu = -1;
  }
  for (uint64_t i = 0; i < n && nu >= 0; ++i) nu += edv::wi_flag(slot, first, i);
  free(owner);
  free(first);
  free(slot);
  return nu;
}
// One message through the unwrap and the scan, each buffer a heap block of exactly len bytes.
struct NodeCounts {
  uint64_t cls[3] = {0, 0, 0}, scanned = 0;
};
bool unwrap_message(const uint8_t* body, uint32_t len, uint32_t esc, NodeCounts& c) {
  uint8_t* text = (uint8_t*)malloc(len ? len : 1);
  uint8_t* mid = (uint8_t*)malloc(len ? len : 1);
  uint8_t* out = (uint8_t*)malloc(len ? len : 1);
  memcpy(text, body, len);
  const int cls = edv::wire_unwrap_one((const uint8_t*)text, len, esc, mid);
  bool ok = cls >= 0 && cls <= 2;
  if (ok) {
    ++c.cls[cls];
    if (len <= edv::kWireMaxText) {
      edv::WireItem it;
      memset(&it, 0, sizeof it);
      const int st = edv::wire_scan_one((const uint8_t*)mid, len, out, it);
      if (st == edv::kWireOk) {
        ++c.scanned;
        ok = cls == edv::kUnwrapRequest && it.msg_len <= len && (uint64_t)it.idr_start + it.idr_len <= len;
      }
    }
  }
  free(text);
  free(mid);
  free(out);
  return ok;
}

// The entry at [ea, ea + len) of the buffer through the emulated wave, against node_split's answer.
bool lanes_equal(const uint8_t* entry, uint64_t ea, uint64_t len, bool split, const std::vector<edv::NodeSpan>& spans) {
  const edv::EntryCount c = edv::lanes_count(entry, ea, ea + len);
  uint64_t bytes = 0;
  for (const edv::NodeSpan& s : spans) bytes += s.len;
  if (c.split != split || c.members != (split ? spans.size() : 1) || c.bytes != (split ? bytes : len)) return false;
  if (!split) return true;
  uint64_t seen = 0, body = 0;
  bool ok = true;
  std::vector<uint8_t> met(spans.size(), 0);
  edv::lanes_emit(entry, ea, ea + len, [&](uint64_t index, uint64_t at_body, uint64_t first) {
    ok = ok && index < spans.size() && !met[index] && first == ea + spans[index].at;
    if (!ok) return;
    met[index] = 1;
    uint64_t before = 0;
    for (uint64_t j = 0; j < index; ++j) before += spans[j].len;
    ok = at_body == before;
    ++seen;
    body += spans[index].len;
  });
  return ok && seen == spans.size() && body == bytes;
}

int node_main(FILE* f) {
  uint64_t entries = 0, split = 0, messages = 0, at = 0, lane_split = 0, lane_members = 0;
  NodeCounts as_cut, whole, escaped;
  for (;;) {
    uint8_t hdr[4];
    const size_t got = fread(hdr, 1, 4, f);
    if (got == 0) break;
    if (got != 4) {
      fprintf(stderr, "truncated length\n");
      return 1;
    }
    const uint32_t len = (uint32_t)hdr[0] | (uint32_t)hdr[1] << 8 | (uint32_t)hdr[2] << 16 | (uint32_t)hdr[3] << 24;
    if (len > (64u << 20)) {
      fprintf(stderr, "implausible length %u\n", len);
      return 1;
    }
    uint8_t* entry = (uint8_t*)malloc(len ? len : 1);
    if (!entry || fread(entry, 1, len, f) != len) {
      fprintf(stderr, "truncated entry\n");
      return 1;
    }
    ++entries;
    std::vector<edv::NodeSpan> spans;
    bool ok = true;
    const bool is_split = edv::node_split(entry, len, spans);
    if (!lanes_equal(entry, at, len, is_split, spans)) {
      fprintf(stderr, "entry %llu: the lane code and node_split disagree\n", (unsigned long long)entries);
      return 1;
    }
    at += len;
    lane_split += is_split;
    lane_members += is_split ? spans.size() : 0;
    if (is_split) {
      ++split;
      for (const edv::NodeSpan& s : spans) {
        ok = ok && s.at + s.len <= len && unwrap_message(entry + s.at, (uint32_t)s.len, 1, as_cut);
        ++messages;
      }
    } else {
      ok = spans.empty() && unwrap_message(entry, len, 0, as_cut);
      ++messages;
    }
    ok = ok && unwrap_message(entry, len, 0, whole) && unwrap_message(entry, len, 1, escaped);
    free(entry);
    if (!ok) {
      fprintf(stderr, "entry %llu: a result outside its message\n", (unsigned long long)entries);
      return 1;
    }
  }
  printf("entries %llu split %llu messages %llu\n", (unsigned long long)entries, (unsigned long long)split,
         (unsigned long long)messages);
  printf("lane code: split %llu members %llu, equal to node_split on every entry\n", (unsigned long long)lane_split,
         (unsigned long long)lane_members);
  const NodeCounts* rows[3] = {&as_cut, &whole, &escaped};
  const char* names[3] = {"as cut", "entries whole", "entries as escaped bodies"};
  for (int k = 0; k < 3; ++k)
    printf("%s: request %llu host %llu none %llu scanned %llu\n", names[k], (unsigned long long)rows[k]->cls[0],
           (unsigned long long)rows[k]->cls[1], (unsigned long long)rows[k]->cls[2], (unsigned long long)rows[k]->scanned);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const bool node = argc == 3 && strcmp(argv[1], "--node") == 0;
  if (argc != 2 && !node) {
    fprintf(stderr, "usage: %s [--node] CORPUS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[argc - 1], "rb");
  if (!f) {
    perror(argv[argc - 1]);
    return 2;
  }
  if (node) {
    const int r = node_main(f);
    fclose(f);
    return r;
  }
  uint64_t texts = 0, scanned = 0, host = 0, out_bytes = 0;
  std::vector<uint8_t> all, status;
  std::vector<uint64_t> off(1, 0);
  std::vector<uint32_t> span;
  for (;;) {
    uint8_t hdr[4];
    const size_t got = fread(hdr, 1, 4, f);
    if (got == 0) break;
    if (got != 4) {
      fprintf(stderr, "truncated length\n");
      return 1;
    }
    const uint32_t len = (uint32_t)hdr[0] | (uint32_t)hdr[1] << 8 | (uint32_t)hdr[2] << 16 | (uint32_t)hdr[3] << 24;
    if (len > (64u << 20)) {
      fprintf(stderr, "implausible length %u\n", len);
      return 1;
    }
    uint8_t* text = (uint8_t*)malloc(len ? len : 1);
    uint8_t* out = (uint8_t*)malloc(len ? len : 1);
    if (!text || !out || fread(text, 1, len, f) != len) {
      fprintf(stderr, "truncated text\n");
      return 1;
    }
    edv::WireItem it;
    memset(&it, 0, sizeof it);
    const int st = edv::wire_scan_one((const uint8_t*)text, len, out, it);
    ++texts;
    if (st == edv::kWireOk) {
      ++scanned;
      out_bytes += it.msg_len;
      if (it.msg_len > len || (uint64_t)it.idr_start + it.idr_len > len) {
        fprintf(stderr, "text %llu: result outside the text\n", (unsigned long long)texts);
        return 1;
      }
    } else {
      ++host;
    }
    all.insert(all.end(), text, text + len);
    off.push_back(all.size());
    status.push_back((uint8_t)st);
    span.push_back(st == edv::kWireOk ? it.idr_start : 0);
    span.push_back(st == edv::kWireOk ? it.idr_len : 0);
    free(text);
    free(out);
  }
  fclose(f);
  printf("texts %llu scanned %llu host %llu serialized bytes %llu\n", (unsigned long long)texts,
         (unsigned long long)scanned, (unsigned long long)host, (unsigned long long)out_bytes);
  uint8_t* batch = (uint8_t*)malloc(all.size() ? all.size() : 1);
  memcpy(batch, all.data(), all.size());
  uint64_t cap = 64;
  while (cap < 2 * texts) cap <<= 1;
  const long nu = idents(batch, off, status, span, cap);
  uint64_t tight = 1;
  while ((long)tight < nu) tight <<= 1;
  const long nu_tight = idents(batch, off, status, span, tight);
  free(batch);
  printf("identifiers %ld (table of %llu slots) %ld (of %llu)\n", nu, (unsigned long long)cap, nu_tight,
         (unsigned long long)tight);
  if (nu < 0 || nu_tight != nu) {
    fprintf(stderr, "the identifier pass disagrees with itself\n");
    return 1;
  }
  return 0;
}
